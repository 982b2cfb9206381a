// C-ABI of libgmupt.so: adaptive sampling on the device (gmupt_adaptive_*, pt_adaptive.hip) and the render loop that plans as it goes.
#include "gmupt_internal.hpp"

extern "C" int gmupt_adaptive_create(gmupt_renderer* r, gmupt_adaptive** out)
{
    if (out) *out = nullptr;
    if (!r || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_adaptive_create: null argument");
    gmupt_adaptive* a = new (std::nothrow) gmupt_adaptive();
    if (!a) return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_adaptive_create: out of host memory");
    a->r = r;
    *out = a;
    return GMUPT_OK;
}

extern "C" void gmupt_adaptive_destroy(gmupt_adaptive* a)
{
    if (!a) return;
    if (a->r->adaptive == a) a->r->adaptive = nullptr;
    (void)hipSetDevice(a->r->dev->id);
    (void)hipStreamSynchronize(a->r->stream);
    delete a;
}

extern "C" int gmupt_renderer_set_adaptive(gmupt_renderer* r, gmupt_adaptive* a)
{
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_set_adaptive: null renderer");
    if (a && a->r != r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_set_adaptive: the plan belongs to another renderer");
    r->adaptive = a;
    return GMUPT_OK;
}

// The allocation for `pixels` pixels and `cap` entries, carved; the only place that allocates.  Grown, never shrunk: a smaller plan
// is carved afresh over the front of it.
static int adaptive_room(gmupt_adaptive* a, size_t pixels, size_t cap)
{
    if (cap == 0) cap = 1;
    if (a->mem.ptr && a->pixels == pixels && a->cap == cap) return GMUPT_OK;
    GMUPT_TRY(a->mem.grow(a->r->stream, adaptive_carve(nullptr, pixels, cap, nullptr)));   // waits for the stream before it frees
    adaptive_carve(a->mem.ptr, pixels, cap, &a->sc);
    a->pixels = pixels; a->cap = cap;
    return GMUPT_OK;
}

// gmupt_adaptive_select with checked arguments
static int adaptive_select(gmupt_adaptive* a, const float* error, uint32_t W, uint32_t H, const AdParams& prm, uint32_t uniformEvery, gmupt_adaptive_info* info)
{
    gmupt_renderer* r = a->r;
    const size_t n = (size_t)W * H;
    HIP_TRY(hipSetDevice(r->dev->id));
    if (a->pixels != n || a->cap != n * prm.maxRepeat) a->count = 0;     // the list is about to move: an attached plan re-aims nothing meanwhile
    GMUPT_TRY(adaptive_room(a, n, n * prm.maxRepeat));
    GMUPT_TRY(a->ev.start(r->stream));
    const AdPartial* last = launch_adaptive_select(error, n, prm, a->sc, a->cap, r->stream);
    HIP_TRY(hipGetLastError());
    GMUPT_TRY(a->ev.stop(r->stream));
    AdPartial total;
    GMUPT_TRY(copy_sync(&total, last, sizeof(total), hipMemcpyDeviceToHost, r->stream));   // the one synchronisation
    float ms = 0.0f;
    GMUPT_TRY(a->ev.elapsed_ms(&ms));
    a->W = W; a->H = H; a->count = total.entries; a->uniformEvery = uniformEvery; a->generation = r->accumGeneration;
    if (info) { ad_fill_info(total, (uint32_t)n, info); info->ms = (double)ms; }
    return GMUPT_OK;
}

// the size checks of a plan's rectangle under max_repeat (1 for a caller's list)
static int adaptive_rect(const char* fn, uint32_t W, uint32_t H, uint32_t maxRepeat)
{
    const uint64_t n = (uint64_t)W * H;
    if (n == 0 || n > 0xFFFFFFFFull) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: rectangle of %ux%u (1 .. 2^32 - 1 pixels)", fn, W, H);
    if (n * maxRepeat > kAdMaxEntries) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: %ux%u pixels at max_repeat = %u are more than 2^28 entries", fn, W, H, maxRepeat);
    return GMUPT_OK;
}

extern "C" int gmupt_adaptive_select(gmupt_adaptive* a, const float* device_error, uint32_t width, uint32_t height, const gmupt_adaptive_params* params,
                                     gmupt_adaptive_info* info)
{
    const char* fn = "gmupt_adaptive_select";
    if (!a || !device_error || !info) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null handle, error plane or info", fn);
    if ((uintptr_t)device_error & 3u) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: misaligned error plane (4 bytes)", fn);
    AdParams prm;
    GMUPT_TRY(adaptive_params(fn, params, 0.0f, prm));
    GMUPT_TRY(adaptive_rect(fn, width, height, prm.maxRepeat));
    return adaptive_select(a, device_error, width, height, prm, params->uniform_every, info);
}

extern "C" int gmupt_adaptive_set_list(gmupt_adaptive* a, const uint32_t* host_list, uint32_t count, uint32_t width, uint32_t height, uint32_t uniform_every)
{
    const char* fn = "gmupt_adaptive_set_list";
    if (!a || (!host_list && count)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null handle or list", fn);
    GMUPT_TRY(adaptive_rect(fn, width, height, 1));
    if (count > kAdMaxEntries) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: %u entries (at most 2^28)", fn, count);
    const uint64_t n = (uint64_t)width * height;
    for (uint32_t i = 0; i < count; i++)
        if (host_list[i] >= n) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: entry %u is pixel %u of a %ux%u rectangle", fn, i, host_list[i], width, height);
    gmupt_renderer* r = a->r;
    HIP_TRY(hipSetDevice(r->dev->id));
    a->count = 0;
    HIP_TRY(hipStreamSynchronize(r->stream));            // a launch may still read the list this one replaces
    GMUPT_TRY(adaptive_room(a, (size_t)n, count));
    if (count) GMUPT_TRY(copy_sync(a->sc.list, host_list, (size_t)count * 4, hipMemcpyHostToDevice, r->stream));
    a->W = width; a->H = height; a->count = count; a->uniformEvery = uniform_every; a->generation = r->accumGeneration;
    return GMUPT_OK;
}

extern "C" int gmupt_adaptive_read_list(gmupt_adaptive* a, uint32_t* dst, size_t bytes, uint32_t* count)
{
    const char* fn = "gmupt_adaptive_read_list";
    if (!a || (!dst && !count)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    if (dst) {
        if (bytes < (size_t)a->count * 4) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: %zu bytes given, %zu needed", fn, bytes, (size_t)a->count * 4);
        HIP_TRY(hipSetDevice(a->r->dev->id));
        if (a->count) GMUPT_TRY(copy_sync(dst, a->sc.list, (size_t)a->count * 4, hipMemcpyDeviceToHost, a->r->stream));
    }
    if (count) *count = a->count;
    return GMUPT_OK;
}

extern "C" int gmupt_render_adaptive(gmupt_renderer* r, gmupt_camera* cam, gmupt_converge* c, gmupt_adaptive* a, const gmupt_converge_params* cparams,
                                     const gmupt_adaptive_params* aparams, uint32_t check_every, uint32_t max_iterations, uint32_t* iters,
                                     gmupt_converge_info* cinfo, gmupt_adaptive_info* ainfo)
{
    const char* fn = "gmupt_render_adaptive";
    if (!r || !cam || !c || !a || !cinfo) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    if (c->r != r || a->r != r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: the monitor or the plan belongs to another renderer", fn);
    if (check_every == 0) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: check_every = 0", fn);
    CvParams cprm;
    GMUPT_TRY(converge_params(fn, cparams, cprm));
    AdParams aprm;
    GMUPT_TRY(adaptive_params(fn, aparams, cprm.threshold, aprm));
    GMUPT_TRY(adaptive_rect(fn, r->p.fbW, r->p.fbH, aprm.maxRepeat));
    HIP_TRY(hipSetDevice(r->dev->id));
    const size_t n = (size_t)r->p.fbW * r->p.fbH;
    GMUPT_TRY(a->errPlane.grow(r->stream, n * sizeof(float)));
    r->adaptive = nullptr;                               // the loop starts without a plan: it has no error plane of this frame yet
    uint32_t k = 0;
    int rc = GMUPT_OK;
    gmupt_converge_info last{};
    gmupt_adaptive_info lastPlan{};
    bool checked = false, planned = false;
    while (k < max_iterations) {
        cam->cam.update(0.0f);                       // as gmupt_render_until
        const gmupt_camera_buffer* cb = cam->cam.getBuffer();
        if (r->adaptive && (cb->iterationCounter == 0 || a->generation != r->accumGeneration)) r->adaptive = nullptr;   // a restarted frame
        rc = gmupt_set_camera(r, cb);
        if (rc == GMUPT_OK) rc = gmupt_iterate(r);
        if (rc != GMUPT_OK) break;
        k++;
        if (k % check_every) continue;
        rc = gmupt_converge_update(c, cparams, a->errPlane.as<float>(), &last);   // synchronises
        if (rc == GMUPT_OK) rc = gmupt_synchronize(r);           // the sticky ray-cast flags
        if (rc != GMUPT_OK) break;
        checked = true;
        if (last.converged) break;
        rc = adaptive_select(a, a->errPlane.as<float>(), r->p.fbW, r->p.fbH, aprm, aparams->uniform_every, &lastPlan);
        if (rc != GMUPT_OK) break;
        planned = true;
        r->adaptive = a;
    }
    r->adaptive = nullptr;
    if (rc == GMUPT_OK) rc = gmupt_synchronize(r);
    if (iters) *iters = k;
    if (rc == GMUPT_OK && checked) *cinfo = last;
    if (rc == GMUPT_OK && planned && ainfo) *ainfo = lastPlan;
    return rc;
}
