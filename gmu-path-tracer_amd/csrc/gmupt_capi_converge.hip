// C-ABI of libgmupt.so: the convergence monitor on the device (gmupt_converge_*, pt_converge.hip) and the render loop that stops on it.
#include "gmupt_internal.hpp"

extern "C" int gmupt_converge_create(gmupt_renderer* r, gmupt_converge** out)
{
    if (out) *out = nullptr;
    if (!r || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_converge_create: null argument");
    gmupt_converge* c = new (std::nothrow) gmupt_converge();
    if (!c) return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_converge_create: out of host memory");
    c->r = r;
    *out = c;
    return GMUPT_OK;
}

extern "C" void gmupt_converge_destroy(gmupt_converge* c)
{
    if (!c) return;
    (void)hipSetDevice(c->r->dev->id);
    (void)hipStreamSynchronize(c->r->stream);
    delete c;
}

// every pixel back to the initial state, on the stream
static int converge_zero(gmupt_converge* c)
{
    if (c->mem.ptr) HIP_TRY(hipMemsetAsync(c->mem.ptr, 0, converge_state_bytes((size_t)c->W * c->H), c->r->stream));
    return GMUPT_OK;
}

extern "C" int gmupt_converge_reset(gmupt_converge* c)
{
    if (!c) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_converge_reset: null handle");
    HIP_TRY(hipSetDevice(c->r->dev->id));
    return converge_zero(c);
}

// What both updates do once their arguments are checked: (re)allocates for the image size, zeroes on `restart`, enqueues the levels,
// reads the one partial back.  The only place that allocates.
static int converge_run(gmupt_converge* c, const float* rgba, uint32_t W, uint32_t H, const CvParams& prm, bool restart, float* error,
                        gmupt_converge_info* info)
{
    gmupt_renderer* r = c->r;
    const size_t n = (size_t)W * H;
    HIP_TRY(hipSetDevice(r->dev->id));
    if (!c->mem.ptr || W != c->W || H != c->H) {
        HIP_TRY(hipStreamSynchronize(r->stream));   // a launch may still use the allocation this one replaces
        DevMem m;
        GMUPT_TRY(m.alloc(converge_carve(nullptr, n, nullptr), 0, r->stream));
        c->mem = std::move(m);
        c->W = W; c->H = H;
        converge_carve(c->mem.ptr, n, &c->pl);
    } else if (restart) {
        GMUPT_TRY(converge_zero(c));
    }
    GMUPT_TRY(c->ev.start(r->stream));
    const CvPartial* last = launch_converge(reinterpret_cast<const float4*>(rgba), n, c->pl, prm, error, r->stream);
    HIP_TRY(hipGetLastError());
    GMUPT_TRY(c->ev.stop(r->stream));
    CvPartial total;
    GMUPT_TRY(copy_sync(&total, last, sizeof(total), hipMemcpyDeviceToHost, r->stream));   // the one synchronisation
    float ms = 0.0f;
    GMUPT_TRY(c->ev.elapsed_ms(&ms));
    cv_fill_info(total, (uint32_t)n, prm, info);
    info->ms = (double)ms;
    return GMUPT_OK;
}

// gmupt_converge_update with checked arguments: the accumulation target, restarted when it is not the accumulation the state belongs to
static int converge_update(gmupt_converge* c, const CvParams& prm, float* error, gmupt_converge_info* info)
{
    gmupt_renderer* r = c->r;
    const bool restart = !c->seen || c->generation != r->accumGeneration;
    GMUPT_TRY(converge_run(c, reinterpret_cast<const float*>(r->p.fb), r->p.fbW, r->p.fbH, prm, restart, error, info));
    c->seen = true; c->generation = r->accumGeneration;
    return GMUPT_OK;
}

extern "C" int gmupt_converge_update(gmupt_converge* c, const gmupt_converge_params* params, float* device_error_or_null, gmupt_converge_info* info)
{
    const char* fn = "gmupt_converge_update";
    if (!c || !info) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null handle or info", fn);
    if ((uintptr_t)device_error_or_null & 3u) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: misaligned error plane (4 bytes)", fn);
    CvParams prm;
    GMUPT_TRY(converge_params(fn, params, prm));
    return converge_update(c, prm, device_error_or_null, info);
}

extern "C" int gmupt_converge_update_image(gmupt_converge* c, const float* device_rgba, uint32_t width, uint32_t height, const gmupt_converge_params* params,
                                           float* device_error_or_null, gmupt_converge_info* info)
{
    const char* fn = "gmupt_converge_update_image";
    if (!c || !device_rgba || !info) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null handle, image or info", fn);
    if ((uintptr_t)device_rgba & 15u) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: misaligned image (16 bytes)", fn);
    if ((uintptr_t)device_error_or_null & 3u) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: misaligned error plane (4 bytes)", fn);
    const uint64_t n = (uint64_t)width * height;
    if (n == 0 || n > 0xFFFFFFFFull) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: image of %ux%u (1 .. 2^32 - 1 pixels)", fn, width, height);
    CvParams prm;
    GMUPT_TRY(converge_params(fn, params, prm));
    GMUPT_TRY(converge_run(c, device_rgba, width, height, prm, false, device_error_or_null, info));
    c->seen = false;   // the state no longer belongs to an accumulation of the renderer
    return GMUPT_OK;
}

extern "C" int gmupt_converge_read_state(gmupt_converge* c, gmupt_converge_pixel* dst, size_t bytes)
{
    const char* fn = "gmupt_converge_read_state";
    if (!c || !dst) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    const size_t n = c->mem.ptr ? (size_t)c->W * c->H : 0;
    if (bytes < n * sizeof(gmupt_converge_pixel)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: %zu bytes given, %zu needed", fn, bytes, n * sizeof(gmupt_converge_pixel));
    if (n == 0) return GMUPT_OK;
    HIP_TRY(hipSetDevice(c->r->dev->id));
    const size_t stateBytes = converge_state_bytes(n);
    std::vector<char> host;
    try { host.resize(stateBytes); } catch (const std::bad_alloc&) { return fail(GMUPT_ERR_OUT_OF_MEMORY, "%s: out of host memory for %zu pixels", fn, n); }
    GMUPT_TRY(copy_sync(host.data(), c->mem.ptr, stateBytes, hipMemcpyDeviceToHost, c->r->stream));
    CvPlanes pl;
    converge_carve(host.data(), n, &pl);   // the same parts over the host copy
    for (size_t i = 0; i < n; i++) dst[i] = gmupt_converge_pixel{ pl.n[i], pl.k[i], pl.w[i], 0u, pl.s[i], pl.mean[i], pl.m2[i] };
    return GMUPT_OK;
}

extern "C" int gmupt_render_until(gmupt_renderer* r, gmupt_camera* cam, gmupt_converge* c, const gmupt_converge_params* params, uint32_t check_every,
                                  uint32_t max_iterations, uint32_t* iters, gmupt_converge_info* info)
{
    const char* fn = "gmupt_render_until";
    if (!r || !cam || !c || !info) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    if (c->r != r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: the monitor belongs to another renderer", fn);
    if (check_every == 0) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: check_every = 0", fn);
    CvParams prm;
    GMUPT_TRY(converge_params(fn, params, prm));
    uint32_t k = 0;
    int rc = GMUPT_OK;
    gmupt_converge_info last{};
    bool checked = false;
    while (k < max_iterations) {
        cam->cam.update(0.0f);                       // as gmupt_render_budget: Renderer::update, then Renderer::draw
        rc = gmupt_set_camera(r, cam->cam.getBuffer());
        if (rc == GMUPT_OK) rc = gmupt_iterate(r);
        if (rc != GMUPT_OK) break;
        k++;
        if (k % check_every) continue;
        rc = converge_update(c, prm, nullptr, &last);            // synchronises
        if (rc == GMUPT_OK) rc = gmupt_synchronize(r);           // the sticky ray-cast flags
        if (rc != GMUPT_OK) break;
        checked = true;
        if (last.converged) break;
    }
    if (rc == GMUPT_OK) rc = gmupt_synchronize(r);
    if (iters) *iters = k;
    if (rc == GMUPT_OK && checked) *info = last;
    return rc;
}
