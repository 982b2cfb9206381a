// C-ABI of libgmupt.so: the spatial denoiser on device images and the temporal-reuse handle.
#include "gmupt_internal.hpp"

extern "C" int gmupt_denoise_image(gmupt_renderer* r, const float* beauty_rgba, const gmupt_aov* aov, uint32_t width, uint32_t height,
                                   const gmupt_denoise_params* p, float* out_rgba, size_t out_bytes, float* ms)
{
    if (ms) *ms = 0.0f;
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_denoise_image: null renderer");
    DnParams prm;
    GMUPT_TRY(image_args("gmupt_denoise_image", beauty_rgba, aov, width, height, out_rgba, out_bytes, true));
    GMUPT_TRY(denoise_params("gmupt_denoise_image", p, prm));
    HIP_TRY(hipSetDevice(r->dev->id));
    GMUPT_TRY(r->dnScratch.grow(r->stream, (size_t)width * height * kGdScratchBytes));
    GMUPT_TRY(r->dnEv.start(r->stream));
    launch_denoise(reinterpret_cast<const float4*>(beauty_rgba), reinterpret_cast<const float4*>(aov), (int)width, (int)height, prm, r->dnScratch.ptr,
                   reinterpret_cast<float4*>(out_rgba), r->stream);
    HIP_TRY(hipGetLastError());
    GMUPT_TRY(r->dnEv.stop(r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    float t = 0.0f;
    GMUPT_TRY(r->dnEv.elapsed_ms(&t));
    if (ms) *ms = t;
    return GMUPT_OK;
}

// What the render_denoised* chains check once they have a renderer, in this order: the output, the caller's parameters (`params`, which
// has called fail() itself), then what gmupt_render_aovs would refuse, before the scratch is grown for it.  Leaves the device set.
template <class P> static int render_args(const char* fn, gmupt_renderer* r, uint32_t aov_samples, const float* out_rgba, size_t bytes, const P& params, bool centre = true)
{
    const uint32_t W = r->p.fbW, H = r->p.fbH;
    if (!out_rgba || ((uintptr_t)out_rgba & 15u)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null or misaligned output (16 bytes)", fn);
    if (bytes < (size_t)W * H * 16) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: %zu output bytes for %ux%u RGBA32F texels", fn, bytes, W, H);
    GMUPT_TRY(params());
    if (!r->sceneBound) return fail(GMUPT_ERR_NOT_BOUND, "%s: no scene bound", fn);
    if (!r->cameraSet) return fail(GMUPT_ERR_NOT_BOUND, "%s: no camera set", fn);
    GMUPT_TRY(aov_sample_plan(fn, "aov_samples", W, aov_samples, nullptr, centre));
    GMUPT_TRY(query_supported(r, fn));
    HIP_TRY(hipSetDevice(r->dev->id));
    return GMUPT_OK;
}

// gmupt_render_denoised; with `infill` gmupt_render_preview without a history: the infill stage between the framebuffer copy and the filter;
// with `guides` gmupt_render_denoised_lens / gmupt_render_denoised_projected: the records are what it renders (AovGuides, gmupt_internal.hpp)
int render_denoised(const char* fn, gmupt_renderer* r, uint32_t aov_samples, const gmupt_denoise_params* p, const IfParams* infill, float* out_rgba, size_t bytes,
                    gmupt_trace_info* info, const AovGuides& guides)
{
    if (info) std::memset(info, 0, sizeof(*info));
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null renderer", fn);
    const uint32_t W = r->p.fbW, H = r->p.fbH;
    DnParams prm;
    GMUPT_TRY(render_args(fn, r, aov_samples, out_rgba, bytes, [&] { return denoise_params(fn, p, prm); }, !guides));
    GMUPT_TRY(r->dnInput.grow(r->stream, (size_t)W * H * (sizeof(gmupt_aov) + 16)));
    if (infill) GMUPT_TRY(r->ifImage.grow(r->stream, (size_t)W * H * 16));
    gmupt_aov* aov = r->dnInput.as<gmupt_aov>();
    const float* beauty = reinterpret_cast<float*>(r->dnInput.as<char>() + (size_t)W * H * sizeof(gmupt_aov));
    gmupt_trace_info ai;
    const size_t aovBytes = (size_t)W * H * sizeof(gmupt_aov);
    int rc = guides ? guides(aov, aovBytes, &ai) : gmupt_render_aovs(r, aov_samples, aov, aovBytes, &ai);
    if (info) *info = ai;
    if (rc != GMUPT_OK) return rc;
    GMUPT_TRY(gmupt_copy_framebuffer_to_device(r, const_cast<float*>(beauty), (size_t)W * H * 16));
    if (infill) {   // enqueued, not waited for: the filter's launches follow on the same stream
        GMUPT_TRY(r->ifEv.start(r->stream));
        GMUPT_TRY(enqueue_infill(r, reinterpret_cast<const float4*>(beauty), reinterpret_cast<const float4*>(aov), W, H, *infill, r->ifImage.as<float4>(), nullptr));
        GMUPT_TRY(r->ifEv.stop(r->stream));
        beauty = r->ifImage.as<const float>();
    }
    float ms = 0.0f, msInfill = 0.0f;
    rc = gmupt_denoise_image(r, beauty, aov, W, H, p, out_rgba, bytes, &ms);   // synchronises the stream
    if (rc == GMUPT_OK && infill) GMUPT_TRY(r->ifEv.elapsed_ms(&msInfill));
    if (info) info->ms = ai.ms + msInfill + ms;
    return rc;
}

extern "C" int gmupt_render_denoised(gmupt_renderer* r, uint32_t aov_samples, const gmupt_denoise_params* p, float* out_rgba, size_t bytes, gmupt_trace_info* info)
{
    return render_denoised("gmupt_render_denoised", r, aov_samples, p, nullptr, out_rgba, bytes, info);
}

// ------------------------------------------------------------------------------------------------ temporal reuse
static_assert(sizeof(gmupt_history) == 48 && offsetof(gmupt_history, count) == 12 && offsetof(gmupt_history, normal) == 16 &&
              offsetof(gmupt_history, material) == 28 && offsetof(gmupt_history, position) == 32 && offsetof(gmupt_history, valid) == 44, "gmupt_history layout");

extern "C" int gmupt_temporal_create(gmupt_renderer* r, gmupt_temporal** out)
{
    if (out) *out = nullptr;
    if (!r || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_temporal_create: null argument");
    gmupt_temporal* t = new (std::nothrow) gmupt_temporal();
    if (!t) return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_temporal_create: out of host memory");
    t->r = r;
    *out = t;
    return GMUPT_OK;
}

extern "C" void gmupt_temporal_destroy(gmupt_temporal* t)
{
    if (!t) return;
    (void)hipSetDevice(t->r->dev->id);
    (void)hipStreamSynchronize(t->r->stream);
    delete t;
}

extern "C" int gmupt_temporal_reset(gmupt_temporal* t)
{
    if (!t) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_temporal_reset: null handle");
    t->frozen.present = false; t->last.present = false;
    if (t->frozen.verts.ptr || t->last.verts.ptr) {   // the pose snapshots go with the records
        HIP_TRY(hipSetDevice(t->r->dev->id));
        HIP_TRY(hipStreamSynchronize(t->r->stream));
        for (TpSlot* sl : { &t->frozen, &t->last }) { sl->verts = DevMem(); sl->hasPose = false; }
    }
    return GMUPT_OK;
}

// gmupt_temporal_denoise_image (motion == nullptr: k_tp_integrate) and gmupt_temporal_denoise_image_motion (k_tp_integrate_mv); with
// `infill` gmupt_temporal_preview_image: the infill stage between the integration, which has written the records, and the filter
int temporal_denoise(const char* fn, gmupt_temporal* t, const float* beauty_rgba, const gmupt_aov* aov, const gmupt_motion* motion,
                     const gmupt_camera_buffer* cam, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, int new_accumulation,
                     const gmupt_temporal_params* p, const IfParams* infill, float* out_rgba, size_t out_bytes, float* ms)
{
    if (ms) *ms = 0.0f;
    DnParams dn; TpParams tp;
    GMUPT_TRY(image_args(fn, beauty_rgba, aov, width, height, out_rgba, out_bytes, true));   // needs no device: checked first
    GMUPT_TRY(temporal_params(fn, p, dn, tp));                                               // the spatial parameters first
    if (!cam) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null camera", fn);
    if (!t) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null handle", fn);
    gmupt_renderer* r = t->r;
    const size_t n = (size_t)width * height;
    HIP_TRY(hipSetDevice(r->dev->id));
    if (new_accumulation) std::swap(t->frozen, t->last);   // the records of the accumulation that ended become the history
    int rc = t->last.rec.grow(r->stream, n * sizeof(gmupt_history));
    if (rc == GMUPT_OK) rc = t->integrated.grow(r->stream, n * 16);
    if (rc == GMUPT_OK) rc = r->dnScratch.grow(r->stream, n * kGdScratchBytes);
    if (rc == GMUPT_OK && infill) rc = r->ifImage.grow(r->stream, n * 16);
    if (rc != GMUPT_OK) { t->last.present = false; return rc; }
    TpPrev prev{};
    if (t->frozen.present) {
        prev.rec = t->frozen.rec.as<const float4>();
        prev.x0 = (int)t->frozen.x0; prev.y0 = (int)t->frozen.y0; prev.W = (int)t->frozen.W; prev.H = (int)t->frozen.H;
        prev.cam = tp_camera(t->frozen.cam);
    }
    float4* integrated = t->integrated.as<float4>();
    t->last.present = false;                                // until its records are written
    t->last.hasPose = false;                                // until gmupt_render_denoised_temporal_motion says which pose they are in
    GMUPT_TRY(t->ev.start(r->stream));
    if (motion)
        launch_temporal_motion(reinterpret_cast<const float4*>(beauty_rgba), reinterpret_cast<const float4*>(aov), reinterpret_cast<const float4*>(motion),
                               (int)width, (int)height, prev, tp, integrated, t->last.rec.as<float4>(), r->stream);
    else
        launch_temporal(reinterpret_cast<const float4*>(beauty_rgba), reinterpret_cast<const float4*>(aov), (int)width, (int)height, prev, tp, integrated,
                        t->last.rec.as<float4>(), r->stream);
    HIP_TRY(hipGetLastError());
    if (infill) {
        GMUPT_TRY(enqueue_infill(r, integrated, reinterpret_cast<const float4*>(aov), width, height, *infill, r->ifImage.as<float4>(), nullptr));
        integrated = r->ifImage.as<float4>();
    }
    launch_denoise(integrated, reinterpret_cast<const float4*>(aov), (int)width, (int)height, dn, r->dnScratch.ptr, reinterpret_cast<float4*>(out_rgba), r->stream);
    HIP_TRY(hipGetLastError());
    GMUPT_TRY(t->ev.stop(r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    t->last.present = true; t->last.cam = *cam; t->last.x0 = x0; t->last.y0 = y0; t->last.W = width; t->last.H = height;
    float e = 0.0f;
    GMUPT_TRY(t->ev.elapsed_ms(&e));
    if (ms) *ms = e;
    return GMUPT_OK;
}

extern "C" int gmupt_temporal_denoise_image(gmupt_temporal* t, const float* beauty_rgba, const gmupt_aov* aov, const gmupt_camera_buffer* cam,
                                            uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, int new_accumulation,
                                            const gmupt_temporal_params* p, float* out_rgba, size_t out_bytes, float* ms)
{
    return temporal_denoise("gmupt_temporal_denoise_image", t, beauty_rgba, aov, nullptr, cam, x0, y0, width, height, new_accumulation, p, nullptr, out_rgba, out_bytes, ms);
}

extern "C" int gmupt_temporal_denoise_image_motion(gmupt_temporal* t, const float* beauty_rgba, const gmupt_aov* aov, const gmupt_motion* motion,
                                                   const gmupt_camera_buffer* cam, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height,
                                                   int new_accumulation, const gmupt_temporal_params* p, float* out_rgba, size_t out_bytes, float* ms)
{
    const char* fn = "gmupt_temporal_denoise_image_motion";
    if ((uintptr_t)motion & 15u) { if (ms) *ms = 0.0f; return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: misaligned motion plane (16 bytes)", fn); }
    return temporal_denoise(fn, t, beauty_rgba, aov, motion, cam, x0, y0, width, height, new_accumulation, p, nullptr, out_rgba, out_bytes, ms);
}

// gmupt_render_denoised_temporal, and with `poses` gmupt_render_denoised_temporal_motion: the record sets keep their vertex pose; with
// `infill` gmupt_render_preview
int render_denoised_temporal(const char* fn, bool poses, gmupt_renderer* r, gmupt_temporal* t, uint32_t aov_samples, const gmupt_temporal_params* p,
                             const IfParams* infill, float* out_rgba, size_t bytes, gmupt_trace_info* info)
{
    if (info) std::memset(info, 0, sizeof(*info));
    if (!r || !t) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null renderer or handle", fn);
    if (t->r != r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: the handle belongs to another renderer", fn);
    const uint32_t W = r->p.fbW, H = r->p.fbH;
    DnParams dn; TpParams tp;
    GMUPT_TRY(render_args(fn, r, aov_samples, out_rgba, bytes, [&] { return temporal_params(fn, p, dn, tp); }));
    const bool fold = !t->seen || t->generation != r->accumGeneration;
    // the record sets as they will be once the fold has swapped them: `fz` is integrated against, `nw` receives this call's records
    TpSlot& fz = fold ? t->last : t->frozen;
    TpSlot& nw = fold ? t->frozen : t->last;
    const uint32_t nv = r->p.scene.numVerts;
    const auto inPose = [&](const TpSlot& sl) { return sl.hasPose && sl.binding == r->bindingId && sl.numVerts == nv; };
    const bool moved = poses && fz.present && inPose(fz) && fz.geomGeneration != r->geomGeneration;
    const size_t npix = (size_t)W * H;
    GMUPT_TRY(r->dnInput.grow(r->stream, npix * (sizeof(gmupt_aov) + 16 + (moved ? sizeof(gmupt_motion) : 0))));
    gmupt_aov* aov = r->dnInput.as<gmupt_aov>();
    float* beauty = reinterpret_cast<float*>(r->dnInput.as<char>() + npix * sizeof(gmupt_aov));
    gmupt_motion* motion = moved ? reinterpret_cast<gmupt_motion*>(r->dnInput.as<char>() + npix * (sizeof(gmupt_aov) + 16)) : nullptr;
    gmupt_trace_info ai;
    int rc;
    if (moved) rc = gmupt_render_aovs_motion(r, aov_samples, fz.verts.as<const float>(), nv, aov, npix * sizeof(gmupt_aov), motion, npix * sizeof(gmupt_motion), &ai);
    else rc = gmupt_render_aovs(r, aov_samples, aov, npix * sizeof(gmupt_aov), &ai);
    if (info) *info = ai;
    if (rc != GMUPT_OK) return rc;
    GMUPT_TRY(gmupt_copy_framebuffer_to_device(r, beauty, npix * 16));
    if (poses && !(inPose(nw) && nw.geomGeneration == r->geomGeneration)) {
        // the pose of the records this call writes: once per refit, into the set that receives them (never the one integrated against).
        // It is written before temporal_denoise() has checked its arguments and folded, so that one synchronisation serves both; the
        // set is marked as having no pose first and gets it back only after that call succeeded, so a refused call leaves a set that
        // is integrated against without a motion plane, never one with a wrong pose.
        nw.hasPose = false;
        GMUPT_TRY(nw.verts.grow(r->stream, (size_t)nv * 12));
        HIP_TRY(hipMemcpyAsync(nw.verts.ptr, r->p.scene.verts, (size_t)nv * 12, hipMemcpyDeviceToDevice, r->stream));
    }
    float ms = 0.0f;
    rc = temporal_denoise(fn, t, beauty, aov, motion, &r->p.cam, r->tile_x0(), r->tile_y0(), W, H, fold ? 1 : 0, p, infill, out_rgba, bytes, &ms);   // synchronises the stream
    if (info) info->ms = ai.ms + ms;
    if (rc != GMUPT_OK) return rc;
    t->seen = true; t->generation = r->accumGeneration;
    if (poses) { t->last.hasPose = true; t->last.binding = r->bindingId; t->last.geomGeneration = r->geomGeneration; t->last.numVerts = nv; }
    return GMUPT_OK;
}

extern "C" int gmupt_render_denoised_temporal(gmupt_renderer* r, gmupt_temporal* t, uint32_t aov_samples, const gmupt_temporal_params* p,
                                              float* out_rgba, size_t bytes, gmupt_trace_info* info)
{
    return render_denoised_temporal("gmupt_render_denoised_temporal", false, r, t, aov_samples, p, nullptr, out_rgba, bytes, info);
}

extern "C" int gmupt_render_denoised_temporal_motion(gmupt_renderer* r, gmupt_temporal* t, uint32_t aov_samples, const gmupt_temporal_params* p,
                                                     float* out_rgba, size_t bytes, gmupt_trace_info* info)
{
    return render_denoised_temporal("gmupt_render_denoised_temporal_motion", true, r, t, aov_samples, p, nullptr, out_rgba, bytes, info);
}
