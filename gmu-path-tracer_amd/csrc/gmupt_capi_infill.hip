// C-ABI of libgmupt.so: the guided infill on device images and the preview chains that contain it.
#include "gmupt_internal.hpp"

int enqueue_infill(gmupt_renderer* r, const float4* beauty, const float4* aov, uint32_t W, uint32_t H, const IfParams& prm, float4* out, const IfCounters** counts)
{
    GMUPT_TRY(r->ifScratch.grow(r->stream, infill_scratch_bytes((size_t)W * H)));
    HIP_TRY(launch_infill(beauty, aov, (int)W, (int)H, prm, r->ifScratch.ptr, out, r->stream, counts));
    return GMUPT_OK;
}

extern "C" int gmupt_infill_image(gmupt_renderer* r, const float* beauty_rgba, const gmupt_aov* aov, uint32_t width, uint32_t height,
                                  const gmupt_infill_params* p, float* out_rgba, size_t out_bytes, gmupt_infill_info* info)
{
    const char* fn = "gmupt_infill_image";
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null renderer", fn);
    IfParams prm;
    GMUPT_TRY(image_args(fn, beauty_rgba, aov, width, height, out_rgba, out_bytes, true));
    GMUPT_TRY(infill_params(fn, p, prm));
    HIP_TRY(hipSetDevice(r->dev->id));
    if (info) GMUPT_TRY(r->ifEv.start(r->stream));
    const IfCounters* counts = nullptr;
    GMUPT_TRY(enqueue_infill(r, reinterpret_cast<const float4*>(beauty_rgba), reinterpret_cast<const float4*>(aov), width, height, prm,
                             reinterpret_cast<float4*>(out_rgba), &counts));
    if (!info) return GMUPT_OK;
    GMUPT_TRY(r->ifEv.stop(r->stream));
    IfCounters c{};
    GMUPT_TRY(copy_sync(&c, counts, sizeof(c), hipMemcpyDeviceToHost, r->stream));   // the one synchronisation
    float ms = 0.0f;
    GMUPT_TRY(r->ifEv.elapsed_ms(&ms));
    info->sources = c.sources; info->holes = c.holes; info->filled = c.filled; info->open_left = c.openLeft; info->ms = (double)ms;
    return GMUPT_OK;
}

extern "C" int gmupt_temporal_preview_image(gmupt_temporal* t, const float* beauty_rgba, const gmupt_aov* aov, const gmupt_motion* motion,
                                            const gmupt_camera_buffer* cam, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height,
                                            int new_accumulation, const gmupt_temporal_params* p, const gmupt_infill_params* infill,
                                            float* out_rgba, size_t out_bytes, float* ms)
{
    if (!infill)
        return motion ? gmupt_temporal_denoise_image_motion(t, beauty_rgba, aov, motion, cam, x0, y0, width, height, new_accumulation, p, out_rgba, out_bytes, ms)
                      : gmupt_temporal_denoise_image(t, beauty_rgba, aov, cam, x0, y0, width, height, new_accumulation, p, out_rgba, out_bytes, ms);
    const char* fn = "gmupt_temporal_preview_image";
    if (ms) *ms = 0.0f;
    IfParams prm;
    GMUPT_TRY(infill_params(fn, infill, prm));
    if ((uintptr_t)motion & 15u) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: misaligned motion plane (16 bytes)", fn);
    return temporal_denoise(fn, t, beauty_rgba, aov, motion, cam, x0, y0, width, height, new_accumulation, p, &prm, out_rgba, out_bytes, ms);
}

extern "C" int gmupt_render_preview(gmupt_renderer* r, gmupt_temporal* t, uint32_t flags, uint32_t aov_samples, const gmupt_temporal_params* p,
                                    const gmupt_infill_params* infill, float* out_rgba, size_t bytes, gmupt_trace_info* info)
{
    const char* fn = "gmupt_render_preview";
    if ((flags & ~GMUPT_PREVIEW_MOTION) || (!t && flags)) {
        if (info) std::memset(info, 0, sizeof(*info));
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: flags = 0x%x (GMUPT_PREVIEW_MOTION, and only with a history handle)", fn, flags);
    }
    const bool motion = (flags & GMUPT_PREVIEW_MOTION) != 0u;
    if (!infill) {
        if (!t) return gmupt_render_denoised(r, aov_samples, p ? &p->spatial : nullptr, out_rgba, bytes, info);
        return motion ? gmupt_render_denoised_temporal_motion(r, t, aov_samples, p, out_rgba, bytes, info)
                      : gmupt_render_denoised_temporal(r, t, aov_samples, p, out_rgba, bytes, info);
    }
    IfParams prm;
    if (infill_params(fn, infill, prm) != GMUPT_OK) { if (info) std::memset(info, 0, sizeof(*info)); return GMUPT_ERR_INVALID_ARGUMENT; }
    if (t) return render_denoised_temporal(fn, motion, r, t, aov_samples, p, &prm, out_rgba, bytes, info);
    return render_denoised(fn, r, aov_samples, p ? &p->spatial : nullptr, &prm, out_rgba, bytes, info);
}
