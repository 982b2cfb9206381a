// C-ABI of libgmupt.so: the lens-filtered AOV records (include/gmupt_lens_aov.h) -- gmupt_render_aovs_lens through pt_lens_aov.hip and the
// chunk loop of gmupt_render_aovs (render_aov_chunks), the host rule of its rays, and the denoiser on these records.
#include "gmupt_internal.hpp"

// the lens of a call: the one given, checked as gmupt_renderer_set_lens checks it, or the renderer's (none attached: aperture 0)
static int call_lens(const char* fn, const gmupt_renderer* r, const gmupt_lens* lens_or_null, gmupt_lens* out)
{
    if (lens_or_null) GMUPT_TRY(lens_params(fn, lens_or_null));
    *out = lens_or_null ? *lens_or_null : r->lens;
    return GMUPT_OK;
}

// gmupt_render_aovs_lens under a checked lens, with fn as the name in its errors
static int render_aovs_lens(const char* fn, gmupt_renderer* r, const gmupt_lens& lens, uint32_t samples, gmupt_aov* out, size_t bytes, gmupt_trace_info* info)
{
    return render_aov_chunks(fn, r, samples, false, out, bytes, info,
        [&](const AovRows& c) { launch_laov_raygen(r->p.cam, lens, r->tile_x0(), r->tile_y0() + c.row, c.W, c.rows, samples, c.rays, r->stream); },
        [&](const AovRows& c) { launch_laov_resolve(r->p, c.rows * c.W, samples, c.rays, c.hits, out + (size_t)c.row * c.W, r->stream); });
}

extern "C" int gmupt_render_aovs_lens(gmupt_renderer* r, const gmupt_lens* lens_or_null, uint32_t samples, gmupt_aov* out, size_t bytes, gmupt_trace_info* info)
{
    const char* fn = "gmupt_render_aovs_lens";
    if (info) std::memset(info, 0, sizeof(*info));
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null renderer", fn);
    gmupt_lens lens;
    GMUPT_TRY(call_lens(fn, r, lens_or_null, &lens));
    return render_aovs_lens(fn, r, lens, samples, out, bytes, info);
}

extern "C" int gmupt_aov_lens_ray(const gmupt_camera_buffer* cam, const gmupt_lens* lens, uint32_t x, uint32_t y, uint32_t samples, uint32_t k, gmupt_ray* out)
{
    const char* fn = "gmupt_aov_lens_ray";
    if (!cam || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null camera or result", fn);
    GMUPT_TRY(lens_params(fn, lens));
    uint32_t R;
    GMUPT_TRY(aov_sample_plan(fn, "samples", 0, samples, &R, false));
    if (k >= R) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: ray %u of %u", fn, k, R);
    lens_aov_ray_host(*cam, *lens, x, y, samples, k, out);
    return GMUPT_OK;
}

extern "C" int gmupt_render_denoised_lens(gmupt_renderer* r, const gmupt_lens* lens_or_null, uint32_t aov_samples, const gmupt_denoise_params* p, float* out_rgba,
                                          size_t bytes, gmupt_trace_info* info)
{
    const char* fn = "gmupt_render_denoised_lens";
    if (info) std::memset(info, 0, sizeof(*info));
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null renderer", fn);
    gmupt_lens lens;
    GMUPT_TRY(call_lens(fn, r, lens_or_null, &lens));
    return render_denoised(fn, r, aov_samples, p, nullptr, out_rgba, bytes, info,
                           [&](gmupt_aov* aov, size_t n, gmupt_trace_info* ai) { return render_aovs_lens(fn, r, lens, aov_samples, aov, n, ai); });
}
