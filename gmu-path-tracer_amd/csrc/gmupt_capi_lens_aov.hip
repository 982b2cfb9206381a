// C-ABI of libgmupt.so: the lens-filtered AOV records (include/gmupt_lens_aov.h) -- gmupt_render_aovs_lens through pt_lens_aov.hip on the
// chunk scratch and the query counters of gmupt_render_aovs, the host rule of its rays, and the denoiser on these records.
#include "gmupt_internal.hpp"

// the lens of a call: the one given, checked as gmupt_renderer_set_lens checks it, or the renderer's (none attached: aperture 0)
static int call_lens(const char* fn, const gmupt_renderer* r, const gmupt_lens* lens_or_null, gmupt_lens* out)
{
    if (lens_or_null) GMUPT_TRY(lens_params(fn, lens_or_null));
    *out = lens_or_null ? *lens_or_null : r->lens;
    return GMUPT_OK;
}

int render_aovs_lens(const char* fn, gmupt_renderer* r, const gmupt_lens& lens, uint32_t samples, gmupt_aov* out, size_t bytes, gmupt_trace_info* info)
{
    if (info) std::memset(info, 0, sizeof(*info));
    if (!r->sceneBound) return fail(GMUPT_ERR_NOT_BOUND, "%s: no scene bound", fn);
    if (!r->cameraSet) return fail(GMUPT_ERR_NOT_BOUND, "%s: no camera set", fn);
    if (!out || ((uintptr_t)out & 15u)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null or misaligned output (16 bytes)", fn);
    const uint32_t W = r->p.fbW, H = r->p.fbH;
    uint32_t R;
    GMUPT_TRY(aov_sample_plan(fn, "samples", W, samples, &R, false));
    if (bytes < (size_t)W * H * sizeof(gmupt_aov)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: %zu bytes for %ux%u records of 64 bytes", fn, bytes, W, H);
    GMUPT_TRY(query_supported(r, fn));
    GMUPT_TRY(query_buffers(r));
    GMUPT_TRY(aov_chunk_scratch(r));
    const RenderParams& p = r->p;
    gmupt_ray* rays = r->aovRays.as<gmupt_ray>(); gmupt_hit* hits = r->aovHits.as<gmupt_hit>();
    const uint32_t rowsPerChunk = GMUPT_AOV_CHUNK_RAYS / (W * R);   // >= 1: aov_sample_plan admitted the row
    RenderParams q;
    GMUPT_TRY(query_begin(r, &q));
    for (uint32_t row = 0; row < H; row += rowsPerChunk) {
        const uint32_t rows = std::min(rowsPerChunk, H - row), n = rows * W * R;
        launch_laov_raygen(p.cam, lens, r->tile_x0(), r->tile_y0() + row, W, rows, samples, rays, r->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(q.travCounters, 0, 128, r->stream));
        launch_trace_wide(q, rays, n, hits, nullptr, 0, nullptr, p.cam.lightCount, r->stream);
        HIP_TRY(hipGetLastError());
        launch_laov_resolve(p, rows * W, samples, rays, hits, out + (size_t)row * W, r->stream);
        HIP_TRY(hipGetLastError());
    }
    return query_end(r, fn, "records", info);
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
    return render_denoised(fn, r, aov_samples, p, nullptr, out_rgba, bytes, info, &lens);
}
