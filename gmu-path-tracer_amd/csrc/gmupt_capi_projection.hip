// C-ABI of libgmupt.so: the camera projections (include/gmupt_projection.h) -- the projection of a renderer (launched by run_iteration
// through pt_projection.hip), the host rules, picking, and the AOV records and the denoiser under a projection: the chunk loop of
// gmupt_render_aovs (render_aov_chunks) with this file's ray generation and the resolve of gmupt_render_aovs_lens.
#include "gmupt_internal.hpp"

static_assert(sizeof(gmupt_projection) == 16 && offsetof(gmupt_projection, fov) == 4 && offsetof(gmupt_projection, extent) == 8 &&
              offsetof(gmupt_projection, pad) == 12, "gmupt_projection layout");

extern "C" void gmupt_projection_default_params(gmupt_projection* proj)
{
    if (!proj) return;
    proj->kind = GMUPT_PROJ_PINHOLE; proj->fov = 3.14159274f; proj->extent = 1.0f; proj->pad = 0;
}

int projection_params(const char* fn, const gmupt_projection* proj)
{
    if (!proj) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null projection", fn);
    if (const char* what = projection_fault(*proj))
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: kind %u, fov %g, extent %g: %s", fn, proj->kind, (double)proj->fov, (double)proj->extent, what);
    return GMUPT_OK;
}

// the projection of a call: the one given, checked, or the renderer's (none attached: the pinhole)
static int call_projection(const char* fn, const gmupt_renderer* r, const gmupt_projection* proj_or_null, gmupt_projection* out)
{
    if (proj_or_null) GMUPT_TRY(projection_params(fn, proj_or_null));
    *out = proj_or_null ? *proj_or_null : r->projection;
    return GMUPT_OK;
}

extern "C" int gmupt_renderer_set_projection(gmupt_renderer* r, const gmupt_projection* proj)
{
    const char* fn = "gmupt_renderer_set_projection";
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null renderer", fn);
    gmupt_projection none;
    gmupt_projection_default_params(&none);
    if (!proj) { r->projection = none; return GMUPT_OK; }
    GMUPT_TRY(projection_params(fn, proj));
    if (proj->kind != GMUPT_PROJ_PINHOLE && r->lens.aperture_radius > 0.0f)
        return fail(GMUPT_ERR_UNSUPPORTED, "%s: a lens with aperture_radius %g is attached: lens and projection do not combine", fn, (double)r->lens.aperture_radius);
    r->projection = proj->kind != GMUPT_PROJ_PINHOLE ? *proj : none;   // the launch argument of the iterations that follow; nothing is enqueued here
    return GMUPT_OK;
}

extern "C" int gmupt_renderer_get_projection(gmupt_renderer* r, gmupt_projection* out)
{
    if (!r || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_get_projection: null argument");
    *out = r->projection;
    return GMUPT_OK;
}

extern "C" int gmupt_projection_ray_host(const gmupt_camera_buffer* cam, const gmupt_projection* proj, uint32_t q, uint32_t cx, uint32_t cy, gmupt_ray* out)
{
    const char* fn = "gmupt_projection_ray_host";
    if (!cam || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null camera or result", fn);
    GMUPT_TRY(projection_params(fn, proj));
    store_ray(projection_fresh_ray(*cam, *proj, q, cx, cy), out);
    return GMUPT_OK;
}

extern "C" int gmupt_projection_pick_ray(const gmupt_camera_buffer* cam, const gmupt_projection* proj, float px, float py, gmupt_ray* out)
{
    const char* fn = "gmupt_projection_pick_ray";
    if (!cam || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null camera or result", fn);
    GMUPT_TRY(projection_params(fn, proj));
    store_ray(projection_pixel_ray(*cam, *proj, px, py), out);
    return GMUPT_OK;
}

extern "C" int gmupt_projection_project_host(const gmupt_camera_buffer* cam, const gmupt_projection* proj, const float world[3], double* px, double* py, int* on_image)
{
    const char* fn = "gmupt_projection_project_host";
    if (!cam || !world || !px || !py || !on_image) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    GMUPT_TRY(projection_params(fn, proj));
    *on_image = projection_project(*cam, *proj, world, px, py) ? 1 : 0;
    return GMUPT_OK;
}

extern "C" int gmupt_aov_projected_ray(const gmupt_camera_buffer* cam, const gmupt_projection* proj, uint32_t x, uint32_t y, uint32_t samples, uint32_t k, gmupt_ray* out)
{
    const char* fn = "gmupt_aov_projected_ray";
    if (!cam || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null camera or result", fn);
    GMUPT_TRY(projection_params(fn, proj));
    uint32_t R;
    GMUPT_TRY(aov_sample_plan(fn, "samples", 0, samples, &R, false));
    if (k >= R) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: ray %u of %u", fn, k, R);
    store_ray(projection_aov_ray(*cam, *proj, x, y, samples, k), out);
    return GMUPT_OK;
}

extern "C" int gmupt_pick_projected(gmupt_renderer* r, float px, float py, uint32_t light_count, gmupt_ray* ray_out, gmupt_hit* hit_out)
{
    const char* fn = "gmupt_pick_projected";
    if (!r || !hit_out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    if (!r->cameraSet) return fail(GMUPT_ERR_NOT_BOUND, "%s: no camera set", fn);
    if (!r->sceneBound) return fail(GMUPT_ERR_NOT_BOUND, "%s: no scene bound", fn);
    gmupt_ray ray;
    GMUPT_TRY(gmupt_projection_pick_ray(&r->p.cam, &r->projection, px, py, &ray));
    return pick_ray_hit(r, ray, light_count, ray_out, hit_out);
}

extern "C" int gmupt_debug_read_aov_rays(gmupt_renderer* r, gmupt_ray* out, uint32_t count)
{
    const char* fn = "gmupt_debug_read_aov_rays";
    if (!r || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    if (!r->aovRays.ptr) return fail(GMUPT_ERR_NOT_BOUND, "%s: no AOV call has allocated the chunk scratch yet", fn);
    if (count > GMUPT_AOV_CHUNK_RAYS) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: %u rays, a chunk holds %u", fn, count, (unsigned)GMUPT_AOV_CHUNK_RAYS);
    HIP_TRY(hipSetDevice(r->dev->id));
    return copy_sync(out, r->aovRays.ptr, (size_t)count * sizeof(gmupt_ray), hipMemcpyDeviceToHost, r->stream);
}

// gmupt_render_aovs_projected under a checked projection, with fn as the name in its errors
static int render_aovs_projected(const char* fn, gmupt_renderer* r, const gmupt_projection& proj, uint32_t samples, gmupt_aov* out, size_t bytes, gmupt_trace_info* info)
{
    return render_aov_chunks(fn, r, samples, false, out, bytes, info,
        [&](const AovRows& c) { launch_paov_raygen(r->p.cam, proj, r->tile_x0(), r->tile_y0() + c.row, c.W, c.rows, samples, c.rays, r->stream); },
        [&](const AovRows& c) { launch_laov_resolve(r->p, c.rows * c.W, samples, c.rays, c.hits, out + (size_t)c.row * c.W, r->stream); });
}

extern "C" int gmupt_render_aovs_projected(gmupt_renderer* r, const gmupt_projection* proj_or_null, uint32_t samples, gmupt_aov* out, size_t bytes, gmupt_trace_info* info)
{
    const char* fn = "gmupt_render_aovs_projected";
    if (info) std::memset(info, 0, sizeof(*info));
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null renderer", fn);
    gmupt_projection proj;
    GMUPT_TRY(call_projection(fn, r, proj_or_null, &proj));
    return render_aovs_projected(fn, r, proj, samples, out, bytes, info);
}

extern "C" int gmupt_render_denoised_projected(gmupt_renderer* r, const gmupt_projection* proj_or_null, uint32_t aov_samples, const gmupt_denoise_params* p,
                                               float* out_rgba, size_t bytes, gmupt_trace_info* info)
{
    const char* fn = "gmupt_render_denoised_projected";
    if (info) std::memset(info, 0, sizeof(*info));
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null renderer", fn);
    gmupt_projection proj;
    GMUPT_TRY(call_projection(fn, r, proj_or_null, &proj));
    return render_denoised(fn, r, aov_samples, p, nullptr, out_rgba, bytes, info,
                           [&](gmupt_aov* aov, size_t n, gmupt_trace_info* ai) { return render_aovs_projected(fn, r, proj, aov_samples, aov, n, ai); });
}
