// C-ABI of libgmupt.so: the shutter of a renderer (gmupt_renderer_set_shutter / get_shutter, launched by run_iteration through
// pt_shutter.hip) and the host rules of include/gmupt_shutter.h.
#include "gmupt_internal.hpp"

static_assert(sizeof(gmupt_shutter) == 48 && offsetof(gmupt_shutter, upperLeftCorner) == 12 && offsetof(gmupt_shutter, horizontal) == 24 &&
              offsetof(gmupt_shutter, vertical) == 36, "gmupt_shutter layout");

static int shutter_params(const char* fn, const gmupt_shutter* sh)
{
    if (!sh) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null shutter", fn);
    if (const char* what = shutter_fault(*sh)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: %s", fn, what);
    return GMUPT_OK;
}

extern "C" int gmupt_renderer_set_shutter(gmupt_renderer* r, const gmupt_shutter* shutter)
{
    const char* fn = "gmupt_renderer_set_shutter";
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null renderer", fn);
    if (!shutter) { r->shutterAttached = false; return GMUPT_OK; }
    GMUPT_TRY(shutter_params(fn, shutter));
    r->shutter = *shutter; r->shutterAttached = true;   // the launch argument of the iterations that follow; nothing is enqueued here
    return GMUPT_OK;
}

extern "C" int gmupt_renderer_get_shutter(gmupt_renderer* r, gmupt_shutter* out, int* attached)
{
    if (!r || !out || !attached) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_get_shutter: null argument");
    if (r->shutterAttached) *out = r->shutter; else std::memset(out, 0, sizeof(*out));
    *attached = r->shutterAttached ? 1 : 0;
    return GMUPT_OK;
}

extern "C" int gmupt_shutter_from_camera(const gmupt_camera_buffer* close, gmupt_shutter* out)
{
    if (!close || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_shutter_from_camera: null argument");
    gmupt_shutter sh;
    for (int k = 0; k < 3; k++) {
        sh.position[k] = close->position[k]; sh.upperLeftCorner[k] = close->upperLeftCorner[k];
        sh.horizontal[k] = close->horizontal[k]; sh.vertical[k] = close->vertical[k];
    }
    GMUPT_TRY(shutter_params("gmupt_shutter_from_camera", &sh));
    *out = sh;
    return GMUPT_OK;
}

extern "C" int gmupt_shutter_camera_host(const gmupt_camera_buffer* cam, const gmupt_shutter* shutter, float t, gmupt_camera_buffer* out)
{
    const char* fn = "gmupt_shutter_camera_host";
    if (!cam || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null camera or result", fn);
    GMUPT_TRY(shutter_params(fn, shutter));
    if (!std::isfinite(t)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: time %g is not finite", fn, (double)t);
    shutter_camera_host(*cam, *shutter, t, out);
    return GMUPT_OK;
}

extern "C" int gmupt_shutter_time_host(const gmupt_camera_buffer* cam, uint32_t q, float* t)
{
    if (!cam || !t) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_shutter_time_host: null argument");
    *t = shutter_time_host(*cam, q);
    return GMUPT_OK;
}

extern "C" int gmupt_shutter_ray_host(const gmupt_camera_buffer* cam, const gmupt_shutter* shutter, const gmupt_lens* lens_or_null, const gmupt_projection* proj_or_null,
                                      uint32_t q, uint32_t cx, uint32_t cy, gmupt_ray* out)
{
    const char* fn = "gmupt_shutter_ray_host";
    if (!cam || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null camera or result", fn);
    GMUPT_TRY(shutter_params(fn, shutter));
    if (lens_or_null && proj_or_null) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: both a lens and a projection: the two do not combine", fn);
    if (lens_or_null) GMUPT_TRY(lens_params(fn, lens_or_null));
    if (proj_or_null) GMUPT_TRY(projection_params(fn, proj_or_null));
    shutter_ray_host(*cam, *shutter, lens_or_null, proj_or_null, q, cx, cy, out);
    return GMUPT_OK;
}
