// C-ABI of libgmupt.so: the thin lens of a renderer (gmupt_renderer_set_lens / get_lens, launched by run_iteration through pt_lens.hip)
// and the autofocus on a picked pixel.
#include "gmupt_internal.hpp"

extern "C" int gmupt_renderer_set_lens(gmupt_renderer* r, const gmupt_lens* lens)
{
    const char* fn = "gmupt_renderer_set_lens";
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null renderer", fn);
    gmupt_lens none;
    gmupt_lens_default_params(&none);
    if (!lens) { r->lens = none; return GMUPT_OK; }
    GMUPT_TRY(lens_params(fn, lens));
    if (lens->aperture_radius > 0.0f && r->projection.kind != GMUPT_PROJ_PINHOLE)   // include/gmupt_projection.h: the focal plane has no meaning behind the camera
        return fail(GMUPT_ERR_UNSUPPORTED, "%s: a projection of kind %u is attached: lens and projection do not combine", fn, r->projection.kind);
    r->lens = lens->aperture_radius > 0.0f ? *lens : none;   // the launch argument of the iterations that follow; nothing is enqueued here
    return GMUPT_OK;
}

extern "C" int gmupt_renderer_get_lens(gmupt_renderer* r, gmupt_lens* out)
{
    if (!r || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_get_lens: null argument");
    *out = r->lens;
    return GMUPT_OK;
}

extern "C" int gmupt_lens_focus_at(gmupt_renderer* r, float px, float py, uint32_t light_count, gmupt_lens* inout)
{
    const char* fn = "gmupt_lens_focus_at";
    if (!r || !inout) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    gmupt_ray ray;
    gmupt_hit hit;
    GMUPT_TRY(gmupt_pick(r, px, py, light_count, &ray, &hit));
    if (hit.triangle < 0 && hit.light == 0) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: pixel (%g, %g) sees neither a triangle nor a light: nothing to focus on", fn, (double)px, (double)py);
    inout->focus_distance = lens_focus_depth(r->p.cam, ray.direction, hit.t);
    return GMUPT_OK;
}
