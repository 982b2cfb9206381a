// The rule of the shutter (include/gmupt_shutter.h states it), shared by the host functions (pt_shutter.cpp) and k_shutter_retarget
// (pt_shutter.hip).  One copy, so that host and device run the same statements: binary32 in the written order, nothing contracted
// (build.py).  The ray of a camera at time t is the attached rule's, unchanged: lens_ray (pt_lens.hpp), projection_fresh_ray
// (pt_projection.hpp), or the pinhole below.  pt_kernels.hip does not include this file (pt_lens.hpp says why).
#pragma once
#include "pt_lens.hpp"
#include "pt_projection.hpp"
#include "../../include/gmupt_shutter.h"

namespace gmupt {

// 1. the time of the fresh camera path at entry q of the new-path queue: the fifth draw of the generator whose first two are the jitter
// and whose third and fourth are the lens point
GM_HD float shutter_time(const gmupt_camera_buffer& cam, uint32_t q)
{
    Rng g; g.seed(q, cam.randomSeed[0], cam.randomSeed[1]);
    g.next(); g.next(); g.next(); g.next();
    return g.next();
}

// 2. the camera at time t: the twelve pose components c = a + (b - a) * t, everything else cam's
GM_HD gmupt_camera_buffer shutter_camera(const gmupt_camera_buffer& cam, const gmupt_shutter& sh, float t)
{
    gmupt_camera_buffer c = cam;
    for (int k = 0; k < 3; k++) {
        c.position[k] = cam.position[k] + (sh.position[k] - cam.position[k]) * t;
        c.upperLeftCorner[k] = cam.upperLeftCorner[k] + (sh.upperLeftCorner[k] - cam.upperLeftCorner[k]) * t;
        c.horizontal[k] = cam.horizontal[k] + (sh.horizontal[k] - cam.horizontal[k]) * t;
        c.vertical[k] = cam.vertical[k] + (sh.vertical[k] - cam.vertical[k]) * t;
    }
    return c;
}

// the pinhole ray of a fresh path (newPath.hlsl:27,36-39): the origin is the camera position, the direction step 1 of lens_ray
GM_HD CamRay pinhole_fresh_ray(const gmupt_camera_buffer& cam, uint32_t q, uint32_t cx, uint32_t cy)
{
    Rng g; g.seed(q, cam.randomSeed[0], cam.randomSeed[1]);
    const float jx = g.next() * 2.0f - 1.0f;
    const float jy = g.next() * 2.0f - 1.0f;
    const float u = ((float)cx + jx) * cam.pixelSize[0];
    const float v = ((float)cy + jy) * cam.pixelSize[1];
    const f3 ulc = mk3(cam.upperLeftCorner[0], cam.upperLeftCorner[1], cam.upperLeftCorner[2]);
    const f3 hor = mk3(cam.horizontal[0], cam.horizontal[1], cam.horizontal[2]);
    const f3 ver = mk3(cam.vertical[0], cam.vertical[1], cam.vertical[2]);
    CamRay r;
    r.origin = mk3(cam.position[0], cam.position[1], cam.position[2]);
    r.direction = normalize3((ulc + hor * u) - ver * v);
    return r;
}

// 3. the rules a shutter composes with: (camera at t, q, cx, cy) -> CamRay, each carrying its own parameters
struct ShutterPinhole {
    GM_HD CamRay operator()(const gmupt_camera_buffer& cam, uint32_t q, uint32_t cx, uint32_t cy) const { return pinhole_fresh_ray(cam, q, cx, cy); }
};
struct ShutterLens {
    float apertureRadius, focusDistance;
    GM_HD CamRay operator()(const gmupt_camera_buffer& cam, uint32_t q, uint32_t cx, uint32_t cy) const { return lens_ray(cam, apertureRadius, focusDistance, q, cx, cy); }
};
struct ShutterProjection {
    gmupt_projection proj;
    GM_HD CamRay operator()(const gmupt_camera_buffer& cam, uint32_t q, uint32_t cx, uint32_t cy) const { return projection_fresh_ray(cam, proj, q, cx, cy); }
};

// the ray of the fresh camera path at entry q of the new-path queue whose screen coordinate is the whole-frame pixel (cx, cy)
template <class Rule> GM_HD CamRay shutter_ray(const gmupt_camera_buffer& cam, const gmupt_shutter& sh, const Rule& rule, uint32_t q, uint32_t cx, uint32_t cy)
{
    return rule(shutter_camera(cam, sh, shutter_time(cam, q)), q, cx, cy);
}

// ---- host side (pt_shutter.cpp)
// the argument errors of include/gmupt_shutter.h as a message, nullptr for a close pose that is admitted
const char* shutter_fault(const gmupt_shutter& sh);
// gmupt_shutter_ray_host with checked arguments: lens and proj are not both given; neither = the pinhole
void shutter_ray_host(const gmupt_camera_buffer& cam, const gmupt_shutter& sh, const gmupt_lens* lens, const gmupt_projection* proj, uint32_t q, uint32_t cx,
                      uint32_t cy, gmupt_ray* out);
float shutter_time_host(const gmupt_camera_buffer& cam, uint32_t q);
void shutter_camera_host(const gmupt_camera_buffer& cam, const gmupt_shutter& sh, float t, gmupt_camera_buffer* out);

// ---- device side (pt_shutter.hip): the launch between k_material (and k_ad_retarget) and the ray cast, in place of the lens's or the
// projection's.  lens.aperture_radius > 0 selects the lens rule, otherwise proj.kind != GMUPT_PROJ_PINHOLE the projection's, otherwise the pinhole
void launch_shutter_retarget(const RenderParams& p, const gmupt_shutter& sh, const gmupt_lens& lens, const gmupt_projection& proj, hipStream_t s);

} // namespace gmupt
