// The rule of the thin lens (include/gmupt_lens.h states it), shared by the host function (pt_lens.cpp) and k_lens_retarget
// (pt_lens.hip).  One copy, so that host and device run the same statements: binary32 in the written order, nothing contracted
// (build.py), sin / cos / sqrt from detmath.hpp.  pt_kernels.hip does not include this file: step 1's lines are stage_new_path's,
// restated, because sharing them through a header moved k_material's register allocation (pt_adaptive.hip).
#pragma once
#include "pt_camera_rays.hpp"     // CamRay, store_ray
#include "../../include/gmupt_lens.h"

namespace gmupt {

// the ray of the fresh camera path at entry q of the new-path queue whose screen coordinate is the whole-frame pixel (cx, cy)
GM_HD CamRay lens_ray(const gmupt_camera_buffer& cam, float apertureRadius, float focusDistance, uint32_t q, uint32_t cx, uint32_t cy)
{
    // 1. the pinhole ray (newPath.hlsl:27,36-39)
    Rng g; g.seed(q, cam.randomSeed[0], cam.randomSeed[1]);
    const float jx = g.next() * 2.0f - 1.0f;
    const float jy = g.next() * 2.0f - 1.0f;
    const float u = ((float)cx + jx) * cam.pixelSize[0];
    const float v = ((float)cy + jy) * cam.pixelSize[1];
    const f3 pos = mk3(cam.position[0], cam.position[1], cam.position[2]);
    const f3 ulc = mk3(cam.upperLeftCorner[0], cam.upperLeftCorner[1], cam.upperLeftCorner[2]);
    const f3 hor = mk3(cam.horizontal[0], cam.horizontal[1], cam.horizontal[2]);
    const f3 ver = mk3(cam.vertical[0], cam.vertical[1], cam.vertical[2]);
    const f3 d = normalize3((ulc + hor * u) - ver * v);
    // 2. the point on the lens
    const float r1 = g.next();
    const float r2 = g.next();
    const float rad = apertureRadius * dsqrt(r1);
    const float phi = r2 * 6.2831853f;
    const float lx = rad * dcos(phi);
    const float ly = rad * dsin(phi);
    // 3. the camera frame
    const f3 right = normalize3(hor);
    const f3 up = normalize3(ver);
    const f3 fn = normalize3((ulc + hor * 0.5f) - ver * 0.5f);
    // 4. the focal point
    const float t = focusDistance / dot3(d, fn);
    const f3 Pf = pos + d * t;
    // 5. the new ray
    CamRay r;
    r.origin = (pos + right * lx) + up * ly;
    r.direction = normalize3(Pf - r.origin);
    return r;
}

// ---- host side (pt_lens.cpp)
// gmupt_lens_ray_host with checked arguments: the rule as a gmupt_ray (store_ray)
void lens_ray_host(const gmupt_camera_buffer& cam, const gmupt_lens& lens, uint32_t q, uint32_t cx, uint32_t cy, gmupt_ray* out);
// gmupt_lens_focus_at: the depth along the forward axis fn of step 3 of the point at distance t on a ray of direction `dir` from the camera
float lens_focus_depth(const gmupt_camera_buffer& cam, const float dir[3], float t);

// ---- device side (pt_lens.hip): the launch between k_material (and k_ad_retarget) and the ray cast
void launch_lens_retarget(const RenderParams& p, float apertureRadius, float focusDistance, hipStream_t s);

} // namespace gmupt
