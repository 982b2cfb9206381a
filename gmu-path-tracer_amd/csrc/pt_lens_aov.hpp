// The rays of the lens-filtered AOV planes (include/gmupt_lens_aov.h states the rule), shared by the host function (pt_lens_aov.cpp)
// and k_laov_raygen (pt_lens_aov.hip).  One copy, so that host and device run the same statements: binary32 in the written order,
// nothing contracted (build.py), sin / cos / sqrt from detmath.hpp.  Steps 2-5 are lens_ray's lines (pt_lens.hpp), restated with the
// stratum in place of the two draws: lens_ray keeps its own copy, as it keeps stage_new_path's, so that k_lens_retarget stays the
// instructions it was.
#pragma once
#include "pt_lens.hpp"         // and through it pt_shading.hpp: camera_ray_direction, aov_ray_coords
#include "../../include/gmupt_lens_aov.h"

namespace gmupt {

// ray k (0 .. s*s - 1) of whole-frame pixel (x, y) at s samples per axis
GM_HD CamRay lens_aov_ray(const gmupt_camera_buffer& cam, float apertureRadius, float focusDistance, uint32_t x, uint32_t y, uint32_t s, uint32_t k)
{
    // 1. the pixel-filter cell (a, b): the stratified AOV ray k + 1, or the pixel centre at s == 1
    const uint32_t a = k % s, b = k / s;
    float px, py;
    aov_ray_coords(x, y, s, s > 1 ? k + 1 : 0u, px, py);
    const f3 d = camera_ray_direction(cam, px, py);
    // 2. the point on the lens: stratum (a2, b2) = (b, s - 1 - a)
    const uint32_t a2 = b, b2 = s - 1 - a;
    const float r1 = ((float)a2 + 0.5f) / (float)s;
    const float r2 = ((float)b2 + 0.5f) / (float)s;
    const float rad = apertureRadius * dsqrt(r1);
    const float phi = r2 * 6.2831853f;
    const float lx = rad * dcos(phi);
    const float ly = rad * dsin(phi);
    // 3. the camera frame
    const f3 pos = mk3(cam.position[0], cam.position[1], cam.position[2]);
    const f3 ulc = mk3(cam.upperLeftCorner[0], cam.upperLeftCorner[1], cam.upperLeftCorner[2]);
    const f3 hor = mk3(cam.horizontal[0], cam.horizontal[1], cam.horizontal[2]);
    const f3 ver = mk3(cam.vertical[0], cam.vertical[1], cam.vertical[2]);
    const f3 right = normalize3(hor);
    const f3 up = normalize3(ver);
    const f3 fn = normalize3((ulc + hor * 0.5f) - ver * 0.5f);
    // 4. the focal point
    const float t = focusDistance / dot3(d, fn);
    const f3 Pf = pos + d * t;
    // 5. the ray
    CamRay r;
    r.origin = (pos + right * lx) + up * ly;
    r.direction = normalize3(Pf - r.origin);
    return r;
}

// ---- host side (pt_lens_aov.cpp)
// gmupt_aov_lens_ray with checked arguments: the rule as a gmupt_ray (store_ray)
void lens_aov_ray_host(const gmupt_camera_buffer& cam, const gmupt_lens& lens, uint32_t x, uint32_t y, uint32_t samples, uint32_t k, gmupt_ray* out);

// ---- device side (pt_lens_aov.hip).  rays / hits: the chunk scratch of gmupt_render_aovs, 32 bytes per ray; out: the chunk's first record.
void launch_laov_raygen(const gmupt_camera_buffer& cam, const gmupt_lens& lens, uint32_t x0, uint32_t y0, uint32_t width, uint32_t rows, uint32_t samples,
                        gmupt_ray* rays, hipStream_t s);
void launch_laov_resolve(const RenderParams& p, uint32_t npix, uint32_t samples, const gmupt_ray* rays, const gmupt_hit* hits, gmupt_aov* out, hipStream_t s);

} // namespace gmupt
