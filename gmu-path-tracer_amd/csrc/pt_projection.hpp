// The rule of the camera projections (include/gmupt_projection.h states it), shared by the host functions (pt_projection.cpp) and the
// kernels k_proj_retarget and k_paov_raygen (pt_projection.hip).  One copy, so that host and device run the same statements: binary32
// in the written order, nothing contracted (build.py), sin / cos / sqrt from detmath.hpp.  pt_kernels.hip does not include this file:
// the jitter of a fresh path is stage_new_path's lines, restated, as pt_lens.hpp restates them.
#pragma once
#include "pt_camera_rays.hpp"  // CamRay, store_ray; and through it pt_shading.hpp: aov_ray_coords
#include "../../include/gmupt_projection.h"

namespace gmupt {

// the ray through the screen coordinates (u, v) that the pinhole feeds into (ulc + hor*u) - ver*v
GM_HD CamRay projection_ray(const gmupt_camera_buffer& cam, const gmupt_projection& proj, float u, float v)
{
    const f3 pos = mk3(cam.position[0], cam.position[1], cam.position[2]);
    const f3 ulc = mk3(cam.upperLeftCorner[0], cam.upperLeftCorner[1], cam.upperLeftCorner[2]);
    const f3 hor = mk3(cam.horizontal[0], cam.horizontal[1], cam.horizontal[2]);
    const f3 ver = mk3(cam.vertical[0], cam.vertical[1], cam.vertical[2]);
    CamRay r;
    r.origin = pos;
    if (proj.kind == GMUPT_PROJ_PINHOLE) {      // newPath.hlsl:39
        r.direction = normalize3((ulc + hor * u) - ver * v);
        return r;
    }
    const float sx = 2.0f * u - 1.0f;
    const float sy = 1.0f - 2.0f * v;
    // the camera frame (step 3 of the lens rule)
    const f3 right = normalize3(hor);
    const f3 up = normalize3(ver);
    const f3 fn = normalize3((ulc + hor * 0.5f) - ver * 0.5f);
    // the whole-frame size the camera buffer encodes, as floats
    const float Wf = 1.0f / cam.pixelSize[0];
    const float Hf = 1.0f / cam.pixelSize[1];
    switch (proj.kind) {
    case GMUPT_PROJ_ORTHOGRAPHIC: {
        const float halfH = proj.extent * 0.5f;
        const float halfW = halfH * (Wf / Hf);
        r.origin = (pos + right * (sx * halfW)) + up * (sy * halfH);
        r.direction = fn;
        break;
    }
    case GMUPT_PROJ_FISHEYE: {
        const float m = Wf < Hf ? Wf : Hf;
        const float ax = sx * (Wf / m);
        const float ay = sy * (Hf / m);
        const float rr = dsqrt(ax * ax + ay * ay);
        const float theta = rr * (proj.fov * 0.5f);
        if (rr == 0.0f) r.direction = fn;
        else if (rr > 1.0f) r.direction = mk3(0.0f, 0.0f, 0.0f);      // outside the image circle: a degenerate ray, a miss of everything
        else {
            const float c = dcos(theta);
            const float s = dsin(theta);
            r.direction = normalize3(fn * c + (right * (ax / rr) + up * (ay / rr)) * s);
        }
        break;
    }
    default: {   // GMUPT_PROJ_EQUIRECT
        const float lon = sx * 3.14159274f;
        const float lat = sy * 1.57079637f;
        const float cl = dcos(lat);
        r.direction = normalize3((fn * (cl * dcos(lon)) + right * (cl * dsin(lon))) + up * dsin(lat));
        break;
    }
    }
    return r;
}

// the ray of the fresh camera path at entry q of the new-path queue whose screen coordinate is the whole-frame pixel (cx, cy)
GM_HD CamRay projection_fresh_ray(const gmupt_camera_buffer& cam, const gmupt_projection& proj, uint32_t q, uint32_t cx, uint32_t cy)
{
    Rng g; g.seed(q, cam.randomSeed[0], cam.randomSeed[1]);     // newPath.hlsl:27,36-37
    const float jx = g.next() * 2.0f - 1.0f;
    const float jy = g.next() * 2.0f - 1.0f;
    const float u = ((float)cx + jx) * cam.pixelSize[0];
    const float v = ((float)cy + jy) * cam.pixelSize[1];
    return projection_ray(cam, proj, u, v);
}

// the un-jittered ray through whole-frame pixel coordinates (px, py)
GM_HD CamRay projection_pixel_ray(const gmupt_camera_buffer& cam, const gmupt_projection& proj, float px, float py)
{
    return projection_ray(cam, proj, px * cam.pixelSize[0], py * cam.pixelSize[1]);
}

// ray k (0 .. s*s - 1) of whole-frame pixel (x, y) at s samples per axis: the pixel-filter cell of AOV ray k + 1, the centre at s == 1
GM_HD CamRay projection_aov_ray(const gmupt_camera_buffer& cam, const gmupt_projection& proj, uint32_t x, uint32_t y, uint32_t s, uint32_t k)
{
    float px, py;
    aov_ray_coords(x, y, s, s > 1 ? k + 1 : 0u, px, py);
    return projection_pixel_ray(cam, proj, px, py);
}

// ---- host side (pt_projection.cpp)
// the argument errors of include/gmupt_projection.h as a message, nullptr for a projection that is admitted
const char* projection_fault(const gmupt_projection& proj);
// gmupt_projection_project_host with checked arguments: false = not on the image, (px, py) untouched
bool projection_project(const gmupt_camera_buffer& cam, const gmupt_projection& proj, const float world[3], double* px, double* py);

// ---- device side (pt_projection.hip)
// the launch between k_material (and k_ad_retarget) and the ray cast
void launch_proj_retarget(const RenderParams& p, const gmupt_projection& proj, hipStream_t s);
// rays: the chunk scratch of gmupt_render_aovs, 32 bytes per ray, pixel-major (ray k of chunk pixel j at j * s*s + k)
void launch_paov_raygen(const gmupt_camera_buffer& cam, const gmupt_projection& proj, uint32_t x0, uint32_t y0, uint32_t width, uint32_t rows, uint32_t samples,
                        gmupt_ray* rays, hipStream_t s);

} // namespace gmupt
