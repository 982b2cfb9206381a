/*
 * include/gmupt_projection.h -- camera projections: orthographic, equidistant fisheye and 360-degree equirectangular panorama.  An
 * extension of include/gmupt.h with that file's conventions (status returns, gmupt_last_error, creator owns).
 */
#ifndef GMUPT_PROJECTION_H
#define GMUPT_PROJECTION_H

#include "gmupt_lens.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Projections (an extension; Camera.cpp and newPath.hlsl:36-41 of the reference are a perspective pinhole).  A renderer with a
 * projection attached gives every camera path k_material has just generated the ray of that projection, in one extra launch between
 * the shading stage and the ray cast (after the re-aim of an attached sampling plan, include/gmupt_adaptive.h; where the lens launch
 * would be, include/gmupt_lens.h).  After ray generation a camera ray is just a ray: no shipped kernel is changed.  Opt-in everywhere:
 * with no projection attached (kind GMUPT_PROJ_PINHOLE) an iteration launches exactly what it launched before, and the oracle still
 * defines every default frame.
 *
 * The rule (the host functions and the kernels run the same statements, csrc/pt_projection.hpp: projection_ray).  All arithmetic is
 * binary32 in the written order, nothing contracted; sin, cos and sqrt are detmath's (csrc/detmath.hpp), normalize3 as everywhere
 * else.  The forward rule uses no inverse trigonometric function.
 *   Inputs: the camera buffer cam (pos = position, ulc = upperLeftCorner, hor = horizontal, ver = vertical, ps = pixelSize), the
 *     projection, and the screen coordinates (u, v) that the pinhole feeds into (ulc + hor*u) - ver*v: u = px * ps.x, v = py * ps.y
 *     for whole-frame pixel coordinates (px, py), in tile mode too (a tile's pixels are whole-frame pixels).
 *     sx = 2.0f*u - 1.0f;  sy = 1.0f - 2.0f*v;                          -- (-1, 1) is the upper left corner of the frame
 *     right = normalize3(hor);  up = normalize3(ver);  fn = normalize3((ulc + hor*0.5f) - ver*0.5f);   -- step 3 of the lens rule
 *     Wf = 1.0f / ps.x;  Hf = 1.0f / ps.y;                              -- the whole-frame size as floats, not truncated
 *   GMUPT_PROJ_PINHOLE:  origin = pos;  direction = normalize3((ulc + hor*u) - ver*v)       -- gmupt_camera_pick_ray
 *   GMUPT_PROJ_ORTHOGRAPHIC (extent > 0: the world-space height of the view):
 *     halfH = extent*0.5f;  halfW = halfH * (Wf/Hf);
 *     origin = (pos + right*(sx*halfW)) + up*(sy*halfH);  direction = fn.
 *   GMUPT_PROJ_FISHEYE (equidistant; fov in (0, 2 pi], the angle across the image circle, which is inscribed in the shorter side):
 *     m = Wf < Hf ? Wf : Hf;  ax = sx * (Wf/m);  ay = sy * (Hf/m);
 *     r = sqrt(ax*ax + ay*ay);  theta = r * (fov*0.5f);  origin = pos;
 *     r == 0:  direction = fn.
 *     r > 1:   direction = (0, 0, 0): outside the image circle.  Under "Degenerate rays" (include/gmupt.h) such a ray misses every
 *              triangle and light, raises no fault flag, and its path ends with cam.envColor.
 *     else:    direction = normalize3(fn*cos(theta) + (right*(ax/r) + up*(ay/r)) * sin(theta)).
 *   GMUPT_PROJ_EQUIRECT (any aspect ratio; 2:1 gives square angular pixels):
 *     lon = sx * 3.14159274f;  lat = sy * 1.57079637f;  cl = cos(lat);  origin = pos;
 *     direction = normalize3((fn*(cl*cos(lon)) + right*(cl*sin(lon))) + up*sin(lat)).
 *   A fresh path: the jittered (u, v) of entry q of the new-path queue at whole-frame pixel (cx, cy), newPath.hlsl:27,36-37 as the
 *     shading stage runs it (step 1 of the lens rule): Rng g; g.seed(q, cam.randomSeed[0], cam.randomSeed[1]);
 *     jx = g.next()*2 - 1;  jy = g.next()*2 - 1;  u = ((float)cx + jx) * ps.x;  v = ((float)cy + jy) * ps.y.
 *   Only the ray origin and the ray direction of the slot are rewritten (six words); a path that the path_budget retired is left
 *   alone.  The launch reads (cx, cy) from the state, so it follows a tile origin and an attached sampling plan without knowing them.
 * Lens and projection do not combine: the thin lens focuses on a plane (focus_distance / dot3(d, fn)), which has no meaning behind the
 *   camera.  gmupt_renderer_set_projection returns GMUPT_ERR_UNSUPPORTED while a lens with aperture_radius > 0 is attached, and
 *   gmupt_renderer_set_lens returns it for aperture_radius > 0 while a projection other than the pinhole is attached.
 * Accumulation.  Setting, changing or detaching a projection does NOT clear the frame by itself (as the lens): a caller that wants a
 *   clean frame restarts the accumulation, as ProgressiveSession.set_projection, Renderer::setProjection and gmupt_render do.
 * gmupt_renderer_set_projection(r, proj or NULL): attaches a copy; NULL or kind GMUPT_PROJ_PINHOLE detaches.  The projection survives
 *   gmupt_resize and gmupt_set_camera.  gmupt_debug_run_stage(GMUPT_STAGE_SHADE) includes its launch.
 * gmupt_renderer_get_projection: the attached projection; gmupt_projection_default_params' value when none is.
 * gmupt_projection_ray_host: the fresh-path ray above on the host, no device; tmax = FLT_MAX, pad = 0.
 * gmupt_projection_pick_ray: the un-jittered ray through whole-frame pixel coordinates (px, py), u = px*ps.x, v = py*ps.y: the
 *   counterpart of gmupt_camera_pick_ray, and that function's ray for the pinhole.
 * gmupt_projection_project_host: the inverse, a world point to whole-frame pixel coordinates.  Host only, binary64 with the C
 *   library's functions, NO bit-for-bit promise.  Returns GMUPT_OK and sets *on_image to 1 with (*px, *py) written, or to 0 with
 *   them left alone when the point is not on the image: at the camera position, behind or in the plane of an orthographic, a pinhole
 *   or a fisheye of fov <= pi camera, outside the image circle.  Points outside the frame's rectangle but on the projection's plane are on
 *   the image (their coordinates lie outside [0, W] x [0, H]).  It is for callers and for the round-trip test; the temporal projection
 *   does not use it.
 * gmupt_pick_projected: gmupt_pick on gmupt_projection_pick_ray of the attached projection.
 * gmupt_aov_projected_ray (host only): ray k = b*s + a of the R = s*s stratified rays of whole-frame pixel (x, y): the pixel-filter
 *   cell (a, b) of gmupt_aov_ray's ray k + 1 for s > 1, the pixel centre at s == 1 (step 1 of include/gmupt_lens_aov.h), through
 *   the un-jittered rule.  There is no centre ray, as the lens records have none.
 * gmupt_render_aovs_projected(r, proj or NULL, ...): the 64-byte gmupt_aov records of the renderer's rectangle under the projection
 *   (NULL: the attached one): k_paov_raygen, the wide ray cast and the resolve of gmupt_render_aovs_lens, the record rule of
 *   include/gmupt_lens_aov.h word for word, on the chunk scratch and with the chunking and errors of that function.  For an
 *   orthographic projection the origin differs per ray: `position` is still the mean of origin_k + direction_k * t_k over the surface
 *   samples, the surface point, and `depth` the mean of t_k, the distance from the ray's own origin on the camera plane (not from
 *   cam.position).  A fisheye pixel outside the image circle is a miss record: albedo = cam.envColor, coverage 0, position 0.
 *   With the pinhole kind (given, or NULL with nothing attached) these are the records of the s*s stratified PINHOLE rays without a
 *   centre ray: NOT the records of gmupt_render_aovs, whose depth, position and ids come from its centre ray.
 * gmupt_render_denoised_projected: gmupt_render_denoised with these records in place of the pinhole ones.
 * gmupt_debug_read_aov_rays (a debug access, for the tests): copies the first `count` gmupt_ray records of the renderer's AOV chunk
 *   scratch to host memory -- after a gmupt_render_aovs* call whose frame fits one chunk, the rays its ray generation wrote, pixel-major
 *   (ray k of pixel j at j * R + k).  GMUPT_ERR_NOT_BOUND before any AOV call, GMUPT_ERR_INVALID_ARGUMENT for count > GMUPT_AOV_CHUNK_RAYS.
 * What stays a pinhole (limits): the temporal projection (gmupt_render_denoised_temporal*, k_tp_integrate inverts a pinhole), the
 *   motion plane, gmupt_render_aovs, gmupt_pick and gmupt_lens_focus_at.  No anamorphic squeeze, no stereo or cube-map layouts.
 * Errors: GMUPT_ERR_INVALID_ARGUMENT for a NULL renderer, camera, projection or result, an unknown kind, for the fisheye a fov that
 *   is NaN, infinite, not > 0 or > 6.28318548f (2 pi as binary32), for the orthographic an extent that is NaN, infinite or not > 0;
 *   each check applies only to the kind that uses the field.  gmupt_aov_projected_ray: samples outside 1..GMUPT_AOV_MAX_SAMPLES or
 *   k >= s*s.  No error path changes the attached projection or writes an output. */
enum { GMUPT_PROJ_PINHOLE = 0, GMUPT_PROJ_ORTHOGRAPHIC = 1, GMUPT_PROJ_FISHEYE = 2, GMUPT_PROJ_EQUIRECT = 3 };
typedef struct { uint32_t kind; float fov; float extent; uint32_t pad; } gmupt_projection;   /* 16 bytes; fov in radians, extent in scene units */
void gmupt_projection_default_params(gmupt_projection* proj);   /* kind GMUPT_PROJ_PINHOLE, fov pi (a hemisphere), extent 1, pad 0 */
int gmupt_renderer_set_projection(gmupt_renderer* r, const gmupt_projection* proj_or_null);
int gmupt_renderer_get_projection(gmupt_renderer* r, gmupt_projection* out);
int gmupt_projection_ray_host(const gmupt_camera_buffer* cam, const gmupt_projection* proj, uint32_t q, uint32_t cx, uint32_t cy, gmupt_ray* out);
int gmupt_projection_pick_ray(const gmupt_camera_buffer* cam, const gmupt_projection* proj, float px, float py, gmupt_ray* out);
int gmupt_projection_project_host(const gmupt_camera_buffer* cam, const gmupt_projection* proj, const float world[3], double* px, double* py, int* on_image);
int gmupt_pick_projected(gmupt_renderer* r, float px, float py, uint32_t light_count, gmupt_ray* ray_out, gmupt_hit* hit_out);
int gmupt_aov_projected_ray(const gmupt_camera_buffer* cam, const gmupt_projection* proj, uint32_t x, uint32_t y, uint32_t samples, uint32_t k, gmupt_ray* out);
int gmupt_render_aovs_projected(gmupt_renderer* r, const gmupt_projection* proj_or_null, uint32_t samples, gmupt_aov* out, size_t bytes, gmupt_trace_info* info);
int gmupt_debug_read_aov_rays(gmupt_renderer* r, gmupt_ray* host_out, uint32_t count);
int gmupt_render_denoised_projected(gmupt_renderer* r, const gmupt_projection* proj_or_null, uint32_t aov_samples, const gmupt_denoise_params* p,
                                    float* out_rgba, size_t bytes, gmupt_trace_info* info);

#ifdef __cplusplus
}
#endif
#endif
