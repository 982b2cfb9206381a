/*
 * include/gmupt_shutter.h -- the shutter part of the C-ABI of libgmupt.so, an extension of include/gmupt.h with that file's
 * conventions (status returns, gmupt_last_error, creator owns).
 */
#ifndef GMUPT_SHUTTER_H
#define GMUPT_SHUTTER_H

#include "gmupt.h"
#include "gmupt_lens.h"
#include "gmupt_projection.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Shutter: camera motion blur (an extension; the reference takes every frame at one instant).  The renderer's camera
 * (gmupt_set_camera) is the pose at shutter open, t = 0; an attached shutter carries the pose at shutter close, t = 1.  Every fresh camera
 * path draws a time in [0, 1) and its ray is made from the camera interpolated to that time, by the pinhole rule, the attached lens
 * (include/gmupt_lens.h) or the attached projection (include/gmupt_projection.h).  One launch between the shading stage and the ray cast
 * (after the re-aim of an attached sampling plan), IN PLACE OF the lens's or the projection's.  Opt-in everywhere: with no shutter
 * attached an iteration launches exactly what it launched before, no shipped kernel is changed, and the oracle still defines every
 * default frame.  The shutter is a box: every time is as likely as every other.  Geometry does not move during the exposure (no geometry
 * motion blur: that needs a time in the ray cast).
 *
 * The rule (the host functions and the kernel run the same statements, csrc/pt_shutter.hpp).  All arithmetic is binary32 in the written
 * order, nothing contracted.
 *   Inputs: the camera buffer cam, the close pose sh (position, upperLeftCorner, horizontal, vertical), the index q of the fresh path in
 *     the new-path queue, and its whole-frame pixel (cx, cy) as the path state holds it (screenCoord).
 *   1. The time:  Rng g; g.seed(q, cam.randomSeed[0], cam.randomSeed[1]);  four draws are made and discarded;  t = g.next().
 *        It is the fifth draw of the generator whose first two are the jitter and whose third and fourth are the lens point, so the time
 *        of a path is the same number whether a lens, a projection or neither is attached.  (gmupt_shutter_time_host)
 *   2. The camera at t:  for each of the twelve components of position, upperLeftCorner, horizontal and vertical (x, y, z of each)
 *        c = a + (b - a) * t,  a from cam, b from sh.
 *        pixelSize, randomSeed, envColor, the counts, the fourth word of each vector and everything else are cam's.
 *        (gmupt_shutter_camera_host)
 *   3. The ray: the attached rule on that camera with the same (q, cx, cy) -- with a lens gmupt_lens_ray_host's rule, with a projection
 *        gmupt_projection_ray_host's, with neither the pinhole: origin = the interpolated position, direction = step 1 of the lens rule
 *        (d = normalize3((ulc + hor*u) - ver*v) on the jittered coordinates).  Not the lens rule at aperture 0: its direction is d only
 *        up to rounding.
 *   Only the ray origin and the ray direction of the slot are rewritten (six words), as by the lens.  A path that the path_budget retired
 *   is left alone; (cx, cy) is read from the state, so the shutter follows an attached sampling plan and a tile origin.
 * Identity.  A close pose bit-equal to the camera's gives c = a + 0 * t = a: without a lens the six words are those the shading stage
 *   wrote, and the frame is the frame without a shutter.  One exception: a component of cam that is -0.0 comes out as +0.0
 *   (-0.0 + +0.0).  Such a shutter is allowed and stays attached.
 * Linear, not spherical (a limit).  The three image-plane vectors are interpolated component by component; there is no slerp.  Where the
 *   camera turns by an angle theta across the shutter, the parts of upperLeftCorner, horizontal and vertical that turn are shorter at
 *   an inner time than at the ends, by the factor cos(theta/2) at mid-shutter where it is smallest, while the parts along the axis of rotation
 *   keep their length.  A yaw therefore leaves the horizontal field of view as it is (forward and horizontal shrink together) and widens
 *   the tangent of the vertical one by 1 / cos(theta/2) at mid-shutter; a pitch does the same to the horizontal one.  The error reaches
 *   1 % at theta = 2 acos(0.99) = 16.2 degrees, 0.1 % at 5.1 degrees.  The directions are normalised, so the rays stay unit vectors.  The
 *   lens frame (right, up, fn) is renormalised by the lens rule; its focus distance is measured along the interpolated forward axis.
 * What stays at t = 0 (a limit).  gmupt_pick, gmupt_camera_pick_ray, gmupt_lens_focus_at, every AOV call (gmupt_render_aovs, _lens,
 *   _projected and the denoisers on them), the motion plane and the temporal projection use cam as set: the guide planes of a blurred
 *   frame are sharp.  Time-stratified guides would follow include/gmupt_lens_aov.h and are not part of this extension.
 * Accumulation.  Setting, changing or detaching a shutter does NOT clear the frame by itself: the samples that follow are simply made
 *   with the new shutter.  A caller that wants a clean frame restarts the accumulation, as ProgressiveSession.set_shutter,
 *   Renderer::setShutter and gmupt_render do.
 * gmupt_renderer_set_shutter(r, shutter or NULL): attaches a copy of *shutter; NULL detaches.  The shutter is a value on the renderer:
 *   it survives gmupt_set_camera (the close pose stays where it was put while the open pose follows the camera), and gmupt_resize
 *   detaches it, because the aspect changes `horizontal`, as it detaches a sampling plan.  Lens and projection still refuse each other
 *   exactly as before; either may be attached, changed or detached while a shutter is.  gmupt_debug_run_stage(GMUPT_STAGE_SHADE)
 *   includes the shutter launch.
 * gmupt_renderer_get_shutter: *attached = 1 and the attached close pose, or *attached = 0 and *out all zero.
 * gmupt_shutter_from_camera: the close pose of a camera buffer (the first three words of its four vectors).
 * gmupt_shutter_camera_host / _time_host / _ray_host: steps 2, 1 and the whole rule on the host, no device; the ray has tmax = FLT_MAX,
 *   pad = 0.  _ray_host takes the lens or the projection of step 3, or neither (both NULL: the pinhole); a lens with aperture_radius 0 is
 *   allowed there and runs the lens rule, as in gmupt_lens_ray_host.
 * Errors: GMUPT_ERR_INVALID_ARGUMENT for a NULL renderer, camera, shutter or result, a close pose with a component that is NaN or
 *   infinite, a time that is NaN or infinite (gmupt_shutter_camera_host), a lens or a projection that its own header refuses, and both a
 *   lens and a projection passed to gmupt_shutter_ray_host.  No error path changes the attached shutter or writes an output. */
typedef struct { float position[3]; float upperLeftCorner[3]; float horizontal[3]; float vertical[3]; } gmupt_shutter;   /* 48 bytes; the pose at t = 1 */
int gmupt_renderer_set_shutter(gmupt_renderer* r, const gmupt_shutter* shutter_or_null);
int gmupt_renderer_get_shutter(gmupt_renderer* r, gmupt_shutter* out, int* attached);
int gmupt_shutter_from_camera(const gmupt_camera_buffer* close, gmupt_shutter* out);
int gmupt_shutter_camera_host(const gmupt_camera_buffer* cam, const gmupt_shutter* shutter, float t, gmupt_camera_buffer* out);
int gmupt_shutter_time_host(const gmupt_camera_buffer* cam, uint32_t q, float* t);
int gmupt_shutter_ray_host(const gmupt_camera_buffer* cam, const gmupt_shutter* shutter, const gmupt_lens* lens_or_null, const gmupt_projection* projection_or_null,
                           uint32_t q, uint32_t cx, uint32_t cy, gmupt_ray* out);

#ifdef __cplusplus
}
#endif
#endif
