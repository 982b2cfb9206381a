/*
 * include/gmupt_lens.h -- the thin-lens part of the C-ABI of libgmupt.so, an extension of include/gmupt.h with that file's
 * conventions (status returns, gmupt_last_error, creator owns).
 */
#ifndef GMUPT_LENS_H
#define GMUPT_LENS_H

#include "gmupt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Lens: depth of field (an extension; Camera.cpp and newPath.hlsl:36-41 of the reference are a pinhole -- every camera ray leaves
 * cam.position).  A renderer with a lens attached moves the origin of every camera path k_material has just generated onto a disk around
 * the camera position and aims it through the point where its pinhole ray meets the focal plane, in one extra launch between the shading
 * stage and the ray cast (after the re-aim of an attached sampling plan, include/gmupt_adaptive.h).  Opt-in everywhere: with no lens
 * attached, or aperture_radius == 0, an iteration launches exactly what it launched before, no shipped kernel is changed, and the oracle
 * still defines every default frame.
 *
 * The rule (the host function and the kernel run the same statements, csrc/pt_lens.hpp).  All arithmetic is binary32 in the written
 * order, nothing contracted; sin, cos and sqrt are detmath's (csrc/detmath.hpp), normalize3 and dot3 as everywhere else.
 *   Inputs: the camera buffer cam (pos = position, ulc = upperLeftCorner, hor = horizontal, ver = vertical, ps = pixelSize), the lens,
 *     the index q of the fresh path in the new-path queue, and its whole-frame pixel (cx, cy) as the path state holds it (screenCoord).
 *   1. The pinhole ray, newPath.hlsl:27,36-39 as the shading stage runs it:
 *        Rng g; g.seed(q, cam.randomSeed[0], cam.randomSeed[1]);
 *        jx = g.next()*2 - 1;  jy = g.next()*2 - 1;
 *        u = ((float)cx + jx) * ps.x;  v = ((float)cy + jy) * ps.y;
 *        d = normalize3((ulc + hor*u) - ver*v);          -- bit for bit the direction already in the slot
 *   2. The point on the lens, two more draws of the same generator:
 *        r1 = g.next();  r2 = g.next();
 *        rad = aperture_radius * sqrt(r1);  phi = r2 * 6.2831853f;
 *        lx = rad * cos(phi);  ly = rad * sin(phi);
 *   3. The camera frame:
 *        right = normalize3(hor);  up = normalize3(ver);
 *        F = (ulc + hor*0.5f) - ver*0.5f;  fn = normalize3(F);   -- the forward vector of the temporal projection
 *   4. The focal point:  t = focus_distance / dot3(d, fn);  Pf = pos + d*t;
 *   5. The new ray:      origin = (pos + right*lx) + up*ly;  direction = normalize3(Pf - origin).
 *   Only the ray origin and the ray direction of the slot are rewritten (six words).  Screen coordinates, throughput, pixel lists and
 *   queues stay as the shading stage left them; a path that the path_budget retired is left alone.  The lens reads (cx, cy) from the
 *   state, so it follows an attached sampling plan without knowing about it.
 * What stays a pinhole (a limit).  gmupt_pick, gmupt_camera_pick_ray, the AOV rays (gmupt_aov_ray, gmupt_render_aovs), the motion
 *   plane and the temporal projection stay on the centre ray through cam.position: the guide planes of a frame with depth of field
 *   are sharp where the beauty is not.  Lens-filtered AOV planes, the same record from rays through the lens, are an extension of
 *   their own: include/gmupt_lens_aov.h (gmupt_render_aovs_lens, gmupt_render_denoised_lens).
 * Accumulation.  Setting, changing or detaching a lens does NOT clear the frame by itself: the samples that follow are simply made
 *   with the new lens.  A caller that wants a clean frame restarts the accumulation (gmupt_camera_reset_accumulation, a camera whose
 *   iterationCounter is 0), as ProgressiveSession.set_lens, Renderer::setLens and gmupt_render do.
 * gmupt_renderer_set_lens(r, lens or NULL): attaches a copy of *lens; NULL or aperture_radius == 0 detaches.  The lens is
 *   resolution-independent: it survives gmupt_resize and gmupt_set_camera (a sampling plan does not survive a resize).
 *   gmupt_debug_run_stage(GMUPT_STAGE_SHADE) includes the lens launch.
 * gmupt_renderer_get_lens: the attached lens; { 0, focus_distance of gmupt_lens_default_params } when none is.
 * gmupt_lens_ray_host: the rule above on the host, no device; tmax = FLT_MAX, pad = 0.  aperture_radius == 0 is allowed here (the
 *   origin is then pos and the direction normalize3(Pf - pos), d up to rounding).
 * gmupt_lens_focus_at: autofocus.  gmupt_pick(r, px, py, light_count) on the renderer's current camera; on a hit (a triangle or a
 *   light sphere) inout->focus_distance = hit.t * dot3(pick direction, fn), the depth of the hit along the forward axis, and
 *   aperture_radius is left as it was.  On a miss (the pixel sees neither): GMUPT_ERR_INVALID_ARGUMENT, *inout untouched.  Nothing
 *   is attached: the caller passes *inout to gmupt_renderer_set_lens.  gmupt_pick's own errors (no scene, no camera, a ray cast
 *   without the wide tables) are returned as they are.
 * Errors: GMUPT_ERR_INVALID_ARGUMENT for a NULL renderer, camera, lens or result, an aperture_radius that is NaN, infinite or
 *   negative, and -- while aperture_radius > 0 -- a focus_distance that is NaN, infinite or not > 0.  No error path changes the
 *   attached lens or writes an output.
 * Lens and projection do not combine (include/gmupt_projection.h): the focal plane of step 4 has no meaning behind the camera.
 *   gmupt_renderer_set_lens returns GMUPT_ERR_UNSUPPORTED for aperture_radius > 0 while a projection other than the pinhole is
 *   attached, and gmupt_renderer_set_projection returns it while a lens with aperture_radius > 0 is.  With no projection attached
 *   gmupt_renderer_set_lens is what it was.
 * Extreme lenses.  A lens is checked for the errors above and for nothing else: every finite aperture_radius >= 0 and every finite
 *   focus_distance > 0 is admitted, denormals and FLT_MAX included, and the rule then runs as written, without a guard
 *   (tests/lens_extremes_util.py LENS_CLASSES is the table of such lenses; tests/test_lens_extremes_cpu.py
 *   test_every_class_holds_what_it_is_named_for counts what each produces, from gmupt_lens_ray_host alone).
 *   - Which rays come out.  The origin is always finite.  The direction is a unit vector, or (0, 0, 0), or NaN in at least one
 *     component, and nothing else: a lens offset or a focal distance t beyond about 1.84e19 makes dot3 inside normalize3 overflow, the
 *     length is +inf, 1 / inf is 0 and the direction is ZERO (aperture 1e30, focus 1e30; around the limit a lens gives both kinds,
 *     aperture 3e19 split by the draw r1, focus 1.5e19 split by the pixel); where d*t is itself infinite (focus near FLT_MAX) inf * 0
 *     is NaN, and where Pf rounds onto the origin (a tiny focus with the draw r1 = 0; a tiny focus with a tiny aperture) the zero vector
 *     times 1 / 0 is NaN.  A denormal aperture gives ordinary rays whose denormal lens offset is kept, not flushed (visible only with
 *     cam.position at the origin: pos + 1e-45 is pos elsewhere).  An aperture up to 1.5e19 gives ordinary rays from that far away.
 *     (test_every_class_holds_what_it_is_named_for, test_a_denormal_aperture_moves_the_origin_only_of_a_camera_at_the_origin)
 *   - What such rays get.  A ray with a zero or NaN direction is a ray of include/gmupt.h "Degenerate rays": it misses every triangle
 *     and light, in the renderer's own ray casts (both shipped kernels) as for caller rays, no fault flag is raised, its path ends in
 *     the next shading stage with the environment colour, and the frame stays finite.  A renderer whose lens gives only such rays
 *     renders the environment.  Ordinary rays from 1e18 away get what the oracle gives them, to the bit (mostly a light sphere: its
 *     test cancels from that far).  (tests/test_lens_extremes_cpu.py test_the_oracle_alone_on_the_lens_rays;
 *     tests/test_lens_extremes_gpu.py test_whole_iterations_equal_the_oracle)
 *   - Host and device.  gmupt_lens_ray_host and the renderer's lens launch agree bit for bit on every such lens except in the sign and
 *     payload of a generated NaN, which neither IEEE 754 nor this library pins; which words are NaN is the same.  (On the MI355X
 *     against an x86 host even those agreed: 0xffc00000 on both.)  (tests/test_lens_extremes_gpu.py test_stage_holds_the_host_rays; the numpy restatements against the host rule:
 *     tests/test_lens_extremes_cpu.py test_host_rules_equal_the_restatements_on_every_class)
 *   - The guards of the lens launch (queue length, live paths, path budget) do not depend on the lens, and hold together with a tile
 *     origin and a sampling plan.  (tests/test_lens_extremes_gpu.py test_tile_budget_and_plan_together) */
typedef struct { float aperture_radius; float focus_distance; } gmupt_lens;   /* 8 bytes; scene units */
void gmupt_lens_default_params(gmupt_lens* lens);   /* aperture_radius 0 (a pinhole), focus_distance 1 */
int gmupt_renderer_set_lens(gmupt_renderer* r, const gmupt_lens* lens_or_null);
int gmupt_renderer_get_lens(gmupt_renderer* r, gmupt_lens* out);
int gmupt_lens_ray_host(const gmupt_camera_buffer* cam, const gmupt_lens* lens, uint32_t q, uint32_t cx, uint32_t cy, gmupt_ray* out);
int gmupt_lens_focus_at(gmupt_renderer* r, float px, float py, uint32_t light_count, gmupt_lens* inout);

#ifdef __cplusplus
}
#endif
#endif
