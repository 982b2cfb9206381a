/*
 * include/gmupt_lens_aov.h -- lens-filtered AOV planes: the guide records of a frame with depth of field.  An extension of
 * include/gmupt.h (the gmupt_aov record, gmupt_render_aovs, gmupt_render_denoised) and include/gmupt_lens.h (the thin lens), with
 * their conventions (status returns, gmupt_last_error, creator owns).
 */
#ifndef GMUPT_LENS_AOV_H
#define GMUPT_LENS_AOV_H

#include "gmupt_lens.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Lens AOVs.  gmupt_render_aovs looks through the pinhole: every field but the filtered albedo / normal comes from the centre ray
 * through cam.position.  With a lens attached the beauty of a pixel is a mix of everything its lens rays see, so next to an
 * out-of-focus silhouette the pinhole record is sharp where the beauty is a ramp, and a pixel whose centre ray misses is not a surface
 * pixel for the image stages although blurred foreground reaches it.  gmupt_render_aovs_lens writes the same 64-byte gmupt_aov record
 * from R = s*s rays through the lens, so the denoiser, the temporal integration and the infill take it as they are.  Opt-in: with none
 * of the functions below called, every launch of the library is what it was, and no shipped kernel is changed.
 *
 * The rays (the host function and k_laov_raygen run the same statements, csrc/pt_lens_aov.hpp).  All arithmetic is binary32 in the
 * written order, nothing contracted; sin, cos and sqrt are detmath's.  s = samples (1..GMUPT_AOV_MAX_SAMPLES), A = aperture_radius,
 * F = focus_distance.  Per whole-frame pixel (x, y) there are R = s*s rays and no centre ray; ray k = b*s + a (a, b in 0..s-1):
 *   1. The pixel-filter cell (a, b) of the AOV rays: for s > 1 the coordinates (px, py) of ray k + 1 of gmupt_aov_ray,
 *        px = (float)x + ((float)(2*a + 1)/(float)s - 1.0f);  py = (float)y + ((float)(2*b + 1)/(float)s - 1.0f);
 *      for s == 1 the pixel centre, px = (float)x, py = (float)y.  d = the direction of gmupt_camera_pick_ray(cam, px, py).
 *   2. The lens stratum (a2, b2) = (b, s - 1 - a): a fixed bijection of the s*s cells, the same in every pixel (the transpose,
 *      mirrored), so that every lens stratum is used exactly once per pixel, no pixel draws a random number, the planes carry no
 *      per-pixel noise, and the lens coordinate is not tied to the like-named pixel coordinate.
 *        r1 = ((float)a2 + 0.5f)/(float)s;  r2 = ((float)b2 + 0.5f)/(float)s;
 *        rad = A * sqrt(r1);  phi = r2 * 6.2831853f;  lx = rad * cos(phi);  ly = rad * sin(phi);
 *   3.-5. Steps 3, 4 and 5 of the lens rule of include/gmupt_lens.h on d: the frame right / up / fn, Pf = pos + d*(F/dot3(d, fn)),
 *        origin = (pos + right*lx) + up*ly,  direction = normalize3(Pf - origin).  tmax = FLT_MAX, pad = 0.
 *   gmupt_aov_lens_ray returns exactly these rays (host only).
 *   Aperture 0 is accepted: origin is then pos and direction normalize3(Pf - pos), the stratified pinhole ray d up to the rounding of
 *   that round trip.  The records are then those of the s*s stratified pinhole rays up to that rounding; bit equality with
 *   gmupt_render_aovs is NOT promised (and its centre ray does not exist here).
 *
 * Per-ray shading is that of gmupt_render_aovs: the closest hit of the ray with the light spheres up to cam.lightCount; a *surface
 * sample* is a triangle hit without a nearer light, shaded by the material (textures, and the normal map oriented by the ray's own
 * direction); a light sample has the light's colour, a miss cam.envColor, both with normal, roughness and metallic 0.
 *
 * The record (gmupt_aov; every sum starts at 0.0f and runs in k order, every mean is sum / (float)count):
 *   albedo     sum over all R rays / (float)R (miss = env, light = light colour)
 *   normal     sum over all R rays / (float)R, a non-surface sample adds 0.0f
 *   coverage   the number of surface samples, 0..R
 *   coverage > 0:
 *     depth      sum over the surface samples of t_k / (float)coverage
 *     position   sum over the surface samples of (origin_k + direction_k * t_k) / (float)coverage
 *     roughness, metallic   sum over the surface samples of the sample's value / (float)coverage
 *     triangle, material    those of the first surface sample in k order;  light = 0
 *   coverage == 0:
 *     depth, position, triangle, material, light, roughness, metallic come from ray k = 0 exactly as gmupt_render_aovs treats its
 *     centre ray (position = origin + direction*t at a light, 0 on a miss; roughness = metallic = 0).
 *   For the image stages (gd_prepare) a pixel is therefore a surface pixel exactly when some lens ray saw a surface and the mean
 *   normal is not zero: triangle >= 0 and light == 0 hold exactly when coverage > 0.
 *
 * gmupt_render_aovs_lens: the records of the renderer's rectangle (the tile in tile mode) under `lens_or_null`; NULL means the lens
 *   attached to the renderer (none attached: aperture 0).  Three launches per chunk of pixel rows as gmupt_render_aovs, on its chunk
 *   scratch: k_laov_raygen, the wide ray cast, k_laov_resolve.  A row must fit a chunk: width * s*s <= GMUPT_AOV_CHUNK_RAYS.  The
 *   renderer's frame, path state, queues, counters, statistics and attached lens are not touched.  out: device memory, 16-byte
 *   aligned, width * height records.  info as gmupt_render_aovs.
 * gmupt_render_denoised_lens: gmupt_render_denoised with these records in place of the pinhole ones, through the same scratch.
 * What stays a pinhole (limits): gmupt_render_aovs_motion and the motion plane, gmupt_pick, gmupt_lens_focus_at, and the temporal
 *   projection, which reprojects the record's position -- here a mean over the surface samples.
 * Errors: those of gmupt_render_aovs (gmupt_render_denoised) with `samples` checked against s*s rays per pixel, and the lens checks
 *   of gmupt_renderer_set_lens on a lens that is given.  gmupt_aov_lens_ray: GMUPT_ERR_INVALID_ARGUMENT for a NULL camera, lens or
 *   result, a bad lens, samples outside 1..GMUPT_AOV_MAX_SAMPLES or k >= s*s.  No error path writes an output.
 * Extreme lenses: include/gmupt_lens.h, "Extreme lenses", holds here too -- steps 3-5 are the same statements, so an admitted lens can
 *   give these rays a zero or a NaN direction.  Such a ray misses everything and is never a surface sample: it adds cam.envColor to
 *   the albedo sum and nothing to the others, so no record holds a NaN because of it; a pixel whose every ray is one has coverage 0,
 *   position (0, 0, 0) and the miss record of ray k = 0, is no surface pixel, and gmupt_render_denoised_lens on a frame of such
 *   pixels returns the beauty bit for bit.  (tests/test_lens_extremes_gpu.py test_lens_aov_records_equal_the_oracle,
 *   test_denoiser_copies_a_frame_without_a_surface_pixel, test_denoiser_on_the_mixed_records; the rays on the host:
 *   tests/test_lens_extremes_cpu.py test_host_rules_equal_the_restatements_on_every_class) */
int gmupt_render_aovs_lens(gmupt_renderer* r, const gmupt_lens* lens_or_null, uint32_t samples, gmupt_aov* out, size_t bytes, gmupt_trace_info* info);
int gmupt_aov_lens_ray(const gmupt_camera_buffer* cam, const gmupt_lens* lens, uint32_t x, uint32_t y, uint32_t samples, uint32_t k, gmupt_ray* out);
int gmupt_render_denoised_lens(gmupt_renderer* r, const gmupt_lens* lens_or_null, uint32_t aov_samples, const gmupt_denoise_params* p, float* out_rgba,
                               size_t bytes, gmupt_trace_info* info);

#ifdef __cplusplus
}
#endif
#endif
