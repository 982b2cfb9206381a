/*
 * include/gmupt_adaptive.h -- the adaptive-sampling part of the C-ABI of libgmupt.so, an extension of include/gmupt.h with that
 * file's conventions (status returns, gmupt_last_error, creator owns).
 */
#ifndef GMUPT_ADAPTIVE_H
#define GMUPT_ADAPTIVE_H

#include "gmupt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Adaptive sampling: new camera paths go where the error still is (an extension; newPath.hlsl:33 sends path k to pixel k % (w*h)
 * for ever).  The convergence monitor says per pixel how far it is from the threshold; a PLAN turns that into a list of pixels, and a
 * renderer with a plan attached re-aims the camera paths k_material has just generated, in one extra launch between the shading stage
 * and the ray cast.  Opt-in everywhere: with no plan attached an iteration launches exactly what it launched before, no shipped
 * kernel is changed, and the oracle still defines every default frame.
 *
 * The rule (the host functions and the kernels run the same statements, csrc/pt_adaptive.hpp).
 *   Plan over a w*h rectangle -- the renderer's framebuffer rectangle, the tile of a tile renderer: list[0..count) of rectangle-local
 *     pixel indices y*w + x, and uniform_every (0 = off).
 *   Where path k goes.  k = lastPath + queueIndex in uint32 arithmetic, as newPath.hlsl:19,33.  With a plan attached and count > 0:
 *     uniform_every != 0 && k % uniform_every == 0: pix = k % (w*h), the reference's pixel.  Otherwise pix = list[k % count].
 *     Then cx = tileX0 + pix % w, cy = tileY0 + pix / w, and newPath.hlsl:36-43 follows with the same Rng seed (queueIndex,
 *     randomSeed), the same two next() draws and the same expressions.  Only the screen position and the ray direction of the slot
 *     are rewritten.  A path that the path_budget retired is left alone.  With count == 0, or no plan, nothing is re-aimed.
 *   Selection from the monitor's error plane (one float per pixel), a threshold T > 0 (finite) and max_repeat in 1..64.  Pixels are
 *     visited in ascending order; each contributes rep consecutive entries:
 *       rep = 0   err is NaN or +-inf: more samples do not repair a non-finite mean;
 *       rep = 1   err < 0: "unknown" (-1) and unsampled pixels.  The monitor never counts these as below, so this is asked before
 *       rep = 0   err <= T -- the comparison of the monitor's `below` count, csrc/pt_converge.hpp: "err <= prm.threshold";
 *       else      q = err / T;  m = q * q, both binary32 (nothing is added: nothing can be contracted);
 *                 rep = m >= (float)max_repeat ? max_repeat : max(1u, (uint32_t)ceilf(m)) -- the extra samples, in units of what the
 *                 pixel has, that would bring it to the threshold, capped.
 *     count = the sum of rep.  Summary (gmupt_adaptive_info): pixels; active = pixels with rep > 0; entries = count;
 *     skipped_nonfinite = pixels with a non-finite err; max_rep = the largest rep; ms = device time of the launches (0 on the host).
 *   Known bias.  Samples steered by an estimate made from the same samples bias the mean slightly: a pixel whose first batches
 *     happen to agree looks done and is starved.  uniform_every (every pixel keeps a share) and the monitor's min_batches are the
 *     guards; with uniform_every == 0 a pixel with rep = 0 gets NO further sample while the plan is attached.  A pixel that is at or
 *     below T with fewer than min_batches batches is not `below` for the monitor yet has rep = 0: it is served again once the list
 *     runs empty (count == 0 re-aims nothing), or through uniform_every.
 *   Other stages.  The AOV, denoiser, temporal and infill stages need no change: they read the per-pixel running mean and count of the
 *     accumulation target, which stay valid under uneven counts.
 * gmupt_adaptive_select_host / gmupt_adaptive_pixel_host: the selection and the mapping on the host, no device.  list_out may be NULL
 *   (the summary only); otherwise capacity >= entries is required.
 * gmupt_adaptive: a handle of a renderer, like gmupt_converge; it must not outlive the renderer.  The list, the run totals and their
 *   offsets are one device allocation, sized for pixels * max_repeat entries and grown on demand.
 * gmupt_adaptive_select: the selection on a device error plane of width*height floats (4-byte aligned; width*height is the rectangle
 *   the plan is for), on the renderer's stream: k_ad_count (one total per run of 256 pixels), k_ad_scan (one launch per level of 256
 *   totals), k_ad_emit; no atomics, no launch waits for another.  Then ONE readback of 16 bytes and a synchronise.  The handle then
 *   holds the plan (count, width, height, params->uniform_every).
 * gmupt_adaptive_set_list: a caller's own list (host memory; count may be 0) as the plan; every entry < width*height.
 * gmupt_adaptive_read_list: the plan's list into host memory; *count receives the entries (dst may be NULL to ask for the count).
 * gmupt_renderer_set_adaptive(r, a or NULL): attaches or detaches a plan.  An attached plan whose width*height is not the renderer's
 *   rectangle makes gmupt_iterate fail with GMUPT_ERR_INVALID_ARGUMENT before anything is launched.  gmupt_resize detaches;
 *   gmupt_adaptive_destroy of an attached plan detaches it first.  A plan stays attached across an iteration that clears the frame:
 *   at this level the caller decides.  gmupt_debug_run_stage(GMUPT_STAGE_SHADE) includes the re-aim.
 * gmupt_render_adaptive: the loop of gmupt_render_until with the plan in it.  After every check that does not end the loop:
 *   gmupt_converge_update into an error plane the adaptive handle owns, gmupt_adaptive_select on it, attach.  The plan is detached
 *   before an iteration that clears the frame (a restarted frame has no error plane yet), whenever the renderer's accumulation
 *   generation moved since the plan was made, and before returning.  aparams->threshold == 0 means the monitor's threshold.
 *   *ainfo = the last selection's summary, written only when one ran; *cinfo as gmupt_render_until.
 * Errors: GMUPT_ERR_INVALID_ARGUMENT for a NULL handle, plane, list or info, a misaligned plane, width*height == 0 or >= 2^32, a
 *   threshold that is not finite and > 0, max_repeat outside 1..64, width*height*max_repeat or count above 2^28 entries, capacity or
 *   bytes too small, a list entry >= width*height, a handle of another renderer, check_every == 0.  No error path allocates anything
 *   or writes an output. */
typedef struct { float threshold; uint32_t max_repeat, uniform_every; } gmupt_adaptive_params;   /* 12 bytes */
typedef struct { uint32_t pixels, active, entries, skipped_nonfinite, max_rep, pad; double ms; } gmupt_adaptive_info;   /* 32 bytes */
void gmupt_adaptive_default_params(gmupt_adaptive_params* p);   /* threshold 0 (there is no default threshold), max_repeat 1, uniform_every 0 */
int gmupt_adaptive_select_host(const float* error, uint32_t width, uint32_t height, const gmupt_adaptive_params* params, uint32_t* list_out /* may be NULL */,
                               size_t capacity, gmupt_adaptive_info* info);
int gmupt_adaptive_pixel_host(const uint32_t* list, uint32_t count, uint32_t uniform_every, uint32_t width, uint32_t height, uint32_t k, uint32_t* pix);
typedef struct gmupt_adaptive gmupt_adaptive;
int gmupt_adaptive_create(gmupt_renderer* r, gmupt_adaptive** out);
void gmupt_adaptive_destroy(gmupt_adaptive* a);
int gmupt_adaptive_select(gmupt_adaptive* a, const float* device_error, uint32_t width, uint32_t height, const gmupt_adaptive_params* params,
                          gmupt_adaptive_info* info);
int gmupt_adaptive_set_list(gmupt_adaptive* a, const uint32_t* host_list, uint32_t count, uint32_t width, uint32_t height, uint32_t uniform_every);
int gmupt_adaptive_read_list(gmupt_adaptive* a, uint32_t* dst /* may be NULL */, size_t bytes, uint32_t* count);
int gmupt_renderer_set_adaptive(gmupt_renderer* r, gmupt_adaptive* a_or_null);
int gmupt_render_adaptive(gmupt_renderer* r, gmupt_camera* camera, gmupt_converge* c, gmupt_adaptive* a, const gmupt_converge_params* cparams /* may be NULL */,
                          const gmupt_adaptive_params* aparams, uint32_t check_every, uint32_t max_iterations, uint32_t* iters /* may be NULL */,
                          gmupt_converge_info* cinfo, gmupt_adaptive_info* ainfo /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif
