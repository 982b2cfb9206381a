// Temporal reuse (gmupt_temporal_denoise_image, gmupt_render_denoised_temporal; include/gmupt.h states it)
//
//   k_tp_integrate  one thread per pixel, 64x4 blocks like k_dn_atrous: the beauty texel and the AOV record, the projection into the
//                   previous camera, the four bilinear tap records (loaded before they are tested), the blend -> the integrated texel
//                   and the pixel's new history record
//   k_tp_integrate_mv  the same with the pixel's gmupt_motion record as a fifth load (16 B): a record with flags == 1 moves the projected
//                   point and the origin of the taps' plane test to prev_position (gmupt_temporal_denoise_image_motion)
//
// The denoiser's launches (launch_denoise) follow on the integrated image, unchanged, with no host synchronisation in between.  The
// per-pixel arithmetic is pt_temporal.hpp, which the host integration (pt_temporal.cpp) runs too.
#include "pt_kernel_util.hpp"
#include "pt_temporal.hpp"
#include "pt_launch.hpp"

namespace gmupt {

struct TpArgs { const float4* beauty; const float4* aov; TpPrev prev; TpParams prm; float4* out; float4* hist; int W, H; };

__global__ __launch_bounds__(kTileX * kTileY) void k_tp_integrate(TpArgs a)
{
    int x, y;
    if (!tile_pixel(a.W, a.H, x, y)) return;
    const size_t p = (size_t)y * a.W + x;
    const float4* rec = a.aov + 4 * p;
    float4 o, r0, r1, r2;
    tp_pixel(a.beauty[p], rec[0], rec[1], rec[2], rec[3], a.prev, a.prm, o, r0, r1, r2);
    a.out[p] = o;
    a.hist[3 * p] = r0; a.hist[3 * p + 1] = r1; a.hist[3 * p + 2] = r2;
}

__global__ __launch_bounds__(kTileX * kTileY) void k_tp_integrate_mv(TpArgs a, const float4* motion)
{
    int x, y;
    if (!tile_pixel(a.W, a.H, x, y)) return;
    const size_t p = (size_t)y * a.W + x;
    const float4* rec = a.aov + 4 * p;
    float4 o, r0, r1, r2;
    tp_pixel_t<true>(a.beauty[p], rec[0], rec[1], rec[2], rec[3], motion[p], a.prev, a.prm, o, r0, r1, r2);
    a.out[p] = o;
    a.hist[3 * p] = r0; a.hist[3 * p + 1] = r1; a.hist[3 * p + 2] = r2;
}

// ---- host launcher (gmupt_capi.hip: gmupt_temporal_denoise_image).  beauty / out: W*H float4; aov: W*H records of 4 float4; hist: W*H
// records of 3 float4 (must not be prev.rec); W*H <= 2^28.
void launch_temporal(const float4* beauty, const float4* aov, int W, int H, const TpPrev& prev, const TpParams& prm, float4* out, float4* hist,
                     hipStream_t s)
{
    const TileDims t = tile_dims(W, H);
    TpArgs a{ beauty, aov, prev, prm, out, hist, W, H };
    hipLaunchKernelGGL(k_tp_integrate, t.grid, t.block, 0, s, a);
}

// the same with a motion plane: W*H float4 (gmupt_temporal_denoise_image_motion)
void launch_temporal_motion(const float4* beauty, const float4* aov, const float4* motion, int W, int H, const TpPrev& prev, const TpParams& prm,
                            float4* out, float4* hist, hipStream_t s)
{
    const TileDims t = tile_dims(W, H);
    TpArgs a{ beauty, aov, prev, prm, out, hist, W, H };
    hipLaunchKernelGGL(k_tp_integrate_mv, t.grid, t.block, 0, s, a, motion);
}

} // namespace gmupt
