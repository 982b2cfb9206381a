// Temporal reuse (gmupt_temporal_denoise_image, gmupt_render_denoised_temporal, gmupt_temporal_integrate_host; include/gmupt.h states it)
//
//   k_tp_integrate  one thread per pixel, 64x4 blocks like k_dn_atrous: the beauty texel and the AOV record, the projection into the
//                   previous camera, the four bilinear tap records (loaded before they are tested), the blend -> the integrated texel
//                   and the pixel's new history record
//   k_tp_integrate_mv  the same with the pixel's gmupt_motion record as a fifth load (16 B): a record with flags == 1 moves the projected
//                   point and the origin of the taps' plane test to prev_position (gmupt_temporal_denoise_image_motion)
//
// The denoiser's launches (launch_denoise) follow on the integrated image, unchanged, with no host synchronisation in between.  The
// per-pixel arithmetic is pt_temporal.hpp, which the host integration below runs too.
#include "pt_device.hpp"
#include "detmath.hpp"
#include "pt_denoise.hpp"
#include "pt_temporal.hpp"
#include "pt_launch.hpp"

#include <cstring>
#include <vector>

namespace gmupt {

constexpr int kTpBX = 64, kTpBY = 4;

struct TpArgs { const float4* beauty; const float4* aov; TpPrev prev; TpParams prm; float4* out; float4* hist; int W, H; };

__global__ __launch_bounds__(kTpBX * kTpBY) void k_tp_integrate(TpArgs a)
{
    const int x = blockIdx.x * kTpBX + threadIdx.x, y = blockIdx.y * kTpBY + threadIdx.y;
    if (x >= a.W || y >= a.H) return;
    const size_t p = (size_t)y * a.W + x;
    const float4* rec = a.aov + 4 * p;
    float4 o, r0, r1, r2;
    tp_pixel(a.beauty[p], rec[0], rec[1], rec[2], rec[3], a.prev, a.prm, o, r0, r1, r2);
    a.out[p] = o;
    a.hist[3 * p] = r0; a.hist[3 * p + 1] = r1; a.hist[3 * p + 2] = r2;
}

__global__ __launch_bounds__(kTpBX * kTpBY) void k_tp_integrate_mv(TpArgs a, const float4* motion)
{
    const int x = blockIdx.x * kTpBX + threadIdx.x, y = blockIdx.y * kTpBY + threadIdx.y;
    if (x >= a.W || y >= a.H) return;
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
    const dim3 grid((W + kTpBX - 1) / kTpBX, (H + kTpBY - 1) / kTpBY), block(kTpBX, kTpBY);
    TpArgs a{ beauty, aov, prev, prm, out, hist, W, H };
    hipLaunchKernelGGL(k_tp_integrate, grid, block, 0, s, a);
}

// the same with a motion plane: W*H float4 (gmupt_temporal_denoise_image_motion)
void launch_temporal_motion(const float4* beauty, const float4* aov, const float4* motion, int W, int H, const TpPrev& prev, const TpParams& prm,
                            float4* out, float4* hist, hipStream_t s)
{
    const dim3 grid((W + kTpBX - 1) / kTpBX, (H + kTpBY - 1) / kTpBY), block(kTpBX, kTpBY);
    TpArgs a{ beauty, aov, prev, prm, out, hist, W, H };
    hipLaunchKernelGGL(k_tp_integrate_mv, grid, block, 0, s, a, motion);
}

// ---- the host integration (gmupt_temporal_integrate_host): every pixel reads only the inputs, so the bands cannot change a bit.
// beauty / out: W*H RGBA float texels, aov: W*H 64-byte records, prev / outHist: 48-byte records, motion: W*H 16-byte records or nullptr
// (gmupt_temporal_integrate_motion_host); any alignment (copied into aligned buffers)
void temporal_host(const float* beauty, const void* aov, const void* motion, int W, int H, const void* prev, const gmupt_camera_buffer* prevCam, int px0, int py0,
                   int pW, int pH, const TpParams& prm, float* out, void* outHist, int threads)
{
    const size_t n = (size_t)W * H;
    std::vector<float4> in(n), rec(4 * n), res(n), hist(3 * n), old(prev ? 3 * (size_t)pW * pH : 0), mv(motion ? n : 0);
    if (motion) std::memcpy(mv.data(), motion, n * 16);
    std::memcpy(in.data(), beauty, n * 16);
    std::memcpy(rec.data(), aov, n * 64);
    if (prev) std::memcpy(old.data(), prev, old.size() * 16);
    TpPrev pv{};
    if (prev) { pv.rec = old.data(); pv.x0 = px0; pv.y0 = py0; pv.W = pW; pv.H = pH; pv.cam = tp_camera(*prevCam); }
    dn_bands(H, threads, [&](int y0, int y1) {
        for (size_t i = (size_t)y0 * W; i < (size_t)y1 * W; i++)
            if (motion) tp_pixel_t<true>(in[i], rec[4 * i], rec[4 * i + 1], rec[4 * i + 2], rec[4 * i + 3], mv[i], pv, prm, res[i], hist[3 * i], hist[3 * i + 1], hist[3 * i + 2]);
            else tp_pixel(in[i], rec[4 * i], rec[4 * i + 1], rec[4 * i + 2], rec[4 * i + 3], pv, prm, res[i], hist[3 * i], hist[3 * i + 1], hist[3 * i + 2]);
    });
    std::memcpy(out, res.data(), n * 16);
    std::memcpy(outHist, hist.data(), n * 48);
}

} // namespace gmupt
