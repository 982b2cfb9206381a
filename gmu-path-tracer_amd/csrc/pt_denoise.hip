// Denoiser (gmupt_denoise_image, gmupt_render_denoised; include/gmupt.h states the filter), in 2 + passes launches
//
//   k_dn_prepare    one thread per pixel: beauty texel + 64-byte AOV record -> the guide planes nw / xa / ag / z and colour buffer A
//                   (variance word 0, or -1 for an invalid pixel)
//   k_dn_variance   one thread per pixel: the initial variance from the luminance moments of the 3x3 neighbourhood, A -> B
//   k_dn_atrous     one launch per pass, one thread per pixel: the 3x3 variance Gaussian and the 25 taps at step 1 << k, ping-pong
//                   B -> A -> B ...; the last pass writes the caller's output with the input alpha bits
//
// No host synchronisation between the launches.  The per-pixel arithmetic is pt_denoise.hpp, which the host filter (pt_denoise.cpp) runs too.
#include "pt_kernel_util.hpp"
#include "pt_denoise.hpp"
#include "pt_launch.hpp"

namespace gmupt {

struct DnPrepare { const float4* beauty; const float4* aov; GdPlanes g; float4* col; uint32_t n; };

__global__ __launch_bounds__(kBlock) void k_dn_prepare(DnPrepare a)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const float4* rec = a.aov + 4 * (size_t)i;
    a.col[i] = dn_prepare(a.beauty[i], rec[0], rec[1], rec[2], rec[3], a.g, i);
}

struct DnVariance { const float4* in; float4* out; const float4* nw; int W, H; };

__global__ __launch_bounds__(kTileX * kTileY) void k_dn_variance(DnVariance a)
{
    int x, y;
    if (!tile_pixel(a.W, a.H, x, y)) return;
    const size_t p = (size_t)y * a.W + x;
    const float4 c = a.in[p];
    a.out[p] = dn_valid(c.w) ? make_float4(c.x, c.y, c.z, dn_initial_variance(a.in, a.nw, a.W, a.H, x, y)) : c;
}

struct DnPass { const float4* in; float4* out; GdPlanes g; DnParams prm; int W, H, step; const float4* beauty; };   // beauty: the last pass only

#ifndef GMUPT_DN_WAVES
#define GMUPT_DN_WAVES 4   // waves per SIMD the register budget of k_dn_atrous must allow (4: at most 128 VGPRs)
#endif
__global__ __launch_bounds__(kTileX * kTileY) __attribute__((amdgpu_waves_per_eu(GMUPT_DN_WAVES))) void k_dn_atrous(DnPass a)
{
    int x, y;
    if (!tile_pixel(a.W, a.H, x, y)) return;
    const size_t p = (size_t)y * a.W + x;
    const float4 c = a.in[p];
    if (!dn_valid(c.w)) {                                                     // invalid: the input texel, bit for bit
        if (a.beauty) a.out[p] = a.beauty[p]; else a.out[p] = c;              // (not a ?: of two addresses: that would put c on the stack)
        return;
    }
    float4 r = dn_atrous(a.in, a.g, a.W, a.H, x, y, a.step, a.prm);
    if (a.beauty) r.w = a.beauty[p].w;                                        // alpha: the sample-count bits of the input
    a.out[p] = r;
}

// ---- host launcher (gmupt_capi.hip: gmupt_denoise_image).  beauty / out: W*H float4; aov: W*H records of 4 float4; W*H <= 2^28.
void launch_denoise(const float4* beauty, const float4* aov, int W, int H, const DnParams& prm, void* scratch, float4* out, hipStream_t s)
{
    const size_t n = (size_t)W * H;
    float4 *A, *B;
    const GdPlanes g = gd_carve(scratch, 0, n, A, B);
    DnPrepare pr{ beauty, aov, g, A, (uint32_t)n };
    hipLaunchKernelGGL(k_dn_prepare, dim3((uint32_t)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, pr);
    const TileDims t = tile_dims(W, H);
    DnVariance va{ A, B, g.nw, W, H };
    hipLaunchKernelGGL(k_dn_variance, t.grid, t.block, 0, s, va);
    for (int k = 0; k < prm.passes; k++) {
        const bool last = k == prm.passes - 1;
        DnPass pa{ (k & 1) ? A : B, last ? out : ((k & 1) ? B : A), g, prm, W, H, 1 << k, last ? beauty : nullptr };
        hipLaunchKernelGGL(k_dn_atrous, t.grid, t.block, 0, s, pa);
    }
}

} // namespace gmupt
