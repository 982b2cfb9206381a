// Denoiser (gmupt_denoise_image, gmupt_render_denoised, gmupt_denoise_host; include/gmupt.h states the filter), in 2 + passes launches
//
//   k_dn_prepare    one thread per pixel: beauty texel + 64-byte AOV record -> the guide planes nl / xa / ag / z and colour buffer A
//                   (variance word 0, or -1 for an invalid pixel)
//   k_dn_variance   one thread per pixel: the initial variance from the luminance moments of the 3x3 neighbourhood, A -> B
//   k_dn_atrous     one launch per pass, one thread per pixel: the 3x3 variance Gaussian and the 25 taps at step 1 << k, ping-pong
//                   B -> A -> B ...; the last pass writes the caller's output with the input alpha bits
//
// No host synchronisation between the launches.  The per-pixel arithmetic is pt_denoise.hpp, which the host filter below runs too.
#include "pt_device.hpp"
#include "detmath.hpp"
#include "pt_denoise.hpp"
#include "pt_launch.hpp"

#include <cstring>
#include <vector>

namespace gmupt {

constexpr int kDnBX = 64, kDnBY = 4;   // a wave is a row segment of 64 pixels: every tap load of a wave is 1 KiB (512 B for ag) contiguous

struct DnPrepare { const float4* beauty; const float4* aov; DnPlanes g; float4* col; uint32_t n; };

__global__ __launch_bounds__(kBlock) void k_dn_prepare(DnPrepare a)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const float4* rec = a.aov + 4 * (size_t)i;
    a.col[i] = dn_prepare(a.beauty[i], rec[0], rec[1], rec[2], rec[3], a.g, i);
}

struct DnVariance { const float4* in; float4* out; const float4* nl; int W, H; };

__global__ __launch_bounds__(kDnBX * kDnBY) void k_dn_variance(DnVariance a)
{
    const int x = blockIdx.x * kDnBX + threadIdx.x, y = blockIdx.y * kDnBY + threadIdx.y;
    if (x >= a.W || y >= a.H) return;
    const size_t p = (size_t)y * a.W + x;
    const float4 c = a.in[p];
    a.out[p] = dn_valid(c.w) ? make_float4(c.x, c.y, c.z, dn_initial_variance(a.in, a.nl, a.W, a.H, x, y)) : c;
}

struct DnPass { const float4* in; float4* out; DnPlanes g; DnParams prm; int W, H, step; const float4* beauty; };   // beauty: the last pass only

#ifndef GMUPT_DN_WAVES
#define GMUPT_DN_WAVES 4   // waves per SIMD the register budget of k_dn_atrous must allow (4: at most 128 VGPRs)
#endif
__global__ __launch_bounds__(kDnBX * kDnBY) __attribute__((amdgpu_waves_per_eu(GMUPT_DN_WAVES))) void k_dn_atrous(DnPass a)
{
    const int x = blockIdx.x * kDnBX + threadIdx.x, y = blockIdx.y * kDnBY + threadIdx.y;
    if (x >= a.W || y >= a.H) return;
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

// the scratch of an image of n pixels (kDnScratchBytes per pixel): colour buffers A and B, then the guide planes
static DnPlanes dn_split(void* scratch, size_t n, float4*& A, float4*& B)
{
    char* b = static_cast<char*>(scratch);
    A = reinterpret_cast<float4*>(b); b += n * 16;
    B = reinterpret_cast<float4*>(b); b += n * 16;
    DnPlanes g;
    g.nl = reinterpret_cast<float4*>(b); b += n * 16;
    g.xa = reinterpret_cast<float4*>(b); b += n * 16;
    g.ag = reinterpret_cast<float2*>(b); b += n * 8;
    g.z = reinterpret_cast<float*>(b);
    return g;
}

// ---- host launcher (gmupt_capi.hip: gmupt_denoise_image).  beauty / out: W*H float4; aov: W*H records of 4 float4; W*H <= 2^28.
void launch_denoise(const float4* beauty, const float4* aov, int W, int H, const DnParams& prm, void* scratch, float4* out, hipStream_t s)
{
    const size_t n = (size_t)W * H;
    float4 *A, *B;
    const DnPlanes g = dn_split(scratch, n, A, B);
    DnPrepare pr{ beauty, aov, g, A, (uint32_t)n };
    hipLaunchKernelGGL(k_dn_prepare, dim3((uint32_t)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, pr);
    const dim3 grid((W + kDnBX - 1) / kDnBX, (H + kDnBY - 1) / kDnBY), block(kDnBX, kDnBY);
    DnVariance va{ A, B, g.nl, W, H };
    hipLaunchKernelGGL(k_dn_variance, grid, block, 0, s, va);
    for (int k = 0; k < prm.passes; k++) {
        const bool last = k == prm.passes - 1;
        DnPass pa{ (k & 1) ? A : B, last ? out : ((k & 1) ? B : A), g, prm, W, H, 1 << k, last ? beauty : nullptr };
        hipLaunchKernelGGL(k_dn_atrous, grid, block, 0, s, pa);
    }
}

// ---- the host filter (gmupt_denoise_host): the same phases over row bands of std::threads.  Every pixel of a phase reads only the
// previous phase's buffers, so neither the bands nor the thread count can change a bit of the result.
// beauty / out: W*H RGBA float texels, aov: W*H 64-byte records; any alignment (copied into aligned buffers)
void denoise_host(const float* beauty, const void* aov, int W, int H, const DnParams& prm, float* out, int threads)
{
    const size_t n = (size_t)W * H;
    std::vector<float4> in(n), rec(4 * n), A(n), B(n), nl(n), xa(n), res(n);
    std::vector<float2> ag(n);
    std::vector<float> z(n);
    std::memcpy(in.data(), beauty, n * 16);
    std::memcpy(rec.data(), aov, n * 64);
    const DnPlanes g{ nl.data(), xa.data(), ag.data(), z.data() };
    dn_bands(H, threads, [&](int y0, int y1) {
        for (size_t i = (size_t)y0 * W; i < (size_t)y1 * W; i++) A[i] = dn_prepare(in[i], rec[4 * i], rec[4 * i + 1], rec[4 * i + 2], rec[4 * i + 3], g, i);
    });
    dn_bands(H, threads, [&](int y0, int y1) {
        for (int y = y0; y < y1; y++) for (int x = 0; x < W; x++) {
            const size_t p = (size_t)y * W + x;
            const float4 c = A[p];
            B[p] = dn_valid(c.w) ? make_float4(c.x, c.y, c.z, dn_initial_variance(A.data(), nl.data(), W, H, x, y)) : c;
        }
    });
    for (int k = 0; k < prm.passes; k++) {
        const bool last = k == prm.passes - 1;
        const float4* src = (k & 1) ? A.data() : B.data();
        float4* dst = last ? res.data() : ((k & 1) ? B.data() : A.data());
        dn_bands(H, threads, [&](int y0, int y1) {
            for (int y = y0; y < y1; y++) for (int x = 0; x < W; x++) {
                const size_t p = (size_t)y * W + x;
                const float4 c = src[p];
                if (!dn_valid(c.w)) { dst[p] = last ? in[p] : c; continue; }
                float4 r = dn_atrous(src, g, W, H, x, y, 1 << k, prm);
                if (last) r.w = in[p].w;
                dst[p] = r;
            }
        });
    }
    std::memcpy(out, res.data(), n * 16);
}

} // namespace gmupt
