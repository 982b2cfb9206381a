// Guided infill (gmupt_infill_image, gmupt_temporal_preview_image, gmupt_render_preview; include/gmupt.h states the rule), in
// 1 + passes launches behind one 16-byte memset of the counters
//
//   k_if_prepare    one thread per pixel: beauty texel + 64-byte AOV record -> the guide planes nw / xa / ag / z and colour buffer A with
//                   the state word (no surface / open hole / source); counts sources and holes
//   k_if_pass       one launch per pass, one thread per pixel.  A pixel that is no open hole copies its 16-byte texel through -- a wave
//                   without an open hole does nothing else; an open hole visits the 25 taps at step 1 << k.  Ping-pong A -> B -> A ...;
//                   the last pass writes the caller's output and counts the holes left open
//
// No host synchronisation between the launches.  The counters are integer atomics, one per wave and word: their sums do not depend on
// the order.  The per-pixel arithmetic is pt_infill.hpp, which infill_host (pt_infill.cpp) runs too.
#include "pt_kernel_util.hpp"
#include "pt_infill.hpp"
#include "pt_launch.hpp"

namespace gmupt {

// adds the number of lanes of this wave with `on` to *word: one atomic by the first such lane (threadIdx.x is the lane: kTileX)
__device__ __forceinline__ void if_count(bool on, uint32_t* word)
{
    const unsigned long long m = __ballot(on);
    if (on && (m & ((1ull << threadIdx.x) - 1ull)) == 0ull) atomicAdd(word, (uint32_t)__popcll(m));
}

struct IfPrepare { const float4* beauty; const float4* aov; GdPlanes g; float4* col; IfCounters* counts; int W, H; };

__global__ __launch_bounds__(kTileX * kTileY) void k_if_prepare(IfPrepare a)
{
    int x, y;
    uint32_t st = kIfNot;
    if (tile_pixel(a.W, a.H, x, y)) {
        const size_t i = (size_t)y * a.W + x;
        const float4* rec = a.aov + 4 * i;
        const float4 c = if_prepare(a.beauty[i], rec[0], rec[1], rec[2], rec[3], a.g, i);
        a.col[i] = c;
        st = if_state(c);
    }
    if_count(st == kIfSource, &a.counts->sources);
    if_count(st == kIfOpen, &a.counts->holes);
}

struct IfPass { const float4* in; float4* out; GdPlanes g; IfParams prm; int W, H, step; const float4* beauty; IfCounters* counts; };   // beauty: the last pass only

constexpr int kIfWaves = 4;   // waves per SIMD the register budget of k_if_pass must allow (at most 128 VGPRs), as k_dn_atrous: a hole holds
                              // the 56 bytes of five taps in flight, and the code object needs 112 VGPRs for that without scratch
__global__ __launch_bounds__(kTileX * kTileY) __attribute__((amdgpu_waves_per_eu(kIfWaves))) void k_if_pass(IfPass a)
{
    int x, y;
    bool filled = false, left = false;
    if (tile_pixel(a.W, a.H, x, y)) {
        const size_t p = (size_t)y * a.W + x;
        float4 c = a.in[p];
        if (if_state(c) == kIfOpen) {
            c = if_fill(a.in, a.g, a.W, a.H, x, y, a.step, a.prm);
            filled = if_state(c) == kIfFilled;
            left = !filled;
        }
        if (a.beauty) a.out[p] = if_output(c, a.beauty[p]); else a.out[p] = c;
    }
    if_count(filled, &a.counts->filled);
    if (a.beauty) if_count(left, &a.counts->openLeft);
}

// the scratch of an image of n pixels: kIfCounterBytes for the counters, then kGdScratchBytes per pixel
size_t infill_scratch_bytes(size_t n) { return kIfCounterBytes + n * kGdScratchBytes; }

// ---- host launcher.  beauty / out: W*H float4; aov: W*H records of 4 float4; W*H <= 2^28.  *countsOut (if asked for): where the
// call's counters stand (device memory at the head of the scratch) once the stream has run the launches.
hipError_t launch_infill(const float4* beauty, const float4* aov, int W, int H, const IfParams& prm, void* scratch, float4* out, hipStream_t s,
                         const IfCounters** countsOut)
{
    const size_t n = (size_t)W * H;
    IfCounters* counts = static_cast<IfCounters*>(scratch);
    float4 *A, *B;
    const GdPlanes g = gd_carve(scratch, kIfCounterBytes, n, A, B);
    if (countsOut) *countsOut = counts;
    const hipError_t e = hipMemsetAsync(counts, 0, sizeof(IfCounters), s);
    if (e != hipSuccess) return e;
    const TileDims t = tile_dims(W, H);
    IfPrepare pr{ beauty, aov, g, A, counts, W, H };
    hipLaunchKernelGGL(k_if_prepare, t.grid, t.block, 0, s, pr);
    for (int k = 0; k < prm.passes; k++) {
        const bool last = k == prm.passes - 1;
        IfPass pa{ (k & 1) ? B : A, last ? out : ((k & 1) ? A : B), g, prm, W, H, 1 << k, last ? beauty : nullptr, counts };
        hipLaunchKernelGGL(k_if_pass, t.grid, t.block, 0, s, pa);
    }
    return hipGetLastError();
}

} // namespace gmupt
