// The convergence monitor on the device (gmupt_converge_update; include/gmupt.h "Convergence" states the rule).  No atomics of any
// kind, no fences, no waiting inside a launch: a level is a launch, and the stream orders the levels.
//   k_cv_update   one thread per pixel, one block per run of 256: one 16-byte load of the pixel, the six state planes (three of 4-byte
//                 and three of 8-byte words, each read and written by consecutive lanes at consecutive addresses), the pixel's update
//                 and error (pt_converge.hpp), the optional 4-byte error store, then the block reduction of the pixel's summary entry;
//                 one 32-byte partial per block.  A pixel whose count did not move stores no state.
//   k_cv_reduce   the same reduction over the partials of the level below, one thread per partial, until one is left
// The block reduction is the stride halving of the rule, as in pt_treecost.hip: s = 128 and s = 64 go through LDS (the upper half
// writes, the lower half adds), s = 32 .. 1 are cross-lane moves inside wave 0 (a double moves as two dwords).  Every index is checked
// against the entry count; a thread beyond it holds the padding entry of the rule.  The kernel is bound by the 52 bytes it reads and
// the up to 40 it writes per pixel.
#include "pt_converge.hpp"
#include "pt_scratch.hpp"
#include "pt_launch.hpp"

namespace gmupt {

static_assert(kCvRun == 256, "the block reduction below is written for four waves of 64");

// lane i receives the entry of lane i + s of its wave (its own where there is none: those lanes' results are never used)
__device__ __forceinline__ CvPartial cv_shfl_down(const CvPartial& v, int s)
{
    CvPartial o;
    o.sumError = __shfl_down(v.sumError, s, 64);
    o.unsampled = (uint32_t)__shfl_down((int)v.unsampled, s, 64); o.known = (uint32_t)__shfl_down((int)v.known, s, 64);
    o.nonfinite = (uint32_t)__shfl_down((int)v.nonfinite, s, 64); o.below = (uint32_t)__shfl_down((int)v.below, s, 64);
    o.maxError = __shfl_down(v.maxError, s, 64); o.pad = 0;
    return o;
}

// x[0] of the run whose entry t this thread holds, in thread 0; the other threads return what they last held
__device__ __forceinline__ CvPartial cv_block_reduce(CvPartial v)
{
    __shared__ CvPartial sh[kCvRun / 2];
    const uint32_t t = threadIdx.x;
    if (t >= 128) sh[t - 128] = v;
    __syncthreads();
    if (t < 128) cv_combine(v, sh[t]);              // s = 128
    __syncthreads();
    if (t >= 64 && t < 128) sh[t - 64] = v;
    __syncthreads();
    if (t < 64) {
        cv_combine(v, sh[t]);                       // s = 64
        for (int s = 32; s > 0; s >>= 1) cv_combine(v, cv_shfl_down(v, s));
    }
    return v;
}

__global__ __launch_bounds__(kCvRun) void k_cv_update(const float4* __restrict__ rgba, size_t n, CvPlanes pl, CvParams prm, float* __restrict__ error,
                                                      CvPartial* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * kCvRun + threadIdx.x;
    CvPartial v = cv_zero();
    if (i < n) {
        const float4 px = rgba[i];
        CvState st = { pl.n[i], pl.k[i], pl.w[i], pl.s[i], pl.mean[i], pl.m2[i] };
        const uint32_t n0 = st.n;
        const uint32_t n1 = cv_update(st, px.x, px.y, px.z, px.w);
        if (n1 != n0) {             // a batch arrived or the pixel restarted: otherwise the state is unchanged
            pl.n[i] = st.n; pl.k[i] = st.k; pl.w[i] = st.w; pl.s[i] = st.s; pl.mean[i] = st.mean; pl.m2[i] = st.m2;
        }
        const float err = cv_error(st);
        if (error) error[i] = err;
        v = cv_pixel(st, n1, err, prm);
    }
    v = cv_block_reduce(v);
    if (threadIdx.x == 0) out[blockIdx.x] = v;
}

__global__ __launch_bounds__(kCvRun) void k_cv_reduce(const CvPartial* __restrict__ in, size_t n, CvPartial* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * kCvRun + threadIdx.x;
    CvPartial v = cv_zero();
    if (i < n) v = in[i];
    v = cv_block_reduce(v);
    if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// ---- host side (gmupt_capi_converge.hip) ----

// the parts of the allocation for `cap` pixels: the state planes first (one contiguous range, what a restart zeroes), then the partials
// of all levels, one level after the other
size_t converge_carve(void* base, size_t cap, CvPlanes* out)
{
    Scratch sc(base);
    CvPlanes p;
    p.n = sc.take<uint32_t>(cap); p.k = sc.take<uint32_t>(cap); p.w = sc.take<uint32_t>(cap);
    p.s = sc.take<double>(cap); p.mean = sc.take<double>(cap); p.m2 = sc.take<double>(cap);
    size_t partials = 0;
    for (size_t m = cv_runs(cap); ; m = cv_runs(m)) { partials += m; if (m == 1) break; }
    p.partials = sc.take<CvPartial>(partials);
    if (out) *out = p;
    return sc.used;
}

size_t converge_state_bytes(size_t cap) { return 3 * scratch_align(cap * sizeof(uint32_t)) + 3 * scratch_align(cap * sizeof(double)); }

// enqueues the levels; returns where the one partial that is left will be
const CvPartial* launch_converge(const float4* rgba, size_t n, const CvPlanes& pl, const CvParams& prm, float* error, hipStream_t s)
{
    size_t m = cv_runs(n);
    hipLaunchKernelGGL(k_cv_update, dim3((uint32_t)m), dim3(kCvRun), 0, s, rgba, n, pl, prm, error, pl.partials);
    CvPartial* level = pl.partials;
    while (m > 1) {
        const size_t next = cv_runs(m);
        hipLaunchKernelGGL(k_cv_reduce, dim3((uint32_t)next), dim3(kCvRun), 0, s, (const CvPartial*)level, m, level + m);
        level += m; m = next;
    }
    return level;
}

} // namespace gmupt
