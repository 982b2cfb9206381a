// The convergence monitor on the device (gmupt_converge_update; include/gmupt.h "Convergence" states the rule).  No atomics of any
// kind, no fences, no waiting inside a launch: a level is a launch, and the stream orders the levels.
//   k_cv_update   one thread per pixel, one block per run of 256: one 16-byte load of the pixel, the six state planes (three of 4-byte
//                 and three of 8-byte words, each read and written by consecutive lanes at consecutive addresses), the pixel's update
//                 and error (pt_converge.hpp), the optional 4-byte error store, then the block reduction of the pixel's summary entry;
//                 one 32-byte partial per block.  A pixel whose count did not move stores no state.
//   k_cv_reduce   the same reduction over the partials of the level below, one thread per partial, until one is left
// The order of the sum -- the block reduction, the level kernel's body and the launches of the levels -- is pt_ordered_sum.hpp.  Every
// index is checked against the entry count.  k_cv_update is bound by the 52 bytes it reads and the up to 40 it writes per pixel.
#include "pt_converge.hpp"
#include "pt_scratch.hpp"
#include "pt_launch.hpp"

namespace gmupt {

__global__ __launch_bounds__(kSumRun) void k_cv_update(const float4* __restrict__ rgba, size_t n, CvPlanes pl, CvParams prm, float* __restrict__ error,
                                                      CvPartial* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * kSumRun + threadIdx.x;
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
    sum_block_store<cv_combine>(v, out);
}

__global__ __launch_bounds__(kSumRun) void k_cv_reduce(const CvPartial* __restrict__ in, size_t n, CvPartial* __restrict__ out)
{
    sum_reduce_level<cv_zero, cv_combine>(in, n, out);
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
    p.partials = sc.take<CvPartial>(sum_level_partials(cap));
    if (out) *out = p;
    return sc.used;
}

size_t converge_state_bytes(size_t cap) { return 3 * scratch_align(cap * sizeof(uint32_t)) + 3 * scratch_align(cap * sizeof(double)); }

// enqueues the levels; returns where the one partial that is left will be
const CvPartial* launch_converge(const float4* rgba, size_t n, const CvPlanes& pl, const CvParams& prm, float* error, hipStream_t s)
{
    const size_t m = sum_runs(n);
    hipLaunchKernelGGL(k_cv_update, dim3((uint32_t)m), dim3(kSumRun), 0, s, rgba, n, pl, prm, error, pl.partials);
    return sum_launch_levels(k_cv_reduce, pl.partials, m, s);
}

} // namespace gmupt
