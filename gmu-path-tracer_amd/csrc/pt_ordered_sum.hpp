// The ORDER of the summaries (include/gmupt.h "Tree cost" states it, "Convergence" refers to it), the one place that writes it: the n
// entries are cut into runs of 256; a run is reduced by stride halving, x[i] += x[i + s] for s = 128, 64 .. 1 and every i < s, entries
// beyond the count being the padding entry; the x[0] of the runs are the entries of the level above, level by level until one partial
// is left.  The tree cost (pt_treecost.*) and the convergence monitor (pt_converge.*) supply their partial type with its padding entry
// and its combination as two template arguments, the functions Zero() and Combine(x, y) for x += y (tc_zero / tc_combine, cv_zero /
// cv_combine), which are called directly and inlined; nothing here assumes that Combine commutes or associates.  Adaptive sampling
// (pt_adaptive.*) shares the run length and the counts only: its sums are integers.
//   host     sum_reduce_run (a run), sum_level_up (a level -> the level above), ordered_sum_host (the whole rule over entry(k))
//   device   sum_block_reduce (a run held one entry per thread), sum_block_store / sum_reduce_level (the bodies of a first-level
//            and of a k_*_reduce kernel), sum_launch_levels (the launches above the first level: a level is a launch, the stream
//            orders the levels)
// The block reduction takes s = 128 and s = 64 through LDS (the upper half writes, the lower half adds); s = 32 .. 1 are cross-lane
// moves inside wave 0, a partial moving dword by dword.  Every index is checked against the entry count; a thread beyond it holds the
// padding entry.
#pragma once
#include "pt_device.hpp"
#include "detmath.hpp"
#include "pt_bands.hpp"

#include <type_traits>
#include <vector>

namespace gmupt {

constexpr uint32_t kSumRun = 256;              // entries per run of the rule == threads per block

// how many partials the level above `n` entries has
inline size_t sum_runs(size_t n) { return (n + kSumRun - 1) / kSumRun; }

// the partials of all levels above `n` entries, one level after the other: what the device scratch holds; the last one is the result
inline size_t sum_level_partials(size_t n)
{
    size_t total = 0;
    for (size_t m = sum_runs(n); ; m = sum_runs(m)) { total += m; if (m == 1) break; }
    return total;
}

// ---- host

// the stride halving of one run: x holds kSumRun entries, the padding included; the result is x[0] (static: not a symbol of the library)
template <auto Combine, class P> static P sum_reduce_run(P* x)
{
    for (uint32_t s = kSumRun / 2; s > 0; s >>= 1)
        for (uint32_t i = 0; i < s; i++) Combine(x[i], x[i + s]);
    return x[0];
}

// the level above the n entries entry(0 .. n - 1).  Threads only share out the runs (host_bands), so no bit of the result depends on
// their number; with threads = 1 entry(k) is called on the calling thread, once per k, in ascending k.
template <auto Zero, auto Combine, class E> auto sum_level_up(size_t n, int threads, const E& entry)
{
    using P = decltype(Zero());
    std::vector<P> up(sum_runs(n));
    host_bands((int)up.size(), threads, [&](int r0, int r1) {          // at most 2^24 runs
        P x[kSumRun];
        for (size_t run = (size_t)r0; run < (size_t)r1; run++) {
            for (uint32_t i = 0; i < kSumRun; i++) {
                const size_t k = run * kSumRun + i;
                x[i] = k < n ? entry(k) : Zero();
            }
            up[run] = sum_reduce_run<Combine>(x);
        }
    });
    return up;
}

// the rule over n >= 1 entries; `threads` serve the first level, the levels above hold 1/256 of the entries each and run on the
// calling thread
template <auto Zero, auto Combine, class E> auto ordered_sum_host(size_t n, int threads, const E& entry)
{
    auto level = sum_level_up<Zero, Combine>(n, threads, entry);
    while (level.size() > 1) {
        auto up = sum_level_up<Zero, Combine>(level.size(), 1, [&](size_t k) { return level[k]; });
        level.swap(up);
    }
    return level[0];
}

// ---- device

static_assert(kSumRun == 256, "the block reduction below is written for four waves of 64");

// lane i receives the entry of lane i + s of its wave (its own where there is none: those lanes' results are never used).  A field
// that Combine never reads from its right operand costs nothing: its moves are dead code.
template <class P> __device__ __forceinline__ P sum_shfl_down(const P& v, int s)
{
    static_assert(std::is_trivially_copyable<P>::value && sizeof(P) % 4 == 0, "a partial moves as dwords");
    uint32_t w[sizeof(P) / 4];
    __builtin_memcpy(w, &v, sizeof(P));
    for (uint32_t& x : w) x = (uint32_t)__shfl_down((int)x, s, 64);
    P o;
    __builtin_memcpy(&o, w, sizeof(P));
    return o;
}

// x[0] of the run whose entry t this thread holds, in thread 0; the other threads return what they last held
template <auto Combine, class P> __device__ __forceinline__ P sum_block_reduce(P v)
{
    __shared__ P sh[kSumRun / 2];
    const uint32_t t = threadIdx.x;
    if (t >= 128) sh[t - 128] = v;
    __syncthreads();
    if (t < 128) Combine(v, sh[t]);                 // s = 128
    __syncthreads();
    if (t >= 64 && t < 128) sh[t - 64] = v;
    __syncthreads();
    if (t < 64) {
        Combine(v, sh[t]);                          // s = 64
        for (int s = 32; s > 0; s >>= 1) Combine(v, sum_shfl_down(v, s));
    }
    return v;
}

// the end of a first-level kernel: the block's run, entry threadIdx.x in v, becomes partial blockIdx.x of the level above
template <auto Combine, class P> __device__ __forceinline__ void sum_block_store(P v, P* __restrict__ out)
{
    v = sum_block_reduce<Combine>(v);
    if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// the body of a reduce kernel: one thread per partial of the level below
template <auto Zero, auto Combine, class P, class N>
__device__ __forceinline__ void sum_reduce_level(const P* __restrict__ in, N n, P* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * kSumRun + threadIdx.x;
    P v = Zero();
    if (i < n) v = in[i];
    sum_block_store<Combine>(v, out);
}

// enqueues the levels above the first, whose m partials the caller's kernel writes to `level`; returns where the one partial that is
// left will be
template <class P, class N> const P* sum_launch_levels(void (*reduce)(const P*, N, P*), P* level, size_t m, hipStream_t s)
{
    while (m > 1) {
        const size_t next = sum_runs(m);
        hipLaunchKernelGGL(reduce, dim3((uint32_t)next), dim3(kSumRun), 0, s, (const P*)level, (N)m, level + m);
        level += m; m = next;
    }
    return level;
}

} // namespace gmupt
