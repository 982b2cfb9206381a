// The tree cost on the device (gmupt_renderer_tree_cost; include/gmupt.h "Tree cost" states the rule): a reduction over the 48-byte node
// records of a GMUPT_BUFFER_BVH_NODES buffer in the fixed order of the rule.  No float atomics, no fences, no waiting inside a launch: a
// level is a launch, and the stream orders the levels.
//   k_tc_nodes    one thread per record, one block per run of 256: three 16-byte loads per thread (the lanes of a wave cover 3 KiB of
//                 consecutive bytes between them), the record's term (pt_treecost.hpp), then the block reduction; one 48-byte partial
//                 per block
//   k_tc_reduce   the same reduction over the partials of the level below, one thread per partial, until one is left
// The block reduction is the stride halving of the rule: s = 128 and s = 64 go through LDS (the upper half writes, the lower half adds),
// s = 32 .. 1 are cross-lane moves inside wave 0 (a double moves as two dwords).  Every index is checked against the entry count; a
// thread beyond it holds the padding entry of the rule.  The kernel is bound by the 48 bytes it reads per record.
#include "pt_treecost.hpp"
#include "pt_launch.hpp"

namespace gmupt {

static_assert(kTcRun == 256, "the block reduction below is written for four waves of 64");

// lane i receives the entry of lane i + s of its wave (its own where there is none: those lanes' results are never used)
__device__ __forceinline__ TcPartial tc_shfl_down(const TcPartial& v, int s)
{
    TcPartial o;
    o.sumInner = __shfl_down(v.sumInner, s, 64); o.sumLeaf = __shfl_down(v.sumLeaf, s, 64);
    o.numRefs = (uint64_t)__shfl_down((unsigned long long)v.numRefs, s, 64);
    o.numInner = (uint32_t)__shfl_down((int)v.numInner, s, 64); o.numLeaves = (uint32_t)__shfl_down((int)v.numLeaves, s, 64);
    o.maxLeafRefs = (uint32_t)__shfl_down((int)v.maxLeafRefs, s, 64);
    o.pad = 0; o.rootHalfArea = 0.0;
    return o;
}

// x[0] of the run whose entry t this thread holds, in thread 0; the other threads return what they last held
__device__ __forceinline__ TcPartial tc_block_reduce(TcPartial v)
{
    __shared__ TcPartial sh[kTcRun / 2];
    const uint32_t t = threadIdx.x;
    if (t >= 128) sh[t - 128] = v;
    __syncthreads();
    if (t < 128) tc_combine(v, sh[t]);              // s = 128
    __syncthreads();
    if (t >= 64 && t < 128) sh[t - 64] = v;
    __syncthreads();
    if (t < 64) {
        tc_combine(v, sh[t]);                       // s = 64
        for (int s = 32; s > 0; s >>= 1) tc_combine(v, tc_shfl_down(v, s));
    }
    return v;
}

__global__ __launch_bounds__(kTcRun) void k_tc_nodes(const gmupt_bvh_node* __restrict__ nodes, uint32_t n, TcPartial* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * kTcRun + threadIdx.x;
    TcPartial v = tc_zero();
    if (i < n) {
        const uint4* rec = reinterpret_cast<const uint4*>(nodes + i);
        const uint4 a = rec[0], b = rec[1], c = rec[2];
        const float mn[3] = { u2f(a.x), u2f(a.y), u2f(a.z) }, mx[3] = { u2f(b.x), u2f(b.y), u2f(b.z) };
        v = tc_node(mn, mx, (int32_t)c.x, (int32_t)c.y, (int32_t)c.z);
    }
    v = tc_block_reduce(v);
    if (threadIdx.x == 0) out[blockIdx.x] = v;
}

__global__ __launch_bounds__(kTcRun) void k_tc_reduce(const TcPartial* __restrict__ in, uint32_t n, TcPartial* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * kTcRun + threadIdx.x;
    TcPartial v = tc_zero();
    if (i < n) v = in[i];
    v = tc_block_reduce(v);
    if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// ---- host side (gmupt_capi_treecost.hip) ----

// partials of all levels, one after the other; the last one is the result
size_t tree_cost_scratch_partials(uint32_t n)
{
    size_t total = 0;
    for (size_t m = tc_runs(n); ; m = tc_runs(m)) { total += m; if (m == 1) break; }
    return total;
}

// enqueues the levels; returns where the one partial that is left will be
const TcPartial* launch_tree_cost(const gmupt_bvh_node* nodes, uint32_t n, TcPartial* scratch, hipStream_t s)
{
    size_t m = tc_runs(n);
    hipLaunchKernelGGL(k_tc_nodes, dim3((uint32_t)m), dim3(kTcRun), 0, s, nodes, n, scratch);
    TcPartial* level = scratch;
    while (m > 1) {
        const size_t next = tc_runs(m);
        hipLaunchKernelGGL(k_tc_reduce, dim3((uint32_t)next), dim3(kTcRun), 0, s, (const TcPartial*)level, (uint32_t)m, level + m);
        level += m; m = next;
    }
    return level;
}

} // namespace gmupt
