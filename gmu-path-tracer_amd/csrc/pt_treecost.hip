// The tree cost on the device (gmupt_renderer_tree_cost; include/gmupt.h "Tree cost" states the rule): a reduction over the 48-byte node
// records of a GMUPT_BUFFER_BVH_NODES buffer in the fixed order of the rule, which pt_ordered_sum.hpp writes (the block reduction, the
// level kernel's body and the launches of the levels).  No float atomics, no fences, no waiting inside a launch.
//   k_tc_nodes    one thread per record, one block per run of 256: three 16-byte loads per thread (the lanes of a wave cover 3 KiB of
//                 consecutive bytes between them), the record's term (pt_treecost.hpp), then the block reduction; one 48-byte partial
//                 per block.  The kernel is bound by the 48 bytes it reads per record.
//   k_tc_reduce   the same reduction over the partials of the level below, one thread per partial, until one is left
#include "pt_treecost.hpp"
#include "pt_launch.hpp"

namespace gmupt {

__global__ __launch_bounds__(kSumRun) void k_tc_nodes(const gmupt_bvh_node* __restrict__ nodes, uint32_t n, TcPartial* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * kSumRun + threadIdx.x;
    TcPartial v = tc_zero();
    if (i < n) {
        const uint4* rec = reinterpret_cast<const uint4*>(nodes + i);
        const uint4 a = rec[0], b = rec[1], c = rec[2];
        const float mn[3] = { u2f(a.x), u2f(a.y), u2f(a.z) }, mx[3] = { u2f(b.x), u2f(b.y), u2f(b.z) };
        v = tc_node(mn, mx, (int32_t)c.x, (int32_t)c.y, (int32_t)c.z);
    }
    sum_block_store<tc_combine>(v, out);
}

__global__ __launch_bounds__(kSumRun) void k_tc_reduce(const TcPartial* __restrict__ in, uint32_t n, TcPartial* __restrict__ out)
{
    sum_reduce_level<tc_zero, tc_combine>(in, n, out);
}

// ---- host side (gmupt_capi_treecost.hip) ----

// partials of all levels, one after the other; the last one is the result
size_t tree_cost_scratch_partials(uint32_t n) { return sum_level_partials(n); }

// enqueues the levels; returns where the one partial that is left will be
const TcPartial* launch_tree_cost(const gmupt_bvh_node* nodes, uint32_t n, TcPartial* scratch, hipStream_t s)
{
    const size_t m = sum_runs(n);
    hipLaunchKernelGGL(k_tc_nodes, dim3((uint32_t)m), dim3(kSumRun), 0, s, nodes, n, scratch);
    return sum_launch_levels(k_tc_reduce, scratch, m, s);
}

} // namespace gmupt
