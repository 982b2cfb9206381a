// gmupt_tree_cost_host: the rule of include/gmupt.h ("Tree cost") on a host array, the reference of the device path (pt_treecost.hip).
// The arithmetic is pt_treecost.hpp, shared with the kernels; the order of the sum is pt_ordered_sum.hpp.  Threads only share out the runs
// of the first level, so the order inside every sum -- and with it every bit of the result -- does not depend on the thread count.
#include "pt_treecost.hpp"

namespace gmupt {

TcPartial tree_cost_host(const gmupt_bvh_node* nodes, uint32_t n, int threads)
{
    const auto entry = [nodes](size_t k) { return tc_node(nodes[k].min, nodes[k].max, nodes[k].left, nodes[k].right, nodes[k].isLeaf); };
    return ordered_sum_host<tc_zero, tc_combine>(n, threads, entry);
}

} // namespace gmupt
