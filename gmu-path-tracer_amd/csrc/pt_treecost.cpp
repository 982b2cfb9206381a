// gmupt_tree_cost_host: the rule of include/gmupt.h ("Tree cost") on a host array, the reference of the device path (pt_treecost.hip).
// The arithmetic is pt_treecost.hpp, shared with the kernels.  A run of 256 entries is reduced by one thread, with the strides of the
// rule; threads only share out the runs of the first level, so the order inside every sum -- and with it every bit of the result -- does
// not depend on the thread count.  The levels above hold 1/256 of the entries each and run on the calling thread.
#include "pt_treecost.hpp"
#include "pt_bands.hpp"

#include <algorithm>
#include <vector>

namespace gmupt {

// the stride halving of one run: x holds kTcRun entries, the padding included; the result is x[0]
static TcPartial tc_reduce_run(TcPartial* x)
{
    for (uint32_t s = kTcRun / 2; s > 0; s >>= 1)
        for (uint32_t i = 0; i < s; i++) tc_combine(x[i], x[i + s]);
    return x[0];
}

TcPartial tree_cost_host(const gmupt_bvh_node* nodes, uint32_t n, int threads)
{
    const size_t N = n;
    std::vector<TcPartial> level(tc_runs(N));
    host_bands((int)level.size(), threads, [&](int r0, int r1) {       // at most 2^24 runs
        TcPartial x[kTcRun];
        for (size_t run = (size_t)r0; run < (size_t)r1; run++) {
            for (uint32_t i = 0; i < kTcRun; i++) {
                const size_t k = run * kTcRun + i;
                x[i] = k < N ? tc_node(nodes[k].min, nodes[k].max, nodes[k].left, nodes[k].right, nodes[k].isLeaf) : tc_zero();
            }
            level[run] = tc_reduce_run(x);
        }
    });
    while (level.size() > 1) {
        std::vector<TcPartial> next(tc_runs(level.size()));
        TcPartial x[kTcRun];
        for (size_t run = 0; run < next.size(); run++) {
            for (uint32_t i = 0; i < kTcRun; i++) {
                const size_t k = run * kTcRun + i;
                x[i] = k < level.size() ? level[k] : tc_zero();
            }
            next[run] = tc_reduce_run(x);
        }
        level.swap(next);
    }
    return level[0];
}

} // namespace gmupt
