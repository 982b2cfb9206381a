// gmupt_tree_optimize_host: the rule of include/gmupt.h ("Tree optimisation") on a host array, the reference of the device path
// (pt_treeopt.hip).  The arithmetic is pt_treeopt.hpp, shared with the kernels.  A pass visits the inner nodes by the depths they had at
// its start, deepest first -- the schedule of the device's level launches; the programme of a treelet runs serially over the subsets in
// increasing value.
#include "pt_treeopt.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

namespace gmupt {

namespace {

// depth of every node of the working copy by its links (a parent is not always below its children's ids any more); returns the largest
uint32_t to_depths(const std::vector<gmupt_bvh_node>& w, std::vector<uint32_t>& depth, std::vector<int32_t>& order)
{
    order.clear();
    order.push_back(0);
    depth[0] = 0;
    uint32_t top = 0;
    for (size_t at = 0; at < order.size(); at++) {                    // breadth first: `order` is by ascending depth
        const int32_t i = order[at];
        top = std::max(top, depth[(size_t)i]);
        if (w[(size_t)i].isLeaf) continue;
        for (const int32_t c : { w[(size_t)i].left, w[(size_t)i].right }) { depth[(size_t)c] = depth[(size_t)i] + 1; order.push_back(c); }
    }
    return top;
}

} // namespace

std::string tree_optimize_host(const gmupt_bvh_node* nodes, uint32_t n, uint32_t passes, gmupt_bvh_node* nodesOut, ToResult& res, int* status)
{
    *status = GMUPT_ERR_INVALID_ARGUMENT;
    const size_t N = n;
    // the input is a tree over all N records: children above their parent, every record but the root the child of exactly one node
    std::vector<int32_t> parent(N, -1);
    std::vector<uint32_t> refs(N, 0);
    for (size_t i = 0; i < N; i++) {
        const gmupt_bvh_node& x = nodes[i];
        if (x.isLeaf) continue;
        if (x.left <= (int32_t)i || x.right <= (int32_t)i || (size_t)x.left >= N || (size_t)x.right >= N)
            return "inner node " + std::to_string(i) + " has children (" + std::to_string(x.left) + ", " + std::to_string(x.right) + ") outside (" + std::to_string(i) + ", " + std::to_string(N) + ")";
        refs[(size_t)x.left]++; refs[(size_t)x.right]++;
        parent[(size_t)x.left] = (int32_t)i; parent[(size_t)x.right] = (int32_t)i;
    }
    for (size_t i = 0; i < N; i++)
        if (refs[i] != (i ? 1u : 0u)) return "record " + std::to_string(i) + " is the child of " + std::to_string(refs[i]) + " nodes: not a tree over all records";

    std::vector<gmupt_bvh_node> w(nodes, nodes + N);
    std::vector<uint32_t> depth(N, 0);
    std::vector<int32_t> order;
    order.reserve(N);
    const uint32_t depthBefore = to_depths(w, depth, order);
    if (depthBefore > kMaxTreeDepth) {
        *status = GMUPT_ERR_UNSUPPORTED;
        return "the tree is " + std::to_string(depthBefore) + " levels deep, the traversal stacks hold " + std::to_string(kMaxTreeDepth);
    }

    std::vector<double> cost(N, 0.0), cost0(N, 0.0);
    for (size_t i = 0; i < N; i++) if (w[i].isLeaf) cost[i] = cost0[i] = to_leaf_cost(w[i]);
    uint32_t rewritten = 0, depthNow = depthBefore;
    ToTreelet t;
    double a[kToSubsets], c[kToSubsets], leafCost[kToLeaves];
    uint8_t part[kToSubsets];
    for (uint32_t pass = 0; pass < passes; pass++) {
        for (size_t at = order.size(); at-- > 0;) {                     // by the depths at the start of the pass, deepest first
            const int32_t X = order[at];
            if (w[(size_t)X].isLeaf) continue;
            const int32_t l0 = w[(size_t)X].left, r0 = w[(size_t)X].right;
            if (!to_form(w.data(), n, X, t)) return "a child link left the array";      // (cannot happen: the links were checked)
            const double aX = to_refresh(w.data(), X);
            const double cX = to_inner_cost(aX, cost[(size_t)l0], cost[(size_t)r0]);
            if (pass == 0) cost0[(size_t)X] = to_inner_cost(aX, cost0[(size_t)l0], cost0[(size_t)r0]);
            cost[(size_t)X] = cX;
            if (t.k < 3) continue;
            for (uint32_t j = 0; j < t.k; j++) leafCost[j] = cost[(size_t)t.slot[j]];
            to_programme(t, leafCost, a, c, part);
            if (c[(1u << t.k) - 1u] < cX) { to_rewrite(w.data(), parent.data(), cost.data(), X, t, c, part); rewritten++; }
        }
        depthNow = to_depths(w, depth, order);
        if (depthNow > kMaxTreeDepth) {
            *status = GMUPT_ERR_UNSUPPORTED;
            return "the tree is " + std::to_string(depthNow) + " levels deep after pass " + std::to_string(pass + 1) + ", the traversal stacks hold " + std::to_string(kMaxTreeDepth);
        }
    }

    // numbering by (depth, working id): `order` is by depth, and stable sorting each depth by id finishes it
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return depth[(size_t)x] != depth[(size_t)y] ? depth[(size_t)x] < depth[(size_t)y] : x < y; });
    std::vector<int32_t> number(N);
    for (size_t p = 0; p < N; p++) number[(size_t)order[p]] = (int32_t)p;
    for (size_t p = 0; p < N; p++) {
        gmupt_bvh_node o = w[(size_t)order[p]];
        if (!o.isLeaf) { o.left = number[(size_t)o.left]; o.right = number[(size_t)o.right]; }
        nodesOut[p] = o;
    }
    res.numNodes = n; res.depthBefore = depthBefore; res.depthAfter = depthNow; res.rewritten = rewritten;
    res.costBefore = passes ? cost0[0] : cost[0]; res.costAfter = cost[0];
    *status = GMUPT_OK;
    return "";
}

} // namespace gmupt
