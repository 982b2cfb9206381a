// The arithmetic of the treelet optimiser (include/gmupt.h "Tree optimisation" states the rule), shared by gmupt_tree_optimize_host
// (pt_treeopt.cpp) and the k_to_* kernels (pt_treeopt.hip): how a treelet grows, the half area of a subset of its leaves, the scan over
// the partitions of a subset, and the order in which a rewrite reuses node ids.  One copy, so that host and device run the same binary64
// statements; nothing is contracted (build.py).  The working copy is the 48-byte node record itself with links to any working id, plus a
// parent link and a cost per node.
#pragma once
#include "pt_lbvh.hpp"                // kMaxTreeDepth, and with it pt_refit.hpp
#include "pt_treecost.hpp"
#include <string>

namespace gmupt {

constexpr uint32_t kToLeaves = 7;              // treelet leaves
constexpr uint32_t kToSubsets = 1u << kToLeaves;
constexpr uint32_t kToMaxPasses = 8;           // params.passes is in 1 .. kToMaxPasses
constexpr uint32_t kToFlagBadLink = 1u, kToFlagNotTree = 2u, kToFlagDeep = 4u;

// "Half area" of the tree cost for a box
GM_HD double to_half_area(const float* mn, const float* mx)
{
    const double ex = tc_extent(mn[0], mx[0]), ey = tc_extent(mn[1], mx[1]), ez = tc_extent(mn[2], mx[2]);
    return (ex * ey + ey * ez) + ez * ex;
}
GM_HD double to_leaf_cost(const gmupt_bvh_node& n) { return to_half_area(n.min, n.max) * (double)((uint32_t)n.right - (uint32_t)n.left); }
GM_HD double to_inner_cost(double a, double cl, double cr) { return a * 2.0 + (cl + cr); }

GM_HD uint32_t to_lowest_slot(uint32_t s) { uint32_t j = 0; while (!((s >> j) & 1u)) j++; return j; }

// The treelet of one inner node: its leaves by slot (working id, kind, box, half area) and the ids of the inner nodes between them and
// the treelet's root, ascending.
struct ToTreelet {
    uint32_t k, numInner;
    int32_t slot[kToLeaves];
    int32_t inner[kToLeaves - 2];
    uint32_t isInner[kToLeaves];
    double area[kToLeaves];
    float mn[kToLeaves][3], mx[kToLeaves][3];
};

GM_HD void to_load_slot(ToTreelet& t, uint32_t j, const gmupt_bvh_node* nodes, int32_t id)
{
    const gmupt_bvh_node& n = nodes[id];
    t.slot[j] = id; t.isInner[j] = n.isLeaf == 0 ? 1u : 0u;
    for (int c = 0; c < 3; c++) { t.mn[j][c] = n.min[c]; t.mx[j][c] = n.max[c]; }
    t.area[j] = to_half_area(n.min, n.max);
}

// the growth step: the slot to replace by its two children, -1 when no treelet leaf is an inner node.  Slots are scanned in ascending
// order; a later slot wins with a larger half area, or with an equal one and a lower working id.
GM_HD int to_pick(const ToTreelet& t)
{
    int best = -1;
    for (uint32_t j = 0; j < t.k; j++) {
        if (!t.isInner[j]) continue;
        if (best < 0 || t.area[j] > t.area[best] || (t.area[j] == t.area[best] && t.slot[j] < t.slot[best])) best = (int)j;
    }
    return best;
}

// the treelet of inner node X of a working copy of N nodes.  false: a child link outside [0, N) was met (it is not followed).
GM_HD bool to_form(const gmupt_bvh_node* nodes, uint32_t N, int32_t X, ToTreelet& t)
{
    t.k = 0; t.numInner = 0;
    int32_t l = nodes[X].left, r = nodes[X].right;
    if ((uint32_t)l >= N || (uint32_t)r >= N) return false;
    to_load_slot(t, 0, nodes, l); to_load_slot(t, 1, nodes, r);
    t.k = 2;
    while (t.k < kToLeaves) {
        const int j = to_pick(t);
        if (j < 0) break;
        const int32_t id = t.slot[j];
        l = nodes[id].left; r = nodes[id].right;
        if ((uint32_t)l >= N || (uint32_t)r >= N) return false;
        uint32_t at = t.numInner++;                                   // kept ascending
        while (at > 0 && t.inner[at - 1] > id) { t.inner[at] = t.inner[at - 1]; at--; }
        t.inner[at] = id;
        to_load_slot(t, (uint32_t)j, nodes, l); to_load_slot(t, t.k, nodes, r);
        t.k++;
    }
    return true;
}

// a[s]: the half area of the box of the slots in s -- the lowest slot's box, the others folded in by ascending slot
GM_HD double to_subset_area(const ToTreelet& t, uint32_t s)
{
    RfBox b;
    bool first = true;
    for (uint32_t j = 0; j < t.k; j++) {
        if (!((s >> j) & 1u)) continue;
        if (first) { for (int c = 0; c < 3; c++) { b.mn[c] = t.mn[j][c]; b.mx[c] = t.mx[j][c]; } first = false; }
        else for (int c = 0; c < 3; c++) { b.mn[c] = rf_lo(b.mn[c], t.mn[j][c]); b.mx[c] = rf_hi(b.mx[c], t.mx[j][c]); }
    }
    return to_half_area(b.mn, b.mx);
}

// min over p of c[p] + c[s \ p] for a subset s of two slots or more: p = the proper subsets of s that hold its lowest slot, in
// increasing numeric value; a later one replaces the best only when strictly smaller
GM_HD double to_partition_scan(const double* c, uint32_t s, uint32_t* bestP)
{
    const uint32_t low = s & (0u - s), rest = s ^ low;
    double best = 0.0;
    uint32_t bp = 0;
    for (uint32_t q = 0; q != rest; q = ((q | ~rest) + 1u) & rest) {   // the subsets of `rest` in increasing value, `rest` itself left out
        const uint32_t p = low | q;
        const double v = c[p] + c[s ^ p];
        if (bp == 0 || v < best) { best = v; bp = p; }
    }
    *bestP = bp;
    return best;
}

// the whole programme of one treelet, serially (the host reference; the kernel spreads the subsets of one size over lanes)
GM_HD void to_programme(const ToTreelet& t, const double* leafCost, double* a, double* c, uint8_t* part)
{
    const uint32_t all = (1u << t.k) - 1u;
    for (uint32_t s = 1; s <= all; s++) {                              // every proper subset of s is smaller than s
        a[s] = to_subset_area(t, s);
        if (!(s & (s - 1u))) { c[s] = leafCost[to_lowest_slot(s)]; part[s] = 0; continue; }
        uint32_t p;
        const double v = to_partition_scan(c, s, &p);
        c[s] = a[s] * 2.0 + v; part[s] = (uint8_t)p;
    }
}

// The rewrite of X's treelet by the partitions in part[]: X keeps its id, the other inner ids are reused, ascending, in pre-order of the
// new topology (left = the p side, right = s \ p); then, children first, every inner node of the treelet gets the union of its
// children's boxes (the refit rule), zero padding and the cost c[its subset].
GM_HD void to_rewrite(gmupt_bvh_node* nodes, int32_t* parent, double* cost, int32_t X, const ToTreelet& t, const double* c, const uint8_t* part)
{
    const uint32_t all = (1u << t.k) - 1u;
    uint32_t stS[kToLeaves + 1]; int32_t stParent[kToLeaves + 1]; uint32_t stSide[kToLeaves + 1];
    int32_t ordId[kToLeaves - 1]; uint32_t ordS[kToLeaves - 1];
    uint32_t sp = 0, cnt = 0, next = 0;
    stS[0] = all; stParent[0] = -1; stSide[0] = 0; sp = 1;
    while (sp) {
        sp--;
        const uint32_t s = stS[sp], side = stSide[sp];
        const int32_t par = stParent[sp];
        int32_t id;
        if (s & (s - 1u)) {
            id = s == all ? X : t.inner[next++];
            ordId[cnt] = id; ordS[cnt] = s; cnt++;
            const uint32_t p = part[s];
            stS[sp] = s ^ p; stParent[sp] = id; stSide[sp] = 1; sp++;
            stS[sp] = p; stParent[sp] = id; stSide[sp] = 0; sp++;
        } else {
            id = t.slot[to_lowest_slot(s)];
        }
        if (par >= 0) {
            if (side) nodes[par].right = id; else nodes[par].left = id;
            parent[id] = par;
        }
    }
    for (uint32_t i = cnt; i-- > 0;) {
        gmupt_bvh_node& n = nodes[ordId[i]];
        const gmupt_bvh_node& l = nodes[n.left];
        const gmupt_bvh_node& r = nodes[n.right];
        const RfBox b = rf_union(l.min, l.max, r.min, r.max);
        for (int k = 0; k < 3; k++) { n.min[k] = b.mn[k]; n.max[k] = b.mx[k]; }
        n.isLeaf = 0; n.pad0 = 0.0f; n.pad1 = 0.0f; n.pad2 = 0.0f;
        cost[ordId[i]] = c[ordS[i]];
    }
}

// what X is before its treelet is looked at: the union of its children's boxes, zero padding; returns its half area
GM_HD double to_refresh(gmupt_bvh_node* nodes, int32_t X)
{
    gmupt_bvh_node& n = nodes[X];
    const gmupt_bvh_node& l = nodes[n.left];
    const gmupt_bvh_node& r = nodes[n.right];
    const RfBox b = rf_union(l.min, l.max, r.min, r.max);
    for (int k = 0; k < 3; k++) { n.min[k] = b.mn[k]; n.max[k] = b.mx[k]; }
    n.pad0 = 0.0f; n.pad1 = 0.0f; n.pad2 = 0.0f;
    return to_half_area(n.min, n.max);
}

// device words of a run: [0] flags, [3] treelets rewritten, [8 + j] the depth the j-th depth launch found (j = 0: the input, j = passes:
// the output), [20..23] cost before and after as two doubles; behind them where each depth starts in the sorted ids (pt_levels.hpp)
constexpr uint32_t kToWordRewritten = 3, kToWordDepth = 8, kToWordCost = 20;

// what a run reports besides the nodes
struct ToResult { uint32_t numNodes, depthBefore, depthAfter, rewritten; double costBefore, costAfter; };

// ---- host reference (pt_treeopt.cpp).  Returns "" and GMUPT_OK in *status, or the message and the status; writes nothing on an error.
std::string tree_optimize_host(const gmupt_bvh_node* nodes, uint32_t n, uint32_t passes, gmupt_bvh_node* nodesOut, ToResult& res, int* status);

} // namespace gmupt
