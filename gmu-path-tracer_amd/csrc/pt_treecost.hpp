// The arithmetic of the tree cost (include/gmupt.h "Tree cost" states the rule), shared by gmupt_tree_cost_host (pt_treecost.cpp) and the
// k_tc_* kernels (pt_treecost.hip): what one node record contributes, how two partial results combine, and the step from the totals to the
// SAH.  One copy, so that host and device run the same binary64 statements; nothing is contracted (build.py).  The ORDER in which the
// terms are combined -- runs of 256, stride halving, level by level -- is the other half of the rule: pt_ordered_sum.hpp, which both callers
// hand tc_zero and tc_combine to.
#pragma once
#include "pt_device.hpp"
#include "detmath.hpp"
#include "pt_ordered_sum.hpp"

namespace gmupt {

// What a node, a run, or the whole buffer amounts to.  rootHalfArea is the half area of the FIRST record the partial covers, so the one
// partial that is left at the end carries that of record 0.  48 bytes: the records of the device scratch.
struct TcPartial {
    double sumInner, sumLeaf;
    uint64_t numRefs;
    uint32_t numInner, numLeaves, maxLeafRefs, pad;
    double rootHalfArea;
};
static_assert(sizeof(TcPartial) == 48, "TcPartial layout");

// "Extent" of the rule: a NaN difference fails the comparison and gives 0
GM_HD double tc_extent(float mn, float mx) { const double d = (double)mx - (double)mn; return d > 0.0 ? d : 0.0; }

// "Half area", "Weight" and "Term" for one record, given as its box and its three link words
GM_HD TcPartial tc_node(const float* mn, const float* mx, int32_t left, int32_t right, int32_t isLeaf)
{
    const double ex = tc_extent(mn[0], mx[0]), ey = tc_extent(mn[1], mx[1]), ez = tc_extent(mn[2], mx[2]);
    const double a = (ex * ey + ey * ez) + ez * ex;
    TcPartial p{};
    p.rootHalfArea = a;
    if (isLeaf == 0) {
        p.sumInner = a * 2.0; p.sumLeaf = 0.0; p.numInner = 1;
    } else {
        const uint32_t refs = (uint32_t)right - (uint32_t)left;
        p.sumInner = 0.0; p.sumLeaf = a * (double)refs; p.numLeaves = 1; p.numRefs = refs; p.maxLeafRefs = refs;
    }
    return p;
}

// the padding entry of a run: +0.0 in both sums, nothing counted
GM_HD TcPartial tc_zero() { return TcPartial{}; }

// x[i] += x[i + s] of the rule; the integer fields are order-free, the first record's half area stays that of x[i]
GM_HD void tc_combine(TcPartial& x, const TcPartial& y)
{
    x.sumInner = x.sumInner + y.sumInner; x.sumLeaf = x.sumLeaf + y.sumLeaf;
    x.numRefs += y.numRefs; x.numInner += y.numInner; x.numLeaves += y.numLeaves;
    x.maxLeafRefs = y.maxLeafRefs > x.maxLeafRefs ? y.maxLeafRefs : x.maxLeafRefs;
}

// "SAH" of the rule, and the public fields (ms stays as it is)
inline void tc_fill_info(const TcPartial& t, gmupt_tree_cost_info* info)
{
    info->sum_inner = t.sumInner; info->sum_leaf = t.sumLeaf;
    info->num_inner = t.numInner; info->num_leaves = t.numLeaves; info->num_refs = t.numRefs; info->max_leaf_refs = t.maxLeafRefs; info->pad = 0;
    info->root_half_area = t.rootHalfArea;
    info->sah = t.rootHalfArea > 0.0 ? (t.sumInner + t.sumLeaf) / t.rootHalfArea : 0.0;
}

// ---- host reference (pt_treecost.cpp): the rule over n >= 1 records; no device, no allocation the caller sees
TcPartial tree_cost_host(const gmupt_bvh_node* nodes, uint32_t n, int threads);

} // namespace gmupt
