// gmupt_lbvh_build_host: the LBVH rule of include/gmupt.h on host arrays, the reference of the device build (pt_lbvh.hip).  The arithmetic
// is pt_lbvh.hpp, shared with the kernels.  The hierarchy is built top-down and breadth-first, which IS the numbering of rule 7: a level is
// visited in order of `first`, so the children of a level are created in order of `first` too.  The device reaches the same tree bottom-up
// (Karras's search per inner node) and the same numbering by a sort.
#include "pt_lbvh.hpp"

#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

namespace gmupt {

std::string lbvh_build_host(const float* verts, uint32_t numVerts, const int32_t* indices, uint32_t numTris, const uint32_t* vertexMaterial,
                            uint32_t maxLeaf, gmupt_bvh_node* nodesOut, gmupt_triangle* trisOut, int32_t* refOut, LbResult& res, int* status)
{
    *status = GMUPT_ERR_INVALID_ARGUMENT;
    const size_t n = numTris;
    // rule 9 first: nothing is written before every input has been seen
    for (size_t i = 0; i < 3 * n; i++) {
        if ((uint32_t)indices[i] >= numVerts) return "triangle " + std::to_string(i / 3) + " references vertex " + std::to_string(indices[i]) + " of " + std::to_string(numVerts);
        const float* p = verts + 3 * (size_t)indices[i];
        if (!(lb_finite(p[0]) && lb_finite(p[1]) && lb_finite(p[2]))) return "vertex " + std::to_string(indices[i]) + " (used by triangle " + std::to_string(i / 3) + ") is not finite";
    }

    // rules 1-2: centres and their bounds
    std::vector<float> centre(3 * n);
    float cmin[3], cmax[3], ext[3];
    for (size_t i = 0; i < n; i++) {
        const int32_t* t = indices + 3 * i;
        float* c = &centre[3 * i];
        lb_centre(verts + 3 * (size_t)t[0], verts + 3 * (size_t)t[1], verts + 3 * (size_t)t[2], c);
        for (int k = 0; k < 3; k++) {
            if (i == 0) cmin[k] = cmax[k] = c[k];
            cmin[k] = rf_lo(cmin[k], c[k]); cmax[k] = rf_hi(cmax[k], c[k]);
        }
    }
    for (int k = 0; k < 3; k++) ext[k] = cmax[k] - cmin[k];

    // rules 3-4: keys, sorted by (key, i)
    std::vector<uint64_t> key(n), keys(n);
    for (size_t i = 0; i < n; i++) key[i] = lb_key(&centre[3 * i], cmin, ext);
    std::vector<uint32_t> src(n);
    std::iota(src.begin(), src.end(), 0u);
    std::stable_sort(src.begin(), src.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    for (size_t p = 0; p < n; p++) keys[p] = key[src[p]];

    // rules 5-7: ranges in breadth-first order
    struct Range { int64_t first, last; uint32_t depth; int32_t left; };
    std::vector<Range> tree;
    tree.reserve(2 * n);
    tree.push_back({ 0, (int64_t)n - 1, 0u, -1 });
    uint32_t depth = 0, leaves = 0;
    for (size_t i = 0; i < tree.size(); i++) {
        const Range r = tree[i];
        depth = std::max(depth, r.depth);
        if ((uint64_t)(r.last - r.first + 1) <= maxLeaf) { leaves++; continue; }
        const int64_t s = lb_split(keys.data(), r.first, r.last);
        tree[i].left = (int32_t)tree.size();
        tree.push_back({ r.first, s, r.depth + 1, -1 });
        tree.push_back({ s + 1, r.last, r.depth + 1, -1 });
    }
    if (depth > kMaxTreeDepth) {
        *status = GMUPT_ERR_UNSUPPORTED;
        return "the tree is " + std::to_string(depth) + " levels deep, the traversal stacks hold " + std::to_string(kMaxTreeDepth);
    }

    // rule 8: records
    for (size_t p = 0; p < n; p++) {
        trisOut[p] = lb_record(indices + 3 * (size_t)src[p], vertexMaterial);
        if (refOut) refOut[p] = (int32_t)src[p];
    }
    const size_t N = tree.size();
    for (size_t i = N; i-- > 0;) {
        gmupt_bvh_node o;
        std::memset(&o, 0, sizeof(o));
        RfBox b;
        if (tree[i].left < 0) {
            o.left = (int32_t)tree[i].first; o.right = (int32_t)tree[i].last + 1; o.isLeaf = 1;
            b = rf_leaf_box(trisOut, verts, o.left, o.right);
        } else {
            o.left = tree[i].left; o.right = o.left + 1; o.isLeaf = 0;
            const gmupt_bvh_node& l = nodesOut[(size_t)o.left];
            const gmupt_bvh_node& r = nodesOut[(size_t)o.right];
            b = rf_union(l.min, l.max, r.min, r.max);
        }
        for (int k = 0; k < 3; k++) { o.min[k] = b.mn[k]; o.max[k] = b.mx[k]; }
        nodesOut[i] = o;
    }
    res.numNodes = (uint32_t)N; res.numLeaves = leaves; res.depth = depth;
    for (int k = 0; k < 3; k++) { res.rootMin[k] = nodesOut[0].min[k]; res.rootMax[k] = nodesOut[0].max[k]; }
    *status = GMUPT_OK;
    return "";
}

} // namespace gmupt
