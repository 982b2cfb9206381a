// Refit's arithmetic (include/gmupt.h states it), shared by the k_rf_* kernels (pt_refit.hip) and refit_host (pt_refit.cpp): one copy of the
// box rule, the triangle record and the flat-child test, so that host and device run the same binary32 statements.  Only comparisons,
// selections and two subtractions per component: no rounding that a compiler flag could change, apart from contraction (off, build.py).
#pragma once
#include "pt_device.hpp"
#include "detmath.hpp"

namespace gmupt {

constexpr uint32_t kRfNone = 0xFFFFFFFFu;   // an entry of a refit map that names no reference node (filler Node64, empty WNode slot)

GM_HD float rf_lo(float a, float b) { return b < a ? b : a; }
GM_HD float rf_hi(float a, float b) { return b > a ? b : a; }

struct RfBox { float mn[3], mx[3]; };

GM_HD void rf_fold(RfBox& b, const float* v)
{
    for (int k = 0; k < 3; k++) { b.mn[k] = rf_lo(b.mn[k], v[k]); b.mx[k] = rf_hi(b.mx[k], v[k]); }
}

// leaf [left, right), right > left: the box of the whole triangles of its references, folded in reference order, vertex order
GM_HD RfBox rf_leaf_box(const gmupt_triangle* tris, const float* verts, int32_t left, int32_t right)
{
    RfBox b;
    const float* v0 = verts + 3 * (size_t)tris[left].v[0];
    for (int k = 0; k < 3; k++) b.mn[k] = b.mx[k] = v0[k];
    for (int32_t i = left; i < right; i++)
        for (int j = (i == left ? 1 : 0); j < 3; j++) rf_fold(b, verts + 3 * (size_t)tris[i].v[j]);
    return b;
}

// inner node: the left child's box, then the right child's
GM_HD RfBox rf_union(const float* lmn, const float* lmx, const float* rmn, const float* rmx)
{
    RfBox b;
    for (int k = 0; k < 3; k++) { b.mn[k] = rf_lo(lmn[k], rmn[k]); b.mx[k] = rf_hi(lmx[k], rmx[k]); }
    return b;
}

// the nine floats of a traversal triangle record: v0, e1 = v1 - v0, e2 = v2 - v0 (extensionRayCast.hlsl:40-41)
GM_HD void rf_tri9(const gmupt_triangle& t, const float* verts, float* c)
{
    const float* v0 = verts + 3 * (size_t)t.v[0]; const float* v1 = verts + 3 * (size_t)t.v[1]; const float* v2 = verts + 3 * (size_t)t.v[2];
    for (int k = 0; k < 3; k++) { c[k] = v0[k]; c[3 + k] = v1[k] - v0[k]; c[6 + k] = v2[k] - v0[k]; }
}

// false when child box c is flat on an axis on which parent box p is not, in the plane of one of p's faces: such a parent must keep
// its own slot in the 4-wide collapse (pt_travtables.cpp: collapse, which calls this; k_rf_wide repeats it on the refitted boxes)
GM_HD bool rf_child_ok(const float* pmn, const float* pmx, const float* cmn, const float* cmx)
{
    for (int k = 0; k < 3; k++)
        if (cmn[k] == cmx[k] && pmn[k] != pmx[k] && (cmn[k] == pmn[k] || cmx[k] == pmx[k])) return false;
    return true;
}

// what a refit needs from bind besides the tables themselves (the refit maps of pt_travtables.hpp, uploaded by the first refit)
struct RfArgs {
    DNode* nodes; const gmupt_triangle* tris; const float* verts;
    uint32_t numNodes, numTris, numVerts;
    const uint32_t* levelNodes;      // inner nodes by height, lowest first
    Tri48* ttris; TriPair* pairs; const uint32_t* pairRef; uint32_t numPairs;
    Node64* tnodes; const uint32_t* nodeMap; uint32_t numPacked;       // packed index -> reference node
    WNode* wnodes; const uint32_t* wideMap; uint32_t wideCount;        // 4 * wide node + slot -> reference node
    const uint32_t* opened; uint32_t numOpened;                        // nodes whose slot the collapse replaced by their children
    uint32_t* flags;                 // [0] kRfFlag* of the vertex check, [1] != 0: an opened node has a flat child in a face plane
};
constexpr uint32_t kRfFlagNonFinite = 1u, kRfFlagBadIndex = 2u;

void refit_host(gmupt_bvh_node* nodes, size_t N, const gmupt_triangle* tris, const float* verts, int threads);   // pt_refit.cpp

} // namespace gmupt
