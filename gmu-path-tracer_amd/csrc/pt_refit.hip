// Refit (gmupt_renderer_refit; include/gmupt.h states it): the boxes of the bound tree and every traversal table
// of the renderer recomputed in place for moved vertices, topology kept.  Streaming kernels, one record (or 16 bytes of one) per thread:
//
//   k_rf_finite  one thread per triangle record: its three vertices are inside the vertex array and finite, else a flag bit
//   k_rf_leaves  one thread per reference node: a non-empty leaf gets the box of the whole triangles of its references
//   k_rf_level   one thread per inner node of one height (the children of a node are lower: no atomics, no waiting inside a launch)
//   k_rf_tris    one thread per reference: Tri48 = v0, e1, e2; the flag and first-equal-reference words kept
//   k_rf_pairs   one thread per TriPair: its two Tri48 records (just written, near-sequential) interleaved; flag and count words kept
//   k_rf_nodes   one thread per Node64: both child boxes through the map packed index -> reference node; descriptors kept
//   k_rf_wide    eight threads per WNode, 16 bytes each: the six plane rows through the map slot -> reference node (NaN slots kept), the
//                link and aux rows not written; the first numOpened threads also run the flat-child test of one opened node
//
// All arithmetic is pt_refit.hpp, which the host refit (pt_refit.cpp) runs too.  Indices are size_t: a table may pass 2 GiB.
#include "pt_refit.hpp"
#include "pt_launch.hpp"
#include "pt_scratch.hpp"

#include <algorithm>
#include <vector>

namespace gmupt {

constexpr int kRfBlock = 256;

GM_HD bool rf_finite(float x) { return (f2u(x) & 0x7F800000u) != 0x7F800000u; }

__global__ __launch_bounds__(kRfBlock) void k_rf_finite(RfArgs a)
{
    const size_t i = (size_t)blockIdx.x * kRfBlock + threadIdx.x;
    if (i >= a.numTris) return;
    const int4 t = *reinterpret_cast<const int4*>(a.tris + i);
    const int32_t v[3] = { t.x, t.y, t.z };
    uint32_t bad = 0;
    for (int k = 0; k < 3; k++) {
        if ((uint32_t)v[k] >= a.numVerts) { bad |= kRfFlagBadIndex; continue; }
        const float* p = a.verts + 3 * (size_t)v[k];
        if (!(rf_finite(p[0]) && rf_finite(p[1]) && rf_finite(p[2]))) bad |= kRfFlagNonFinite;
    }
    if (bad) atomicOr(a.flags, bad);
}

__device__ __forceinline__ void rf_store_box(DNode* n, const RfBox& b)
{
    // the pad words of the two rows are the caller's: 12-byte stores
    *reinterpret_cast<float3*>(&n->mn) = make_float3(b.mn[0], b.mn[1], b.mn[2]);
    *reinterpret_cast<float3*>(&n->mx) = make_float3(b.mx[0], b.mx[1], b.mx[2]);
}

__global__ __launch_bounds__(kRfBlock) void k_rf_leaves(RfArgs a)
{
    const size_t i = (size_t)blockIdx.x * kRfBlock + threadIdx.x;
    if (i >= a.numNodes) return;
    const int4 link = a.nodes[i].link;
    if (!link.z || link.x < 0 || link.y <= link.x || (uint32_t)link.y > a.numTris) return;   // (bind validated the ranges; an empty leaf keeps its box)
    rf_store_box(a.nodes + i, rf_leaf_box(a.tris, a.verts, link.x, link.y));
}

__global__ __launch_bounds__(kRfBlock) void k_rf_level(RfArgs a, uint32_t first, uint32_t count)
{
    const uint32_t j = blockIdx.x * kRfBlock + threadIdx.x;
    if (j >= count) return;
    const size_t i = a.levelNodes[first + j];
    const int4 link = a.nodes[i].link;
    if ((uint32_t)link.x >= a.numNodes || (uint32_t)link.y >= a.numNodes) return;
    const float4 lmn = a.nodes[link.x].mn, lmx = a.nodes[link.x].mx, rmn = a.nodes[link.y].mn, rmx = a.nodes[link.y].mx;
    rf_store_box(a.nodes + i, rf_union(&lmn.x, &lmx.x, &rmn.x, &rmx.x));
}

__global__ __launch_bounds__(kRfBlock) void k_rf_tris(RfArgs a)
{
    const size_t i = (size_t)blockIdx.x * kRfBlock + threadIdx.x;
    if (i >= a.numTris) return;
    const int4 t = *reinterpret_cast<const int4*>(a.tris + i);
    gmupt_triangle tr; tr.v[0] = t.x; tr.v[1] = t.y; tr.v[2] = t.z; tr.materialID = 0;
    float c[9];
    rf_tri9(tr, a.verts, c);
    float4* o = reinterpret_cast<float4*>(a.ttris + i);
    const float4 keep = o[2];
    o[0] = make_float4(c[0], c[1], c[2], c[3]);
    o[1] = make_float4(c[4], c[5], c[6], c[7]);
    o[2] = make_float4(c[8], keep.y, keep.z, keep.w);
}

__global__ __launch_bounds__(kRfBlock) void k_rf_pairs(RfArgs a)
{
    const size_t p = (size_t)blockIdx.x * kRfBlock + threadIdx.x;
    if (p >= a.numPairs) return;
    const uint2 ref = *reinterpret_cast<const uint2*>(a.pairRef + 2 * p);
    float4* o = reinterpret_cast<float4*>(a.pairs + p);
    const float4 keep = o[4];
    float c[2][9];
    const uint32_t rr[2] = { ref.x, ref.y };
    for (int s = 0; s < 2; s++) {
        if (rr[s] < a.numTris) {
            const float4* t = reinterpret_cast<const float4*>(a.ttris + rr[s]);
            const float4 r0 = t[0], r1 = t[1], r2 = t[2];
            c[s][0] = r0.x; c[s][1] = r0.y; c[s][2] = r0.z; c[s][3] = r0.w; c[s][4] = r1.x; c[s][5] = r1.y; c[s][6] = r1.z; c[s][7] = r1.w; c[s][8] = r2.x;
        } else {
            for (int k = 0; k < 9; k++) c[s][k] = 0.0f;    // no reference in this slot: the all-zero triangle of bind
        }
    }
    o[0] = make_float4(c[0][0], c[1][0], c[0][1], c[1][1]);
    o[1] = make_float4(c[0][2], c[1][2], c[0][3], c[1][3]);
    o[2] = make_float4(c[0][4], c[1][4], c[0][5], c[1][5]);
    o[3] = make_float4(c[0][6], c[1][6], c[0][7], c[1][7]);
    o[4] = make_float4(c[0][8], c[1][8], keep.z, keep.w);
}

__global__ __launch_bounds__(kRfBlock) void k_rf_nodes(RfArgs a)
{
    const size_t q = (size_t)blockIdx.x * kRfBlock + threadIdx.x;
    if (q >= a.numPacked) return;
    const uint32_t i = a.nodeMap[q];
    if (i >= a.numNodes) return;                                 // filler record
    const int4 link = a.nodes[i].link;
    if ((uint32_t)link.x >= a.numNodes || (uint32_t)link.y >= a.numNodes) return;
    const float4 lmn = a.nodes[link.x].mn, lmx = a.nodes[link.x].mx, rmn = a.nodes[link.y].mn, rmx = a.nodes[link.y].mx;
    float4* o = reinterpret_cast<float4*>(a.tnodes + q);
    const float4 d = o[3];
    o[0] = make_float4(lmn.x, lmn.y, lmn.z, lmx.x);
    o[1] = make_float4(lmx.y, lmx.z, rmn.x, rmn.y);
    o[2] = make_float4(rmn.z, rmx.x, rmx.y, rmx.z);
    o[3] = d;
}

__global__ __launch_bounds__(kRfBlock) void k_rf_wide(RfArgs a)
{
    const size_t t = (size_t)blockIdx.x * kRfBlock + threadIdx.x;
    const size_t g = t >> 3;
    const uint32_t j = (uint32_t)t & 7u;
    if (g < a.wideCount && j < 6) {
        const uint4 m4 = *reinterpret_cast<const uint4*>(a.wideMap + 4 * g);
        const uint32_t m[4] = { m4.x, m4.y, m4.z, m4.w };
        float4* row = reinterpret_cast<float4*>(a.wnodes + g) + j;
        const float4 old = *row;
        float v[4] = { old.x, old.y, old.z, old.w };
        const uint32_t word = j < 3 ? j : 4 + (5 - j);            // rows: min x, y, z, max z, y, x; a DNode is (min.xyz, pad, max.xyz, pad, ..)
        for (int k = 0; k < 4; k++)
            if (m[k] < a.numNodes) v[k] = reinterpret_cast<const float*>(a.nodes + m[k])[word];
        *row = make_float4(v[0], v[1], v[2], v[3]);
    }
    if (t < a.numOpened) {
        const uint32_t i = a.opened[t];
        if (i < a.numNodes) {
            const DNode pn = a.nodes[i];
            if ((uint32_t)pn.link.x < a.numNodes && (uint32_t)pn.link.y < a.numNodes) {
                const float4 lmn = a.nodes[pn.link.x].mn, lmx = a.nodes[pn.link.x].mx, rmn = a.nodes[pn.link.y].mn, rmx = a.nodes[pn.link.y].mx;
                if (!(rf_child_ok(&pn.mn.x, &pn.mx.x, &lmn.x, &lmx.x) && rf_child_ok(&pn.mn.x, &pn.mx.x, &rmn.x, &rmx.x))) atomicOr(a.flags + 1, 1u);
            }
        }
    }
}

// ---- host launchers (gmupt_capi.hip: gmupt_renderer_refit) ----
void launch_refit_check(const RfArgs& a, hipStream_t s)
{
    if (a.numTris) hipLaunchKernelGGL(k_rf_finite, dim3(grid_for(a.numTris, kRfBlock)), dim3(kRfBlock), 0, s, a);
}

// node boxes of the caller's buffer; levelOff[h] .. levelOff[h + 1] are the nodes of height h + 1 in a.levelNodes.  Returns the launches of
// the inner part.
uint32_t launch_refit_boxes(const RfArgs& a, const std::vector<uint32_t>& levelOff, hipStream_t s)
{
    hipLaunchKernelGGL(k_rf_leaves, dim3(grid_for(a.numNodes, kRfBlock)), dim3(kRfBlock), 0, s, a);
    uint32_t launches = 0;
    for (size_t h = 0; h + 1 < levelOff.size(); h++) {
        const uint32_t first = levelOff[h], count = levelOff[h + 1] - first;
        if (!count) continue;
        hipLaunchKernelGGL(k_rf_level, dim3(grid_for(count, kRfBlock)), dim3(kRfBlock), 0, s, a, first, count);
        launches++;
    }
    return launches;
}

// the traversal tables from the refitted boxes; a.wnodes == nullptr: no wide copy, the pair and wide parts are skipped
void launch_refit_tables(const RfArgs& a, hipStream_t s)
{
    if (a.numTris) hipLaunchKernelGGL(k_rf_tris, dim3(grid_for(a.numTris, kRfBlock)), dim3(kRfBlock), 0, s, a);
    if (a.wnodes && a.numPairs) hipLaunchKernelGGL(k_rf_pairs, dim3(grid_for(a.numPairs, kRfBlock)), dim3(kRfBlock), 0, s, a);
    if (a.numPacked) hipLaunchKernelGGL(k_rf_nodes, dim3(grid_for(a.numPacked, kRfBlock)), dim3(kRfBlock), 0, s, a);
    if (a.wnodes && a.wideCount) hipLaunchKernelGGL(k_rf_wide, dim3(grid_for(std::max((size_t)a.wideCount * 8, (size_t)a.numOpened), kRfBlock)), dim3(kRfBlock), 0, s, a);
}

} // namespace gmupt
