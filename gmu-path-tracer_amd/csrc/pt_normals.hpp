// The arithmetic of the smooth vertex normals (include/gmupt.h states the rule), shared by gmupt_vertex_normals_host (pt_normals.cpp) and
// the k_nm_* kernels (pt_normals.hip): the face vector of a triangle and the step from a vertex's sum to its normal.  One copy, so that
// host and device run the same binary32 statements; nothing is contracted, division and square root are correctly rounded (build.py).
// The ORDER of a vertex's sum -- ascending corner number -- is the other half of the rule; both callers walk a corner list in that order.
#pragma once
#include "pt_device.hpp"
#include "detmath.hpp"

namespace gmupt {

constexpr uint32_t kNmMaxTris = 1u << 30;      // 3 * num_tris corner numbers fit a uint32
constexpr uint32_t kNmFlagBadIndex = 1u;

// rule 1: the area-weighted face vector, e1 x e2
GM_HD void nm_face(const float* p0, const float* p1, const float* p2, float* f)
{
    const float e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
    const float e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
    f[0] = e1y * e2z - e1z * e2y;
    f[1] = e1z * e2x - e1x * e2z;
    f[2] = e1x * e2y - e1y * e2x;
}

// rule 3: the normal of a vertex sum; (0, 1, 0) unless the length is positive and finite (a NaN length fails both comparisons)
GM_HD void nm_finish(const float* s, float* n)
{
    const float l = dsqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
    if (l > 0.0f && l < u2f(0x7F800000u)) {
        const float inv = 1.0f / l;
        n[0] = s[0] * inv; n[1] = s[1] * inv; n[2] = s[2] * inv;
    } else {
        n[0] = 0.0f; n[1] = 1.0f; n[2] = 0.0f;
    }
}

// Byte offsets of the parts of a gmupt_normals handle's device memory (one allocation, pt_normals.hip: normals_layout places them).
// Kept for every update: words, indices, corners, offsets, faces (40 bytes per triangle + 4 per vertex).  Used by create only and
// handed back after it: the sort's keys (in and out), its input values and its temporary storage, placed last.
struct NmLayout { size_t words, indices, corners, offsets, faces, kept, keysIn, keys, valsIn, sortTemp, total; };

// what the kernels of a handle work on
struct NmArgs {
    const int32_t* indices; uint32_t numTris;      // the handle's own copy of the index list
    uint32_t numVerts;
    uint32_t* corners;                             // 3 * numTris corner numbers sorted by (vertex, corner)
    uint32_t* offsets;                             // numVerts + 1: the corners of vertex v are corners[offsets[v] .. offsets[v + 1])
    float4* faces;                                 // numTris face vectors (w = 0)
    uint32_t* words;                               // [0] kNmFlag*, [1] the largest valence
    uint32_t* keysIn; uint32_t* keys; uint32_t* valsIn;   // create only
    const float* verts; gmupt_tri_props* props;    // update only: the buffers the renderer is bound to
};

// ---- host reference (pt_normals.cpp) on validated input: normalsOut holds 3 floats per vertex
void normals_host(const float* verts, uint32_t numVerts, const int32_t* indices, uint32_t numTris, float* normalsOut, int threads);

} // namespace gmupt
