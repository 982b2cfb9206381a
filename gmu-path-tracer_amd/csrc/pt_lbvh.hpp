// The LBVH builder's arithmetic (include/gmupt.h states the rule), shared by gmupt_lbvh_build_host (pt_lbvh.cpp) and the k_lb_* kernels
// (pt_lbvh.hip): triangle box and centre, quantisation, Morton key, delta and the split of a position range.  One copy, so that host and
// device run the same binary32 statements; the division is correctly rounded and nothing is contracted (build.py).
#pragma once
#include "pt_refit.hpp"
#include <string>

namespace gmupt {

constexpr uint32_t kLbMaxLeaf = 64;            // params.max_leaf_size is in 1 .. kLbMaxLeaf
constexpr uint32_t kMaxTreeDepth = 64;         // the traversal stacks hold 64 entries: a deeper tree is GMUPT_ERR_UNSUPPORTED (builder and optimiser)
constexpr uint32_t kLbMaxTris = 1u << 30;      // 2 * num_tris - 1 node ids fit an int32
constexpr uint32_t kLbGrid = 2097152u;         // 2^21 cells per axis, 63-bit keys
constexpr uint32_t kLbFlagNonFinite = 1u, kLbFlagBadIndex = 2u;

// what launch_lbvh (pt_lbvh.hip) leaves in the builder's scratch for the caller: the device words and the staged outputs
struct LbStaging { const void* words; const void* nodes; const void* tris; const void* ref; };

GM_HD bool lb_finite(float x) { return (f2u(x) & 0x7F800000u) != 0x7F800000u; }

// rule 1: the box of the whole triangle (v0, then v1, v2 folded in with lo / hi) and its centre
GM_HD void lb_centre(const float* v0, const float* v1, const float* v2, float* c)
{
    RfBox b;
    for (int k = 0; k < 3; k++) b.mn[k] = b.mx[k] = v0[k];
    rf_fold(b, v1);
    rf_fold(b, v2);
    for (int k = 0; k < 3; k++) c[k] = (b.mn[k] + b.mx[k]) * 0.5f;
}

// rule 3.  x is in [0, 2^21] for finite centres; a centre that overflowed makes it NaN or inf, which takes the last cell (the
// conversion of such a value is not defined, so it is never reached)
GM_HD uint32_t lb_quantise(float c, float cmin, float ext)
{
    if (!(ext > 0.0f)) return 0u;
    const float x = ((c - cmin) / ext) * 2097152.0f;
    if (!(x < 2097152.0f)) return kLbGrid - 1u;
    return x > 0.0f ? (uint32_t)x : 0u;
}

// bit k of a 21-bit value to bit 3k
GM_HD uint64_t lb_spread(uint32_t q)
{
    uint64_t x = q & 0x1FFFFFu;
    x = (x | (x << 32)) & 0x001F00000000FFFFull;
    x = (x | (x << 16)) & 0x001F0000FF0000FFull;
    x = (x | (x << 8)) & 0x100F00F00F00F00Full;
    x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}

// rule 4
GM_HD uint64_t lb_key(const float* c, const float* cmin, const float* ext)
{
    return (lb_spread(lb_quantise(c[0], cmin[0], ext[0])) << 2) | (lb_spread(lb_quantise(c[1], cmin[1], ext[1])) << 1) |
           lb_spread(lb_quantise(c[2], cmin[2], ext[2]));
}

GM_HD int lb_clz64(uint64_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)x);
#else
    return x ? __builtin_clzll(x) : 64;
#endif
}
GM_HD int lb_clz32(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __clz((int)x);
#else
    return x ? __builtin_clz(x) : 32;
#endif
}

// rule 5: sorted positions a != b, both inside the range
GM_HD int lb_delta(const uint64_t* keys, int64_t a, int64_t b)
{
    const uint64_t ka = keys[a], kb = keys[b];
    return ka != kb ? lb_clz64(ka ^ kb) : 64 + lb_clz32((uint32_t)a ^ (uint32_t)b);
}
GM_HD int lb_delta_r(const uint64_t* keys, int64_t n, int64_t a, int64_t b) { return (b < 0 || b >= n) ? -1 : lb_delta(keys, a, b); }

// The split of the node that covers positions [first, last], last > first: the last position whose highest differing bit against
// `first` lies below the node's own, so that the children are [first, split] and [split + 1, last] (Karras 2012, section 3).
GM_HD int64_t lb_split(const uint64_t* keys, int64_t first, int64_t last)
{
    const int dnode = lb_delta(keys, first, last);
    int64_t s = first, step = last - first;
    do {
        step = (step + 1) >> 1;
        const int64_t t = s + step;
        if (t < last && lb_delta(keys, first, t) > dnode) s = t;
    } while (step > 1);
    return s;
}

// the triangle record of rule 8
GM_HD gmupt_triangle lb_record(const int32_t* idx3, const uint32_t* vertexMaterial)
{
    gmupt_triangle t;
    t.v[0] = idx3[0]; t.v[1] = idx3[1]; t.v[2] = idx3[2];
    t.materialID = vertexMaterial ? vertexMaterial[idx3[0]] : 0u;
    return t;
}

// what the host build and the device build report besides the arrays
struct LbResult { uint32_t numNodes, numLeaves, depth; float rootMin[3], rootMax[3]; };

// ---- host reference (pt_lbvh.cpp).  Returns "" and GMUPT_OK in *status, or the message and the status of rule 9; writes nothing on an error.
std::string lbvh_build_host(const float* verts, uint32_t numVerts, const int32_t* indices, uint32_t numTris, const uint32_t* vertexMaterial,
                            uint32_t maxLeaf, gmupt_bvh_node* nodesOut, gmupt_triangle* trisOut, int32_t* refOut, LbResult& res, int* status);

} // namespace gmupt
