// The motion plane's per-pixel arithmetic (include/gmupt.h states it), shared by k_mv_resolve (pt_motion.hip) and motion_host (pt_motion.cpp): one
// copy of the barycentric sums and the displacement, so that both run one binary32 sequence (build.py flags: no contraction).
//
// Record layout: the public gmupt_motion, 16 bytes = one float4 per pixel, row-major:  prev_position xyz, flags bits.
#pragma once
#include "detmath.hpp"
#include "../../include/gmupt.h"

namespace gmupt {

static_assert(sizeof(gmupt_motion) == 16, "gmupt_motion is one float4");

// (w * a + u * b) + v * c per component
GM_HD f3 mv_bary(float w, float u, float v, const float* a, const float* b, const float* c)
{
    return mk3((w * a[0] + u * b[0]) + v * c[0], (w * a[1] + u * b[1]) + v * c[1], (w * a[2] + u * b[2]) + v * c[2]);
}

GM_HD float mv_move(float x, float bprev, float bnow) { return bprev == bnow ? x : x + (bprev - bnow); }

// the centre ray's hit (triangle, u, v, light), the triangle's vertex indices t (all below the vertex count), both vertex arrays and the
// position the AOV record holds -> the motion record
GM_HD float4 mv_pixel(int32_t tri, float u, float v, uint32_t light, const int32_t* t, const float* now, const float* prev, const f3 pos)
{
    if (tri < 0 || light > 0u) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const size_t i0 = 3 * (size_t)t[0], i1 = 3 * (size_t)t[1], i2 = 3 * (size_t)t[2];
    const float w = (1.0f - u) - v;
    const f3 bn = mv_bary(w, u, v, now + i0, now + i1, now + i2);
    const f3 bp = mv_bary(w, u, v, prev + i0, prev + i1, prev + i2);
    return make_float4(mv_move(pos.x, bp.x, bn.x), mv_move(pos.y, bp.y, bn.y), mv_move(pos.z, bp.z, bn.z), u2f(1u));
}

void motion_host(const gmupt_hit* hits, const gmupt_aov* aov, size_t n, const gmupt_triangle* tris, const float* now, const float* prev, gmupt_motion* out);   // pt_motion.cpp

} // namespace gmupt
