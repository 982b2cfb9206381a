// The motion plane (gmupt_render_aovs_motion; include/gmupt.h states it)
//
//   k_mv_resolve   one thread per pixel of an AOV chunk, after k_aov_resolve on the same hits: the centre ray's gmupt_hit (ray pixel * R of
//                  the chunk scratch), the triangle record, its three vertices now and in the caller's previous pose, the position the
//                  AOV resolve has just written -> one 16-byte gmupt_motion record.  No LDS.
//
// The per-pixel arithmetic is pt_motion.hpp, which the host function (pt_motion.cpp) runs too.
#include "pt_device.hpp"
#include "detmath.hpp"
#include "pt_motion.hpp"
#include "pt_launch.hpp"

namespace gmupt {

struct MvResolve {
    const float4* hits;            // the chunk's hits (2 float4 each), R per pixel
    const float4* aov;             // the chunk's first AOV record (4 float4 per pixel)
    const gmupt_triangle* tris;
    const float* now; const float* prev;
    uint32_t numTris, numVerts;
    uint32_t R, npix;
    float4* out;                   // the chunk's first motion record
};

__global__ __launch_bounds__(kBlock) void k_mv_resolve(MvResolve a)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= a.npix) return;
    const size_t base = (size_t)j * a.R;
    const float4 h0 = a.hits[2 * base], h1 = a.hits[2 * base + 1];
    const int32_t tri = (int32_t)f2u(h0.w);
    const uint32_t light = f2u(h1.x);
    float4 rec = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (tri >= 0 && (uint32_t)tri < a.numTris && light == 0u) {
        const int4 T = *reinterpret_cast<const int4*>(&a.tris[tri]);
        const int32_t t[3] = { T.x, T.y, T.z };
        if ((uint32_t)T.x < a.numVerts && (uint32_t)T.y < a.numVerts && (uint32_t)T.z < a.numVerts) {   // bind validated them; never out of bounds
            const float4 x = a.aov[4 * (size_t)j + 2];
            rec = mv_pixel(tri, h0.y, h0.z, light, t, a.now, a.prev, mk3(x.x, x.y, x.z));
        }
    }
    a.out[j] = rec;
}

// ---- host launcher (gmupt_capi.hip: gmupt_render_aovs_motion).  hits: the chunk scratch; aov / out: the chunk's first records.
void launch_mv_resolve(const SceneView& scene, const float* prevVerts, uint32_t npix, uint32_t R, const gmupt_hit* hits, const gmupt_aov* aov,
                       gmupt_motion* out, hipStream_t s)
{
    MvResolve a;
    a.hits = reinterpret_cast<const float4*>(hits); a.aov = reinterpret_cast<const float4*>(aov);
    a.tris = scene.tris; a.now = scene.verts; a.prev = prevVerts;
    a.numTris = scene.numTris; a.numVerts = scene.numVerts;
    a.R = R; a.npix = npix;
    a.out = reinterpret_cast<float4*>(out);
    if (npix) hipLaunchKernelGGL(k_mv_resolve, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, s, a);
}

} // namespace gmupt
