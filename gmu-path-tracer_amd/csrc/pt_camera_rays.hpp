// What the camera-ray features (pt_aov.hip, pt_lens.hip, pt_lens_aov.hip, pt_projection.hip) have in common, one copy of each:
//   CamRay / store_ray   the ray a rule yields, and that ray as a gmupt_ray record on the host
//   AovChunk, aov_raygen, launch_raygen_kernel
//                        the ray generation of one chunk of pixel rows: one thread per ray, pixel-major (ray k of chunk pixel j at
//                        j * R + k).  What differs between the plain, the lens and the projected records is the rule, a functor
//                        (x, y, s, k) -> CamRay that carries its own parameters; the kernels are three thin __global__ wrappers
//                        around the one body, under their own names.
//   aov_shade            the shading of one sample's closest hit, for k_aov_resolve and k_laov_resolve
// The fresh-path jitter of stage_new_path is not here: pt_kernels.hip keeps its own lines (pt_lens.hpp says why).
#pragma once
#include "pt_shading.hpp"

#include <cstring>

namespace gmupt {

struct CamRay { f3 origin, direction; };

// a rule's ray as a gmupt_ray: tmax = FLT_MAX (the reference's starting distance, structs.h:9), pad = 0
inline void store_ray(const f3& origin, const f3& direction, gmupt_ray* out)
{
    std::memset(out, 0, sizeof(*out));
    out->origin[0] = origin.x; out->origin[1] = origin.y; out->origin[2] = origin.z;
    out->direction[0] = direction.x; out->direction[1] = direction.y; out->direction[2] = direction.z;
    out->tmax = kFltMax;
}
inline void store_ray(const CamRay& r, gmupt_ray* out) { store_ray(r.origin, r.direction, out); }

struct AovChunk {
    uint32_t x0, y0;     // whole-frame coordinates of the chunk's first pixel
    uint32_t width;      // pixels per row
    uint32_t samples, R; // s, rays per pixel
    uint32_t n;          // rays of the chunk (rows * width * R <= GMUPT_AOV_CHUNK_RAYS)
    float4* rays;        // 2 float4 per gmupt_ray
};

// the argument of a ray-generation kernel: the rule with its parameters, then the chunk
template <class Rule> struct AovRaygen { Rule rule; AovChunk chunk; };

template <class Rule> __device__ __forceinline__ void aov_raygen(const AovChunk& c, const Rule& rule)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= c.n) return;
    const uint32_t pix = i / c.R, k = i - pix * c.R;
    const uint32_t ly = pix / c.width, lx = pix - ly * c.width;
    const CamRay r = rule(c.x0 + lx, c.y0 + ly, c.samples, k);
    c.rays[2 * (size_t)i] = make_float4(r.origin.x, r.origin.y, r.origin.z, kFltMax);   // tmax = FLT_MAX
    c.rays[2 * (size_t)i + 1] = make_float4(r.direction.x, r.direction.y, r.direction.z, 0.0f);
}

// rays: the chunk scratch of gmupt_render_aovs, 32 bytes per ray; R: the rays per pixel that `rule` is asked for (k = 0 .. R - 1)
template <class Rule> void launch_raygen_kernel(void (*kernel)(AovRaygen<Rule>), const Rule& rule, uint32_t x0, uint32_t y0, uint32_t width, uint32_t rows,
                                             uint32_t samples, uint32_t R, gmupt_ray* rays, hipStream_t s)
{
    const AovRaygen<Rule> g{ rule, { x0, y0, width, samples, R, rows * width * R, reinterpret_cast<float4*>(rays) } };
    if (g.chunk.n) hipLaunchKernelGGL(kernel, dim3((g.chunk.n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, g);
}

// the shading of one ray's closest hit (include/gmupt.h): albedo, normal, metallic, roughness; env: cam.envColor.rgb, the albedo of a
// miss.  Returns true for a surface sample: a triangle hit without a nearer light
__device__ __forceinline__ bool aov_shade(const SceneView& scene, const float (&env)[3], const float4 h0, const float4 h1, f3 dir, f3& albedo, f3& normal,
                                          float& metallic, float& rough)
{
    const int tri = (int)__builtin_bit_cast(uint32_t, h0.w);
    const uint32_t light = __builtin_bit_cast(uint32_t, h1.x);
    normal = mk3(0.0f, 0.0f, 0.0f); metallic = 0.0f; rough = 0.0f;
    if (light > 0) { albedo = sample_light_color(scene.lights, light); return false; }
    if (tri < 0) { albedo = mk3(env[0], env[1], env[2]); return false; }
    // the record finish_extension_ray stores: vertex indices and material of the triangle, bary = (1 - u - v, u, v)
    const int4 T = *reinterpret_cast<const int4*>(&scene.tris[tri]);
    const HitProps hp = material_hit_properties(scene, (uint32_t)T.x, (uint32_t)T.y, (uint32_t)T.z, (uint32_t)T.w,
                                                mk3(1.0f - h0.y - h0.z, h0.y, h0.z), [&]() { return dir; });
    albedo = hp.color; normal = hp.normal; metallic = hp.metallic; rough = hp.roughness;
    return true;
}

} // namespace gmupt
