// AOV buffers (gmupt_render_aovs, include/gmupt.h): the per-pixel G-buffer of the camera rays, in three launches per chunk of pixel rows
//
//   k_aov_raygen   one thread per ray: the R rays of every pixel of the chunk as gmupt_ray records, pixel-major (ray k of chunk pixel j at
//                  j * R + k) -- the centre ray, then the s*s stratified rays
//   k_cast_w       the QueryIO instantiation of the wide ray cast (launch_trace_wide, pt_traverse_wide.hip): one gmupt_hit per ray
//   k_aov_resolve  one thread per pixel: the R hits in order, the hit shading of k_logic (pt_shading.hpp), the ordered mean of the filtered
//                  planes, and the 64-byte record as four float4 stores
//
// Arithmetic as everywhere else: binary32 in the stated order, no contraction (build.py flags), so the records are the CPU oracle's bits.
#include "pt_device.hpp"
#include "detmath.hpp"
#include "pt_shading.hpp"
#include "pt_launch.hpp"

namespace gmupt {

static_assert(sizeof(gmupt_aov) == 64, "gmupt_aov is four float4");

struct AovRaygen {
    gmupt_camera_buffer cam;
    uint32_t x0, y0;     // whole-frame coordinates of the chunk's first pixel
    uint32_t width;      // pixels per row
    uint32_t samples, R; // s, rays per pixel
    uint32_t n;          // rays of the chunk (rows * width * R <= GMUPT_AOV_CHUNK_RAYS)
    float4* rays;        // 2 float4 per gmupt_ray
};

__global__ __launch_bounds__(kBlock) void k_aov_raygen(AovRaygen g)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= g.n) return;
    const uint32_t pix = i / g.R, k = i - pix * g.R;
    const uint32_t ly = pix / g.width, lx = pix - ly * g.width;
    float px, py;
    aov_ray_coords(g.x0 + lx, g.y0 + ly, g.samples, k, px, py);
    const f3 d = camera_ray_direction(g.cam, px, py);
    g.rays[2 * (size_t)i] = make_float4(g.cam.position[0], g.cam.position[1], g.cam.position[2], kFltMax);   // tmax = FLT_MAX (structs.h:9)
    g.rays[2 * (size_t)i + 1] = make_float4(d.x, d.y, d.z, 0.0f);
}

struct AovResolve {
    SceneView scene;
    float env[3];          // cam.envColor.rgb: the albedo of a miss
    uint32_t samples, R;
    uint32_t npix;         // pixels of the chunk
    const float4* rays;    // the chunk's rays and hits (2 float4 each)
    const float4* hits;
    float4* out;           // 4 float4 per pixel: the chunk's first record
};

// the shading of one ray's closest hit (include/gmupt.h): albedo, normal, metallic, roughness; returns true for a triangle hit without a nearer light
__device__ __forceinline__ bool aov_shade(const AovResolve& a, const float4 h0, const float4 h1, f3 dir, f3& albedo, f3& normal, float& metallic, float& rough)
{
    const int tri = (int)__builtin_bit_cast(uint32_t, h0.w);
    const uint32_t light = __builtin_bit_cast(uint32_t, h1.x);
    normal = mk3(0.0f, 0.0f, 0.0f); metallic = 0.0f; rough = 0.0f;
    if (light > 0) { albedo = sample_light_color(a.scene.lights, light); return false; }
    if (tri < 0) { albedo = mk3(a.env[0], a.env[1], a.env[2]); return false; }
    // the record finish_extension_ray stores: vertex indices and material of the triangle, bary = (1 - u - v, u, v)
    const int4 T = *reinterpret_cast<const int4*>(&a.scene.tris[tri]);
    const HitProps hp = material_hit_properties(a.scene, (uint32_t)T.x, (uint32_t)T.y, (uint32_t)T.z, (uint32_t)T.w,
                                                mk3(1.0f - h0.y - h0.z, h0.y, h0.z), [&]() { return dir; });
    albedo = hp.color; normal = hp.normal; metallic = hp.metallic; rough = hp.roughness;
    return true;
}

__global__ __launch_bounds__(kBlock) void k_aov_resolve(AovResolve a)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= a.npix) return;
    const size_t base = (size_t)j * a.R;
    // the centre ray (k = 0)
    const float4 o0 = a.rays[2 * base], d0 = a.rays[2 * base + 1];
    const float4 h0 = a.hits[2 * base], h1 = a.hits[2 * base + 1];
    const f3 o = mk3(o0.x, o0.y, o0.z), d = mk3(d0.x, d0.y, d0.z);
    f3 albedo, normal; float metallic, rough;
    const bool surface = aov_shade(a, h0, h1, d, albedo, normal, metallic, rough);
    uint32_t coverage = surface ? 1u : 0u;
    const float t = h0.x;
    const bool found = (int)__builtin_bit_cast(uint32_t, h0.w) >= 0 || __builtin_bit_cast(uint32_t, h1.x) > 0;
    const f3 position = found ? o + d * t : mk3(0.0f, 0.0f, 0.0f);     // surfacePoint of finish_extension_ray, at the nearer light when there is one
    if (a.R > 1) {
        // the s*s stratified rays, summed in k order from 0.0f, then divided by s*s (include/gmupt.h)
        f3 sa = mk3(0.0f, 0.0f, 0.0f), sn = mk3(0.0f, 0.0f, 0.0f);
        coverage = 0;
        for (uint32_t k = 1; k < a.R; k++) {
            const float4 dk = a.rays[2 * (base + k) + 1];
            const float4 g0 = a.hits[2 * (base + k)], g1 = a.hits[2 * (base + k) + 1];
            f3 ak, nk; float mk, rk;
            coverage += aov_shade(a, g0, g1, mk3(dk.x, dk.y, dk.z), ak, nk, mk, rk) ? 1u : 0u;
            sa = sa + ak; sn = sn + nk;
        }
        const float inv = (float)(a.samples * a.samples);
        albedo = mk3(sa.x / inv, sa.y / inv, sa.z / inv);
        normal = mk3(sn.x / inv, sn.y / inv, sn.z / inv);
    }
    float4* rec = a.out + 4 * (size_t)j;
    rec[0] = make_float4(albedo.x, albedo.y, albedo.z, t);
    rec[1] = make_float4(normal.x, normal.y, normal.z, rough);
    rec[2] = make_float4(position.x, position.y, position.z, metallic);
    rec[3] = make_float4(h0.w, h1.y, h1.x, __builtin_bit_cast(float, coverage));   // triangle, material, light (gmupt_hit words 3, 5, 4), coverage
}

// ---- host launchers (gmupt_capi.hip: gmupt_render_aovs).  rays / hits: the chunk scratch, 32 bytes per ray; out: the chunk's first record.
void launch_aov_raygen(const gmupt_camera_buffer& cam, uint32_t x0, uint32_t y0, uint32_t width, uint32_t rows, uint32_t samples, uint32_t R,
                       gmupt_ray* rays, hipStream_t s)
{
    AovRaygen g;
    g.cam = cam; g.x0 = x0; g.y0 = y0; g.width = width; g.samples = samples; g.R = R; g.n = rows * width * R;
    g.rays = reinterpret_cast<float4*>(rays);
    if (g.n) hipLaunchKernelGGL(k_aov_raygen, dim3((g.n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, g);
}

void launch_aov_resolve(const RenderParams& p, uint32_t npix, uint32_t samples, uint32_t R, const gmupt_ray* rays, const gmupt_hit* hits,
                        gmupt_aov* out, hipStream_t s)
{
    AovResolve a;
    a.scene = p.scene;
    a.env[0] = p.cam.envColor[0]; a.env[1] = p.cam.envColor[1]; a.env[2] = p.cam.envColor[2];
    a.samples = samples; a.R = R; a.npix = npix;
    a.rays = reinterpret_cast<const float4*>(rays); a.hits = reinterpret_cast<const float4*>(hits);
    a.out = reinterpret_cast<float4*>(out);
    if (npix) hipLaunchKernelGGL(k_aov_resolve, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, s, a);
}

} // namespace gmupt
