// AOV buffers (gmupt_render_aovs, include/gmupt.h): the per-pixel G-buffer of the camera rays, in three launches per chunk of pixel rows
//
//   k_aov_raygen   one thread per ray: the R rays of every pixel of the chunk as gmupt_ray records, pixel-major (ray k of chunk pixel j at
//                  j * R + k) -- the centre ray, then the s*s stratified rays.  The body is aov_raygen (pt_camera_rays.hpp), shared
//                  with k_laov_raygen and k_paov_raygen; the centre ray is this rule's k = 0 and the R that the launcher passes
//   k_cast_w       the QueryIO instantiation of the wide ray cast (launch_trace_wide, pt_traverse_wide.hip): one gmupt_hit per ray
//   k_aov_resolve  one thread per pixel: the R hits in order, the hit shading of k_logic (pt_shading.hpp), the ordered mean of the filtered
//                  planes, and the 64-byte record as four float4 stores
//
// Arithmetic as everywhere else: binary32 in the stated order, no contraction (build.py flags), so the records are the CPU oracle's bits.
#include "pt_camera_rays.hpp"
#include "pt_launch.hpp"

namespace gmupt {

static_assert(sizeof(gmupt_aov) == 64, "gmupt_aov is four float4");

// ray k of whole-frame pixel (x, y): the pinhole ray through the coordinates of aov_ray_coords, k = 0 the centre ray
struct PinholeAovRule {
    gmupt_camera_buffer cam;
    __device__ __forceinline__ CamRay operator()(uint32_t x, uint32_t y, uint32_t s, uint32_t k) const
    {
        float px, py;
        aov_ray_coords(x, y, s, k, px, py);
        return CamRay{ mk3(cam.position[0], cam.position[1], cam.position[2]), camera_ray_direction(cam, px, py) };
    }
};

__global__ __launch_bounds__(kBlock) void k_aov_raygen(AovRaygen<PinholeAovRule> g) { aov_raygen(g.chunk, g.rule); }

struct AovResolve {
    SceneView scene;
    float env[3];          // cam.envColor.rgb: the albedo of a miss
    uint32_t samples, R;
    uint32_t npix;         // pixels of the chunk
    const float4* rays;    // the chunk's rays and hits (2 float4 each)
    const float4* hits;
    float4* out;           // 4 float4 per pixel: the chunk's first record
};

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
    const bool surface = aov_shade(a.scene, a.env, h0, h1, d, albedo, normal, metallic, rough);
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
            coverage += aov_shade(a.scene, a.env, g0, g1, mk3(dk.x, dk.y, dk.z), ak, nk, mk, rk) ? 1u : 0u;
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
    launch_raygen_kernel(k_aov_raygen, PinholeAovRule{ cam }, x0, y0, width, rows, samples, R, rays, s);
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
