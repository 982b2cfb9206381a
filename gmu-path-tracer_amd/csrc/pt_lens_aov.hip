// Lens-filtered AOV planes (gmupt_render_aovs_lens, include/gmupt_lens_aov.h): the guide records of a frame with depth of field, in
// three launches per chunk of pixel rows, next to pt_aov.hip's and on its chunk scratch
//
//   k_laov_raygen   one thread per ray: the R = s*s rays of every pixel of the chunk as gmupt_ray records, pixel-major (ray k of chunk
//                   pixel j at j * R + k) -- pixel cell (a, b) through lens stratum (b, s - 1 - a), the rule of pt_lens_aov.hpp
//   k_cast_w        the QueryIO instantiation of the wide ray cast (launch_trace_wide, pt_traverse_wide.hip): one gmupt_hit per ray
//   k_laov_resolve  one thread per pixel: the R hits in order, the hit shading of k_aov_resolve, the ordered sums of the record rule
//                   and the 64-byte record as four float4 stores.  Its cost is k_aov_resolve's, the scattered triangle / property /
//                   texture reads of every sample; the twelve running sums stay in registers, no LDS, no scratch, no atomics.  The
//                   k = 0 ray is read again after the loop by the few pixels without a surface sample instead of being kept live.
//
// Arithmetic as everywhere else: binary32 in the stated order, no contraction (build.py flags).  The ray generation's body and the
// shading of one sample are pt_camera_rays.hpp's, shared with pt_aov.hip; the record rule is this file's own.
#include "pt_lens_aov.hpp"

namespace gmupt {

struct LensAovRule {
    gmupt_camera_buffer cam;
    float apertureRadius, focusDistance;
    __device__ __forceinline__ CamRay operator()(uint32_t x, uint32_t y, uint32_t s, uint32_t k) const { return lens_aov_ray(cam, apertureRadius, focusDistance, x, y, s, k); }
};

__global__ __launch_bounds__(kBlock) void k_laov_raygen(AovRaygen<LensAovRule> g) { aov_raygen(g.chunk, g.rule); }

struct LaovResolve {
    SceneView scene;
    float env[3];          // cam.envColor.rgb: the albedo of a miss
    uint32_t R;            // rays per pixel
    uint32_t npix;         // pixels of the chunk
    const float4* rays;    // the chunk's rays and hits (2 float4 each)
    const float4* hits;
    float4* out;           // 4 float4 per pixel: the chunk's first record
};

__global__ __launch_bounds__(kBlock) void k_laov_resolve(LaovResolve a)
{
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= a.npix) return;
    const size_t base = (size_t)j * a.R;
    // every sum from 0.0f in k order (include/gmupt_lens_aov.h)
    f3 sa = mk3(0.0f, 0.0f, 0.0f), sn = mk3(0.0f, 0.0f, 0.0f), sp = mk3(0.0f, 0.0f, 0.0f);
    float st = 0.0f, sr = 0.0f, sm = 0.0f;
    uint32_t coverage = 0;
    float triangle = 0.0f, material = 0.0f;     // words 3 and 5 of the first surface sample's gmupt_hit, as bits
    for (uint32_t k = 0; k < a.R; k++) {
        const float4 ok = a.rays[2 * (base + k)], dk = a.rays[2 * (base + k) + 1];
        const float4 g0 = a.hits[2 * (base + k)], g1 = a.hits[2 * (base + k) + 1];
        const f3 o = mk3(ok.x, ok.y, ok.z), d = mk3(dk.x, dk.y, dk.z);
        f3 ak, nk; float mk, rk;
        const bool surface = aov_shade(a.scene, a.env, g0, g1, d, ak, nk, mk, rk);
        sa = sa + ak; sn = sn + nk;
        if (surface) {
            if (coverage == 0) { triangle = g0.w; material = g1.y; }
            coverage++;
            st = st + g0.x;
            sp = sp + (o + d * g0.x);
            sr = sr + rk; sm = sm + mk;
        }
    }
    const float inv = (float)a.R;
    const f3 albedo = mk3(sa.x / inv, sa.y / inv, sa.z / inv);
    const f3 normal = mk3(sn.x / inv, sn.y / inv, sn.z / inv);
    float t, rough, metallic, light = 0.0f;
    f3 position;
    if (coverage > 0) {
        const float c = (float)coverage;
        t = st / c; rough = sr / c; metallic = sm / c;
        position = mk3(sp.x / c, sp.y / c, sp.z / c);
    } else {
        // no surface sample: ray k = 0 as k_aov_resolve treats its centre ray -- a light or a miss, so roughness = metallic = 0
        const float4 o0 = a.rays[2 * base], d0 = a.rays[2 * base + 1];
        const float4 h0 = a.hits[2 * base], h1 = a.hits[2 * base + 1];
        t = h0.x; rough = 0.0f; metallic = 0.0f;
        triangle = h0.w; material = h1.y; light = h1.x;
        const bool found = (int)__builtin_bit_cast(uint32_t, h0.w) >= 0 || __builtin_bit_cast(uint32_t, h1.x) > 0;
        position = found ? mk3(o0.x, o0.y, o0.z) + mk3(d0.x, d0.y, d0.z) * t : mk3(0.0f, 0.0f, 0.0f);
    }
    float4* rec = a.out + 4 * (size_t)j;
    rec[0] = make_float4(albedo.x, albedo.y, albedo.z, t);
    rec[1] = make_float4(normal.x, normal.y, normal.z, rough);
    rec[2] = make_float4(position.x, position.y, position.z, metallic);
    rec[3] = make_float4(triangle, material, light, __builtin_bit_cast(float, coverage));
}

// ---- host launchers (gmupt_capi_lens_aov.hip)
void launch_laov_raygen(const gmupt_camera_buffer& cam, const gmupt_lens& lens, uint32_t x0, uint32_t y0, uint32_t width, uint32_t rows, uint32_t samples,
                        gmupt_ray* rays, hipStream_t s)
{
    launch_raygen_kernel(k_laov_raygen, LensAovRule{ cam, lens.aperture_radius, lens.focus_distance }, x0, y0, width, rows, samples, samples * samples, rays, s);
}

void launch_laov_resolve(const RenderParams& p, uint32_t npix, uint32_t samples, const gmupt_ray* rays, const gmupt_hit* hits, gmupt_aov* out, hipStream_t s)
{
    LaovResolve a;
    a.scene = p.scene;
    a.env[0] = p.cam.envColor[0]; a.env[1] = p.cam.envColor[1]; a.env[2] = p.cam.envColor[2];
    a.R = samples * samples; a.npix = npix;
    a.rays = reinterpret_cast<const float4*>(rays); a.hits = reinterpret_cast<const float4*>(hits);
    a.out = reinterpret_cast<float4*>(out);
    if (npix) hipLaunchKernelGGL(k_laov_resolve, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, s, a);
}

} // namespace gmupt
