// Hit shading shared by the renderer's logic stage (k_logic, pt_kernels.hip) and the AOV resolve (k_aov_resolve, pt_aov.hip):
// the texture lookups and setMaterialHitProperties of logic.hlsl:79-133, and sampleLight's colour (logic.hlsl:192-197).
// One copy of the arithmetic, so the AOV planes are what the renderer computes for the same hit, bit for bit.
#pragma once
#include "pt_device.hpp"
#include "detmath.hpp"

namespace gmupt {

// ------------------------------------------------------------------------------------------------ textures
// SampleLevel(linear, wrap) on an RGBA8 UNORM array (logic.hlsl:100,104,111; sampler Scene.cpp:180-192): texel centres at
// u*size - 0.5, fp32 weights, lerp(a,b,t) = a + t*(b-a), horizontal pairs first, c/255 decode.  Stated arithmetic.
__device__ __forceinline__ float4 sample_bilinear(const SceneView& sc, int which, float u, float v, int layer)
{
    float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const uint8_t* tex = sc.tex[which];
    const int n = (int)sc.texSize[which];
    if (!tex || n <= 0 || sc.texLayers[which] == 0) return out;
    if (layer < 0) layer = 0;
    if (layer >= (int)sc.texLayers[which]) layer = (int)sc.texLayers[which] - 1;
    float x = u * (float)n - 0.5f, y = v * (float)n - 0.5f;
    if (!(dabs(x) < 1.0e9f)) x = 0.0f;
    if (!(dabs(y) < 1.0e9f)) y = 0.0f;
    const float x0 = dfloor(x), y0 = dfloor(y);
    const float fx = x - x0, fy = y - y0;
    int ix0 = (int)x0 % n; if (ix0 < 0) ix0 += n;
    int iy0 = (int)y0 % n; if (iy0 < 0) iy0 += n;
    const int ix1 = (ix0 + 1 == n) ? 0 : ix0 + 1, iy1 = (iy0 + 1 == n) ? 0 : iy0 + 1;
    const uchar4* base = reinterpret_cast<const uchar4*>(tex) + (size_t)layer * n * n;
    const uchar4 c00 = base[(size_t)iy0 * n + ix0], c10 = base[(size_t)iy0 * n + ix1], c01 = base[(size_t)iy1 * n + ix0], c11 = base[(size_t)iy1 * n + ix1];
#define GM_BILERP(ch) { const float a = (float)c00.ch / 255.0f, b = (float)c10.ch / 255.0f, c = (float)c01.ch / 255.0f, d = (float)c11.ch / 255.0f; \
                        const float r0 = a + fx * (b - a), r1 = c + fx * (d - c); out.ch = r0 + fy * (r1 - r0); }
    GM_BILERP(x) GM_BILERP(y) GM_BILERP(z) GM_BILERP(w)
#undef GM_BILERP
    return out;
}

// ------------------------------------------------------------------------------------------------ setMaterialHitProperties
struct HitProps { f3 color; float metallic, roughness; f3 normal; uint32_t materialType; };

// logic.hlsl:79-133 for a triangle hit: t0..t2 / tm = the triangle record (vertex indices, materialID) as extensionRayCast.hlsl stores it,
// bary = (1 - u - v, u, v).  ray_direction() gives the direction of the ray that hit; it is only called for a normal-mapped material
// (k_logic then reads the path state exactly where it did before the code was shared).
template <class RayDir>
__device__ __forceinline__ HitProps material_hit_properties(const SceneView& sc, uint32_t t0, uint32_t t1, uint32_t t2, uint32_t tm, f3 bary, RayDir ray_direction)
{
    const uint32_t i0 = (uint32_t)(float)t0, i1 = (uint32_t)(float)t1, i2 = (uint32_t)(float)t2; // :82 float round trip
    const gmupt_tri_props* tp = sc.props;
    f3 n0 = mk3(tp[i0].normal[0], tp[i0].normal[1], tp[i0].normal[2]);
    f3 n1 = mk3(tp[i1].normal[0], tp[i1].normal[1], tp[i1].normal[2]);
    f3 n2 = mk3(tp[i2].normal[0], tp[i2].normal[1], tp[i2].normal[2]);
    f3 normal = (n0 * bary.x + n1 * bary.y) + n2 * bary.z;          // :94
    gmupt_material m = sc.materials[tm < GMUPT_MAX_LIGHTS ? tm : 0u]; // :96
    if (m.textureIndices[0] >= 0 || m.textureIndices[1] >= 0 || m.textureIndices[2] >= 0) {
        const float tu = (tp[i0].uv[0] * bary.x + tp[i1].uv[0] * bary.y) + tp[i2].uv[0] * bary.z; // :93
        const float tv = (tp[i0].uv[1] * bary.x + tp[i1].uv[1] * bary.y) + tp[i2].uv[1] * bary.z;
        if (m.textureIndices[0] >= 0) {                        // :99-100
            const float4 t = sample_bilinear(sc, 0, tu, tv, m.textureIndices[0]);
            m.color[0] = t.x; m.color[1] = t.y; m.color[2] = t.z; m.color[3] = t.w;
        }
        if (m.textureIndices[1] >= 0) {                        // :102-107 metallic = .x, roughness = .y
            const float4 t = sample_bilinear(sc, 1, tu, tv, m.textureIndices[1]);
            m.metallic = t.x; m.roughness = t.y;
        }
        if (m.textureIndices[2] >= 0) {                        // :109-124 normal map
            const float4 t = sample_bilinear(sc, 2, tu, tv, m.textureIndices[2]);
            const f3 data = mk3(t.x * 2.0f - 1.0f, t.y * 2.0f - 1.0f, t.z * 2.0f - 1.0f);
            const f3 rayDirection = ray_direction();
            const f3 ortNormal = dot3(normal, rayDirection) <= 0.0f ? normal : normal * -1.0f;
            const f3 up = dabs(ortNormal.z) < 0.999f ? mk3(0.0f, 0.0f, 1.0f) : mk3(1.0f, 0.0f, 0.0f);
            const f3 tangent = normalize3(cross3(up, ortNormal));
            const f3 bitangent = cross3(ortNormal, tangent);
            normal = (tangent * data.x + bitangent * data.y) + ortNormal * data.z; // :123 (not renormalised)
        }
    }
    HitProps hp;
    hp.color = mk3(m.color[0], m.color[1], m.color[2]);               // :128
    hp.metallic = m.metallic;
    hp.roughness = hmax(0.014f, m.roughness);                         // :126
    hp.normal = normal;                                               // :130
    hp.materialType = m.materialType;
    return hp;
}

// sampleLight (logic.hlsl:192-197): the colour of light sphere isEmitter - 1 (isEmitter > 0), emission / max(emission)
__device__ __forceinline__ f3 sample_light_color(const gmupt_light* lights, uint32_t isEmitter)
{
    uint32_t li = isEmitter - 1; if (li >= GMUPT_MAX_LIGHTS) li = GMUPT_MAX_LIGHTS - 1;
    const gmupt_light L = lights[li];
    float emax = hmax(L.emission[0], hmax(L.emission[1], L.emission[2]));
    return mk3(L.emission[0] / emax, L.emission[1] / emax, L.emission[2] / emax);
}

// ------------------------------------------------------------------------------------------------ camera rays
// newPath.hlsl:36-39 with the jitter folded into (px, py): the direction of the primary ray through whole-frame pixel coordinates (px, py).
// Host (gmupt_camera_pick_ray, gmupt_aov_ray) and device (k_aov_raygen) evaluate the same binary32 sequence.
GM_HD f3 camera_ray_direction(const gmupt_camera_buffer& cam, float px, float py)
{
    const float u = px * cam.pixelSize[0], v = py * cam.pixelSize[1];
    const f3 ulc = mk3(cam.upperLeftCorner[0], cam.upperLeftCorner[1], cam.upperLeftCorner[2]);
    const f3 hor = mk3(cam.horizontal[0], cam.horizontal[1], cam.horizontal[2]);
    const f3 ver = mk3(cam.vertical[0], cam.vertical[1], cam.vertical[2]);
    return normalize3((ulc + hor * u) - ver * v);
}
// the whole-frame coordinates of AOV ray k of pixel (x, y) at s samples (include/gmupt.h): k = 0 the centre, k = 1 + b*s + a the stratified ray
GM_HD void aov_ray_coords(uint32_t x, uint32_t y, uint32_t s, uint32_t k, float& px, float& py)
{
    px = (float)x; py = (float)y;
    if (k > 0) {
        const uint32_t a = (k - 1) % s, b = (k - 1) / s;
        px = px + ((float)(2 * a + 1) / (float)s - 1.0f);
        py = py + ((float)(2 * b + 1) / (float)s - 1.0f);
    }
}

} // namespace gmupt
