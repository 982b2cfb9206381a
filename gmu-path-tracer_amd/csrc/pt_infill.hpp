// The guided infill's per-pixel arithmetic (include/gmupt.h, "Infill", states it), shared by the kernels of pt_infill.hip and the host
// rule infill_host (pt_infill.cpp): one copy of every formula, so that both run one binary32 sequence (build.py flags: no contraction,
// correctly rounded divide / sqrt, denormals kept).  The fixed tap order and the single division per channel are part of the contract.
//
// Working layout (structure of arrays, one element per pixel, row-major):
//   col  float4  rgb, state word -- the ping-pong colour; the state word (uint bits) is kIfNot / kIfOpen / kIfSource / kIfFilled
//   nm   float4  normalised normal xyz, material (uint bits)
//   xa   float4  position xyz, albedo r
//   ag   float2  albedo g, b
//   z    float   depth (read for the hole only)
// Holes keep their guides (dn_prepare zeroes those of a pixel without samples); pixels that are no surface have zeroed planes.
// A tap reads col (16 B), nm (16 B), xa (16 B), ag (8 B): 56 bytes.
#pragma once
#include "detmath.hpp"
#include "pt_denoise.hpp"   // dn_h5, dn_clamp, kDnLog2e, dn_bands

namespace gmupt {

constexpr uint32_t kIfNot = 0u, kIfOpen = 1u, kIfSource = 2u, kIfFilled = 3u;   // not a surface | hole, not yet filled | sampled | filled by an earlier pass
constexpr uint32_t kIfCounterBytes = 256;                       // head of the scratch: the four words of IfCounters, zeroed per call
constexpr uint32_t kIfScratchBytes = 2 * 16 + 16 + 16 + 8 + 4;  // per pixel: two colour buffers, nm, xa, ag, z
constexpr uint32_t kIfOneBits = 1u;                             // alpha of a filled pixel: the bits of sample count 1

struct IfParams { int passes; float sigmaNormal, sigmaPlane, sigmaAlbedo; };
struct IfPlanes { float4* nm; float4* xa; float2* ag; float* z; };
struct IfCounters { uint32_t sources, holes, filled, openLeft; };   // gmupt_infill_info's four words, in its order

GM_HD uint32_t if_state(const float4 c) { return f2u(c.w); }

// the prepare step of pixel i: beauty texel + AOV record (four float4) -> guide planes; returns the first colour texel (rgb, state word)
GM_HD float4 if_prepare(const float4 beauty, const float4 a0, const float4 a1, const float4 a2, const float4 a3, const IfPlanes& g, size_t i)
{
    const uint32_t count = f2u(beauty.w);
    const int32_t tri = (int32_t)f2u(a3.x);
    const uint32_t light = f2u(a3.z);
    const f3 nraw = mk3(a1.x, a1.y, a1.z);
    const bool surface = tri != -1 && light == 0u && length3(nraw) > 0.0f;
    if (!surface) {
        g.nm[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); g.xa[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        g.ag[i] = make_float2(0.0f, 0.0f); g.z[i] = 0.0f;
        return make_float4(beauty.x, beauty.y, beauty.z, u2f(kIfNot));
    }
    const f3 n = normalize3(nraw);
    g.nm[i] = make_float4(n.x, n.y, n.z, a3.y);   // a3.y: the material word, bits kept
    g.xa[i] = make_float4(a2.x, a2.y, a2.z, a0.x);
    g.ag[i] = make_float2(a0.y, a0.z);
    g.z[i] = a0.w;
    return make_float4(beauty.x, beauty.y, beauty.z, u2f(count > 0u ? kIfSource : kIfOpen));
}

// one tap's contribution to the sums (the order of include/gmupt.h)
struct IfSums { float sw, sr, sg, sb; };
struct IfCentre { f3 np, xp; float ar, ag, ab, denX; uint32_t material; };

GM_HD void if_tap(IfSums& a, const IfCentre& c, const float4 cq, const float4 nmq, const float4 xaq, const float2 agq, float h, const IfParams& prm)
{
    const float wn = dpow(hmax(0.0f, dot3(c.np, mk3(nmq.x, nmq.y, nmq.z))), prm.sigmaNormal);
    const float dxp = dabs(dot3(c.np, mk3(xaq.x, xaq.y, xaq.z) - c.xp)) / c.denX;
    const float da = ((dabs(xaq.w - c.ar) + dabs(agq.x - c.ag)) + dabs(agq.y - c.ab)) / prm.sigmaAlbedo;
    const float e = dexp2(-(dxp + da) * kDnLog2e);
    const float w = (h * wn) * e;
    a.sw = a.sw + w;
    a.sr = a.sr + w * cq.x; a.sg = a.sg + w * cq.y; a.sb = a.sb + w * cq.z;
}

// one pass for the open hole (x, y) at step s: (rgb', kIfFilled), or its texel as it is when it stays open.  The loads of a row of five
// taps are issued together before any of them is tested, at addresses clamped into the image (as dn_atrous).
GM_HD float4 if_fill(const float4* col, const IfPlanes& g, int W, int H, int x, int y, int s, const IfParams& prm)
{
    const size_t p = (size_t)y * W + x;
    const float4 nmp = g.nm[p], xap = g.xa[p];
    const float2 agp = g.ag[p];
    IfCentre c;
    c.np = mk3(nmp.x, nmp.y, nmp.z); c.xp = mk3(xap.x, xap.y, xap.z);
    c.ar = xap.w; c.ag = agp.x; c.ab = agp.y;
    c.denX = prm.sigmaPlane * g.z[p];
    c.material = f2u(nmp.w);
    IfSums a = { 0.0f, 0.0f, 0.0f, 0.0f };
    for (int j = -2; j <= 2; j++) {
        const int qy = y + s * j;
        if (qy < 0 || qy >= H) continue;
        const size_t row = (size_t)qy * W;
        float4 cq[5], nmq[5], xaq[5];
        float2 agq[5];
#pragma unroll
        for (int t = 0; t < 5; t++) {
            const size_t q = row + dn_clamp(x + s * (t - 2), W - 1);
            cq[t] = col[q]; nmq[t] = g.nm[q]; xaq[t] = g.xa[q]; agq[t] = g.ag[q];
        }
#pragma unroll
        for (int t = 0; t < 5; t++) {
            const int qx = x + s * (t - 2);
            if (qx < 0 || qx >= W || if_state(cq[t]) < kIfSource || f2u(nmq[t].w) != c.material) continue;
            if_tap(a, c, cq[t], nmq[t], xaq[t], agq[t], dn_h5(t - 2) * dn_h5(j), prm);
        }
    }
    if (!(a.sw > 0.0f)) return col[p];
    return make_float4(a.sr / a.sw, a.sg / a.sw, a.sb / a.sw, u2f(kIfFilled));
}

// what the last pass writes for a pixel whose working texel is c: a filled pixel its colour with the bits of count 1, every other pixel
// (no surface, source, hole still open) its input texel bit for bit
GM_HD float4 if_output(const float4 c, const float4 beauty)
{
    return if_state(c) == kIfFilled ? make_float4(c.x, c.y, c.z, u2f(kIfOneBits)) : beauty;
}

void infill_host(const float* beauty, const void* aov, int W, int H, const IfParams& prm, float* out, IfCounters* counts, int threads);   // pt_infill.cpp

} // namespace gmupt
