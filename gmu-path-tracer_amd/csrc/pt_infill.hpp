// The guided infill's per-pixel arithmetic (include/gmupt.h, "Infill", states it), shared by the kernels of pt_infill.hip and the host
// rule infill_host (pt_infill.cpp): one copy of every formula, so that both run one binary32 sequence (build.py flags: no contraction,
// correctly rounded divide / sqrt, denormals kept).  The fixed tap order and the single division per channel are part of the contract.
//
// Working layout: pt_guides.hpp, with
//   col  float4  rgb, state word -- the ping-pong colour; the state word (uint bits) is kIfNot / kIfOpen / kIfSource / kIfFilled
//   nw   float4  normalised normal xyz, material (uint bits)
// Holes keep their guides (dn_prepare zeroes those of a pixel without samples); pixels that are no surface have zeroed planes.
#pragma once
#include "pt_guides.hpp"

namespace gmupt {

constexpr uint32_t kIfNot = 0u, kIfOpen = 1u, kIfSource = 2u, kIfFilled = 3u;   // not a surface | hole, not yet filled | sampled | filled by an earlier pass
constexpr uint32_t kIfCounterBytes = 256;                       // head of the scratch: the four words of IfCounters, zeroed per call
constexpr uint32_t kIfOneBits = 1u;                             // alpha of a filled pixel: the bits of sample count 1

struct IfParams { int passes; float sigmaNormal, sigmaPlane, sigmaAlbedo; };
struct IfCounters { uint32_t sources, holes, filled, openLeft; };   // gmupt_infill_info's four words, in its order

GM_HD uint32_t if_state(const float4 c) { return f2u(c.w); }

// the prepare step of pixel i: beauty texel + AOV record (four float4) -> guide planes; returns the first colour texel (rgb, state word)
GM_HD float4 if_prepare(const float4 beauty, const float4 a0, const float4 a1, const float4 a2, const float4 a3, const GdPlanes& g, size_t i)
{
    if (!gd_prepare(true, a0, a1, a2, a3, [&] { return a3.y; }, g, i)) return make_float4(beauty.x, beauty.y, beauty.z, u2f(kIfNot));
    return make_float4(beauty.x, beauty.y, beauty.z, u2f(f2u(beauty.w) > 0u ? kIfSource : kIfOpen));
}

// one tap's contribution to the sums (the order of include/gmupt.h)
struct IfSums { float sw, sr, sg, sb; };

// what gd_row5 needs of the hole: which taps count (sources and filled pixels of its material) and what one adds
struct IfCentre {
    GdCentre c; const IfParams& prm;
    GM_HD bool texel_ok(const float4 cq) const { return !(if_state(cq) < kIfSource); }
    GM_HD bool word_ok(const float4 nwq) const { return f2u(nwq.w) == f2u(c.word); }
    GM_HD void tap(IfSums& a, const float4 cq, const float4 nwq, const float4 xaq, const float2 agq, float h) const
    {
        const float wn = gd_wn(c, nwq, prm.sigmaNormal);
        const float dxp = gd_dxp(c, xaq);
        const float da = gd_da(c, xaq, agq, prm.sigmaAlbedo);
        const float e = dexp2(-(dxp + da) * kGdLog2e);
        const float w = (h * wn) * e;
        a.sw = a.sw + w;
        a.sr = a.sr + w * cq.x; a.sg = a.sg + w * cq.y; a.sb = a.sb + w * cq.z;
    }
};

// one pass for the open hole (x, y) at step s: (rgb', kIfFilled), or its texel as it is when it stays open
GM_HD float4 if_fill(const float4* col, const GdPlanes& g, int W, int H, int x, int y, int s, const IfParams& prm)
{
    const size_t p = (size_t)y * W + x;
    const IfCentre c{ gd_centre(g, p, prm.sigmaPlane), prm };
    IfSums a = { 0.0f, 0.0f, 0.0f, 0.0f };
    for (int j = -2; j <= 2; j++) gd_row5(col, g, W, H, x, y, s, j, c, a);
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
