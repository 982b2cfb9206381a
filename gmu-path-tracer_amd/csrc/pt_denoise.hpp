// The a-trous denoiser's per-pixel arithmetic (include/gmupt.h states it), shared by the kernels of pt_denoise.hip and the host filter
// denoise_host (pt_denoise.cpp): one copy of every formula, so that both run one binary32 sequence (build.py flags: no contraction,
// correctly rounded divide / sqrt, denormals kept).  The fixed tap order and the single division per sum are part of the contract.
//
// Working layout: pt_guides.hpp, with
//   col  float4  rgb, variance -- the ping-pong colour + variance; variance word -1 marks an invalid pixel (valid variances are >= 0 or NaN)
//   nw   float4  normalised normal xyz, luminance l
#pragma once
#include "pt_guides.hpp"
#include "../../include/gmupt.h"

namespace gmupt {

constexpr float kDnInvalid = -1.0f;        // variance word of an invalid pixel

struct DnParams { int passes; float sigmaColor, sigmaNormal, sigmaPlane, sigmaAlbedo; };

GM_HD bool dn_valid(float v) { return !(v < 0.0f); }

GM_HD float dn_luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// the prepare step of pixel i: beauty texel + AOV record (four float4) -> guide planes; returns the first colour texel (variance word 0 or
// -1).  A pixel without samples is invalid whatever its surface: its guides are zeroed too.
GM_HD float4 dn_prepare(const float4 beauty, const float4 a0, const float4 a1, const float4 a2, const float4 a3, const GdPlanes& g, size_t i)
{
    const bool valid = gd_prepare(f2u(beauty.w) > 0u, a0, a1, a2, a3, [&] { return dn_luminance(beauty.x, beauty.y, beauty.z); }, g, i);
    return make_float4(beauty.x, beauty.y, beauty.z, valid ? 0.0f : kDnInvalid);
}

// initial variance of valid pixel (x, y): mean(l^2) - mean(l)^2 over the valid pixels of the 3x3 neighbourhood, row-major
GM_HD float dn_initial_variance(const float4* col, const float4* nw, int W, int H, int x, int y)
{
    float s1 = 0.0f, s2 = 0.0f;
    int count = 0;
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= H) continue;
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= W) continue;
            const size_t q = (size_t)qy * W + qx;
            if (!dn_valid(col[q].w)) continue;
            const float l = nw[q].w;
            s1 = s1 + l; s2 = s2 + l * l; count++;
        }
    }
    const float m1 = s1 / (float)count, m2 = s2 / (float)count;
    return hmax(0.0f, m2 - m1 * m1);
}

// one tap's contribution to the sums (the order of include/gmupt.h)
struct DnSums { float sw, sr, sg, sb, sv; };

// what gd_row5 needs of the centre pixel: which taps count (the valid ones) and what one adds
struct DnCentre {
    GdCentre c; float denL; const DnParams& prm;
    GM_HD bool texel_ok(const float4 cq) const { return dn_valid(cq.w); }
    GM_HD bool word_ok(const float4) const { return true; }
    GM_HD void tap(DnSums& a, const float4 cq, const float4 nwq, const float4 xaq, const float2 agq, float h) const
    {
        const float wn = gd_wn(c, nwq, prm.sigmaNormal);
        const float dl = dabs(c.word - nwq.w) / denL;
        const float dxp = gd_dxp(c, xaq);
        const float da = gd_da(c, xaq, agq, prm.sigmaAlbedo);
        const float e = dexp2(-((dl + dxp) + da) * kGdLog2e);
        const float w = (h * wn) * e;
        a.sw = a.sw + w;
        a.sr = a.sr + w * cq.x; a.sg = a.sg + w * cq.y; a.sb = a.sb + w * cq.z;
        a.sv = a.sv + (w * w) * cq.w;
    }
};

// one a-trous pass for valid pixel (x, y) at step s: returns (rgb', variance').  The loads of the nine variance words are issued together
// before any of them is tested, at clamped addresses, as gd_row5 issues a row's taps (invalid pixels have zeroed guide planes).
GM_HD float4 dn_atrous(const float4* col, const GdPlanes& g, int W, int H, int x, int y, int s, const DnParams& prm)
{
    const size_t p = (size_t)y * W + x;
    // 3x3 Gaussian of the variance over the valid neighbours, renormalised
    float gw = 0.0f, gv = 0.0f;
    float vq[9];
#pragma unroll
    for (int t = 0; t < 9; t++) vq[t] = col[(size_t)gd_clamp(y + t / 3 - 1, H - 1) * W + gd_clamp(x + t % 3 - 1, W - 1)].w;
#pragma unroll
    for (int t = 0; t < 9; t++) {
        const int dy = t / 3 - 1, dx = t % 3 - 1;
        if (y + dy < 0 || y + dy >= H || x + dx < 0 || x + dx >= W || !dn_valid(vq[t])) continue;
        const float k = gd_h3(dx) * gd_h3(dy);
        gw = gw + k; gv = gv + k * vq[t];
    }
    const float gp = gv / gw;
    const GdCentre gc = gd_centre(g, p, prm.sigmaPlane);
    const DnCentre c{ gc, prm.sigmaColor * dsqrt(gp) + 1e-6f, prm };
    DnSums a = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    for (int j = -2; j <= 2; j++) gd_row5(col, g, W, H, x, y, s, j, c, a);
    if (!(a.sw > 0.0f)) return col[p];
    return make_float4(a.sr / a.sw, a.sg / a.sw, a.sb / a.sw, a.sv / (a.sw * a.sw));
}

void denoise_host(const float* beauty, const void* aov, int W, int H, const DnParams& prm, float* out, int threads);   // pt_denoise.cpp

} // namespace gmupt
