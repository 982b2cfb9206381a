// The a-trous denoiser's per-pixel arithmetic (include/gmupt.h states it), shared by the kernels of pt_denoise.hip and the host filter
// gmupt_denoise_host: one copy of every formula, so that both run one binary32 sequence (build.py flags: no contraction, correctly
// rounded divide / sqrt, denormals kept).  The fixed tap order and the single division per sum are part of the contract.
//
// Working layout (structure of arrays, one element per pixel, row-major):
//   col  float4  rgb, variance -- the ping-pong colour + variance; variance word -1 marks an invalid pixel (valid variances are >= 0 or NaN)
//   nl   float4  normalised normal xyz, luminance l
//   xa   float4  position xyz, albedo r
//   ag   float2  albedo g, b
//   z    float   depth (read for the centre pixel only)
// A tap reads col (16 B), nl (16 B), xa (16 B), ag (8 B): 56 bytes, everything the weight and the sums need.
#pragma once
#include "detmath.hpp"
#include "../../include/gmupt.h"

#include <algorithm>
#include <thread>
#include <vector>

namespace gmupt {

constexpr float kDnInvalid = -1.0f;        // variance word of an invalid pixel
constexpr float kDnLog2e = 1.44269504f;    // exp(-d) = exp2(-d * log2(e))
constexpr uint32_t kDnTapBytes = 16 + 16 + 16 + 8;             // what one tap loads: col, nl, xa, ag
constexpr uint32_t kDnScratchBytes = 2 * 16 + 16 + 16 + 8 + 4; // per pixel: two colour buffers, nl, xa, ag, z

struct DnParams { int passes; float sigmaColor, sigmaNormal, sigmaPlane, sigmaAlbedo; };

struct DnPlanes {
    float4* nl; float4* xa; float2* ag; float* z;
};

GM_HD bool dn_valid(float v) { return !(v < 0.0f); }

GM_HD float dn_luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// weight of a-trous tap i (-2..2): {1/16, 1/4, 3/8, 1/4, 1/16}; of the 3x3 variance Gaussian (-1..1): {1/4, 1/2, 1/4}
GM_HD float dn_h5(int i) { return i == 0 ? 0.375f : (i == 1 || i == -1) ? 0.25f : 0.0625f; }
GM_HD float dn_h3(int i) { return i == 0 ? 0.5f : 0.25f; }

// the prepare step of pixel i: beauty texel + AOV record (four float4) -> guide planes; returns the first colour texel (variance word 0 or -1)
GM_HD float4 dn_prepare(const float4 beauty, const float4 a0, const float4 a1, const float4 a2, const float4 a3, const DnPlanes& g, size_t i)
{
    const uint32_t count = f2u(beauty.w);
    const int32_t tri = (int32_t)f2u(a3.x);
    const uint32_t light = f2u(a3.z);
    const f3 nraw = mk3(a1.x, a1.y, a1.z);
    const bool valid = count > 0u && tri != -1 && light == 0u && length3(nraw) > 0.0f;
    if (!valid) {
        g.nl[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); g.xa[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        g.ag[i] = make_float2(0.0f, 0.0f); g.z[i] = 0.0f;
        return make_float4(beauty.x, beauty.y, beauty.z, kDnInvalid);
    }
    const f3 n = normalize3(nraw);
    g.nl[i] = make_float4(n.x, n.y, n.z, dn_luminance(beauty.x, beauty.y, beauty.z));
    g.xa[i] = make_float4(a2.x, a2.y, a2.z, a0.x);
    g.ag[i] = make_float2(a0.y, a0.z);
    g.z[i] = a0.w;
    return make_float4(beauty.x, beauty.y, beauty.z, 0.0f);
}

// initial variance of valid pixel (x, y): mean(l^2) - mean(l)^2 over the valid pixels of the 3x3 neighbourhood, row-major
GM_HD float dn_initial_variance(const float4* col, const float4* nl, int W, int H, int x, int y)
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
            const float l = nl[q].w;
            s1 = s1 + l; s2 = s2 + l * l; count++;
        }
    }
    const float m1 = s1 / (float)count, m2 = s2 / (float)count;
    return hmax(0.0f, m2 - m1 * m1);
}

// dn_atrous issues the loads of the nine variance words, and of the five taps of a row, together before any of them is tested, at
// addresses clamped into the image: a load whose tap is outside or invalid is made and ignored (invalid pixels have zeroed guide planes).

GM_HD int dn_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// one tap's contribution to the sums (the order of include/gmupt.h)
struct DnSums { float sw, sr, sg, sb, sv; };
struct DnCentre { f3 np, xp; float lp, ar, ag, ab, denL, denX; };

GM_HD void dn_tap(DnSums& a, const DnCentre& c, const float4 cq, const float4 nlq, const float4 xaq, const float2 agq, float h, const DnParams& prm)
{
    const float wn = dpow(hmax(0.0f, dot3(c.np, mk3(nlq.x, nlq.y, nlq.z))), prm.sigmaNormal);
    const float dl = dabs(c.lp - nlq.w) / c.denL;
    const float dxp = dabs(dot3(c.np, mk3(xaq.x, xaq.y, xaq.z) - c.xp)) / c.denX;
    const float da = ((dabs(xaq.w - c.ar) + dabs(agq.x - c.ag)) + dabs(agq.y - c.ab)) / prm.sigmaAlbedo;
    const float e = dexp2(-((dl + dxp) + da) * kDnLog2e);
    const float w = (h * wn) * e;
    a.sw = a.sw + w;
    a.sr = a.sr + w * cq.x; a.sg = a.sg + w * cq.y; a.sb = a.sb + w * cq.z;
    a.sv = a.sv + (w * w) * cq.w;
}

// one a-trous pass for valid pixel (x, y) at step s: returns (rgb', variance')
GM_HD float4 dn_atrous(const float4* col, const DnPlanes& g, int W, int H, int x, int y, int s, const DnParams& prm)
{
    const size_t p = (size_t)y * W + x;
    // 3x3 Gaussian of the variance over the valid neighbours, renormalised
    float gw = 0.0f, gv = 0.0f;
    float vq[9];
#pragma unroll
    for (int t = 0; t < 9; t++) vq[t] = col[(size_t)dn_clamp(y + t / 3 - 1, H - 1) * W + dn_clamp(x + t % 3 - 1, W - 1)].w;
#pragma unroll
    for (int t = 0; t < 9; t++) {
        const int dy = t / 3 - 1, dx = t % 3 - 1;
        if (y + dy < 0 || y + dy >= H || x + dx < 0 || x + dx >= W || !dn_valid(vq[t])) continue;
        const float k = dn_h3(dx) * dn_h3(dy);
        gw = gw + k; gv = gv + k * vq[t];
    }
    const float gp = gv / gw;
    const float4 nlp = g.nl[p], xap = g.xa[p];
    const float2 agp = g.ag[p];
    DnCentre c;
    c.np = mk3(nlp.x, nlp.y, nlp.z); c.xp = mk3(xap.x, xap.y, xap.z); c.lp = nlp.w;
    c.ar = xap.w; c.ag = agp.x; c.ab = agp.y;
    c.denL = prm.sigmaColor * dsqrt(gp) + 1e-6f;
    c.denX = prm.sigmaPlane * g.z[p];
    DnSums a = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    for (int j = -2; j <= 2; j++) {
        const int qy = y + s * j;
        if (qy < 0 || qy >= H) continue;
        const size_t row = (size_t)qy * W;
        float4 cq[5], nlq[5], xaq[5];
        float2 agq[5];
#pragma unroll
        for (int t = 0; t < 5; t++) {
            const size_t q = row + dn_clamp(x + s * (t - 2), W - 1);
            cq[t] = col[q]; nlq[t] = g.nl[q]; xaq[t] = g.xa[q]; agq[t] = g.ag[q];
        }
#pragma unroll
        for (int t = 0; t < 5; t++) {
            const int qx = x + s * (t - 2);
            if (qx < 0 || qx >= W || !dn_valid(cq[t].w)) continue;
            dn_tap(a, c, cq[t], nlq[t], xaq[t], agq[t], dn_h5(t - 2) * dn_h5(j), prm);
        }
    }
    if (!(a.sw > 0.0f)) return col[p];
    return make_float4(a.sr / a.sw, a.sg / a.sw, a.sb / a.sw, a.sv / (a.sw * a.sw));
}

// the host filters' row bands (gmupt_denoise_host, gmupt_temporal_integrate_host): fn(y0, y1) over bands of H rows on up to `threads`
// std::threads
template <class F> void dn_bands(int H, int threads, const F& fn)
{
    threads = std::max(1, std::min(threads, H));
    if (threads == 1) { fn(0, H); return; }
    const int per = (H + threads - 1) / threads;
    std::vector<std::thread> pool;
    pool.reserve((size_t)threads);
    int y0 = 0;
    try {
        for (; y0 < H; y0 += per) pool.emplace_back([&fn, y0, per, H]() { fn(y0, std::min(H, y0 + per)); });
    } catch (...) {
        // a thread could not be started: the bands not yet handed out run here (the bands never depend on who computes them)
        for (; y0 < H; y0 += per) fn(y0, std::min(H, y0 + per));
    }
    for (std::thread& t : pool) t.join();
}

} // namespace gmupt
