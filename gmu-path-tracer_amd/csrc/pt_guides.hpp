// What the denoiser (pt_denoise.hpp) and the guided infill (pt_infill.hpp) share: the guide planes of an image, their scratch layout, the
// prepare step's surface rule, the row of the 25-tap walk and the three guide terms of a tap's weight.  One copy, run by the kernels and the host
// rules alike, so that a change to a tap rule is made once, in one binary32 order.
//
// Guide planes (structure of arrays, one element per pixel, row-major), behind the stage's two ping-pong colour buffers (float4):
//   nw   float4  normalised normal xyz, one stage-owned word (the denoiser's luminance, infill's material bits)
//   xa   float4  position xyz, albedo r
//   ag   float2  albedo g, b
//   z    float   depth (read for the centre pixel only)
// A tap reads its colour texel (16 B), nw (16 B), xa (16 B), ag (8 B): 56 bytes, everything the weight and the sums need.
#pragma once
#include "detmath.hpp"

namespace gmupt {

constexpr float kGdLog2e = 1.44269504f;                         // exp(-d) = exp2(-d * log2(e))
constexpr uint32_t kGdScratchBytes = 2 * 16 + 16 + 16 + 8 + 4;  // per pixel: two colour buffers, nw, xa, ag, z

struct GdPlanes { float4* nw; float4* xa; float2* ag; float* z; };

// the scratch of an image of n pixels behind a head of `head` bytes (infill's counters): colour buffers A and B, then the guide planes
inline GdPlanes gd_carve(void* scratch, size_t head, size_t n, float4*& A, float4*& B)
{
    char* b = static_cast<char*>(scratch) + head;
    A = reinterpret_cast<float4*>(b); b += n * 16;
    B = reinterpret_cast<float4*>(b); b += n * 16;
    GdPlanes g;
    g.nw = reinterpret_cast<float4*>(b); b += n * 16;
    g.xa = reinterpret_cast<float4*>(b); b += n * 16;
    g.ag = reinterpret_cast<float2*>(b); b += n * 8;
    g.z = reinterpret_cast<float*>(b);
    return g;
}

// weight of a-trous tap i (-2..2): {1/16, 1/4, 3/8, 1/4, 1/16}; of the 3x3 variance Gaussian (-1..1): {1/4, 1/2, 1/4}
GM_HD float gd_h5(int i) { return i == 0 ? 0.375f : (i == 1 || i == -1) ? 0.25f : 0.0625f; }
GM_HD float gd_h3(int i) { return i == 0 ? 0.5f : 0.25f; }

GM_HD int gd_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the prepare step's guide write for pixel i from its AOV record (four float4).  A surface pixel (a triangle, no light, a normal that is
// not zero) that the caller `wants` gets its guides, with `word` next to the normalised normal; every other pixel gets four zeroed planes.
// Returns which of the two it was.  word() is evaluated for a pixel that gets its guides only.
template <class Word>
GM_HD bool gd_prepare(bool want, const float4 a0, const float4 a1, const float4 a2, const float4 a3, const Word& word, const GdPlanes& g, size_t i)
{
    const int32_t tri = (int32_t)f2u(a3.x);
    const uint32_t light = f2u(a3.z);
    const f3 nraw = mk3(a1.x, a1.y, a1.z);
    if (!(want && tri != -1 && light == 0u && length3(nraw) > 0.0f)) {
        g.nw[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); g.xa[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        g.ag[i] = make_float2(0.0f, 0.0f); g.z[i] = 0.0f;
        return false;
    }
    const f3 n = normalize3(nraw);
    g.nw[i] = make_float4(n.x, n.y, n.z, word());
    g.xa[i] = make_float4(a2.x, a2.y, a2.z, a0.x);
    g.ag[i] = make_float2(a0.y, a0.z);
    g.z[i] = a0.w;
    return true;
}

// the centre pixel's guides as a tap's weight needs them, and its stage-owned word
struct GdCentre { f3 np, xp; float word, ar, ag, ab, denX; };

GM_HD GdCentre gd_centre(const GdPlanes& g, size_t p, float sigmaPlane)
{
    const float4 nwp = g.nw[p], xap = g.xa[p];
    const float2 agp = g.ag[p];
    GdCentre c;
    c.np = mk3(nwp.x, nwp.y, nwp.z); c.xp = mk3(xap.x, xap.y, xap.z); c.word = nwp.w;
    c.ar = xap.w; c.ag = agp.x; c.ab = agp.y;
    c.denX = sigmaPlane * g.z[p];
    return c;
}

// the guide terms of tap q against centre c: the normal factor, the plane distance and the albedo distance (the order of include/gmupt.h)
GM_HD float gd_wn(const GdCentre& c, const float4 nwq, float sigmaNormal) { return dpow(hmax(0.0f, dot3(c.np, mk3(nwq.x, nwq.y, nwq.z))), sigmaNormal); }
GM_HD float gd_dxp(const GdCentre& c, const float4 xaq) { return dabs(dot3(c.np, mk3(xaq.x, xaq.y, xaq.z) - c.xp)) / c.denX; }
GM_HD float gd_da(const GdCentre& c, const float4 xaq, const float2 agq, float sigmaAlbedo) { return ((dabs(xaq.w - c.ar) + dabs(agq.x - c.ag)) + dabs(agq.y - c.ab)) / sigmaAlbedo; }

// Row j (-2..2) of the 25 taps of pixel (x, y) at step s, left to right; the walk is `for (j = -2; j <= 2; j++) gd_row5(...)`, rows top
// to bottom.  A row outside the image is skipped.  The loads of its five taps are issued together before any of them is tested, at
// addresses clamped into the image: a load whose tap is outside or does not count is made and ignored.  A tap counts when it is inside
// the image and the stage takes its colour texel (st.texel_ok) and its guide word (st.word_ok); st.tap then adds it to the sums with
// h = gd_h5 * gd_h5.  (The row loop stays with the caller and each test is one comparison: the kernels keep their instruction streams
// in this form only -- profiles/image_stage_refactor.)
template <class Stage, class Sums>
GM_HD void gd_row5(const float4* col, const GdPlanes& g, int W, int H, int x, int y, int s, int j, const Stage& st, Sums& a)
{
    const int qy = y + s * j;
    if (qy < 0 || qy >= H) return;
    const size_t row = (size_t)qy * W;
    float4 cq[5], nwq[5], xaq[5];
    float2 agq[5];
#pragma unroll
    for (int t = 0; t < 5; t++) {
        const size_t q = row + gd_clamp(x + s * (t - 2), W - 1);
        cq[t] = col[q]; nwq[t] = g.nw[q]; xaq[t] = g.xa[q]; agq[t] = g.ag[q];
    }
#pragma unroll
    for (int t = 0; t < 5; t++) {
        const int qx = x + s * (t - 2);
        if (qx < 0 || qx >= W || !st.texel_ok(cq[t]) || !st.word_ok(nwq[t])) continue;
        st.tap(a, cq[t], nwq[t], xaq[t], agq[t], gd_h5(t - 2) * gd_h5(j));
    }
}

} // namespace gmupt
