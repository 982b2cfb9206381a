// Temporal reuse's per-pixel arithmetic (include/gmupt.h states it), shared by k_tp_integrate (pt_temporal.hip) and the host integration
// temporal_host (pt_temporal.cpp): one copy of the projection, the tap tests, the blend and the new record, so that both run one binary32
// sequence (build.py flags: no contraction, correctly rounded divide / sqrt, denormals kept).  No transcendental is needed.
//
// History layout: the public gmupt_history record, 48 bytes = three float4 per pixel, row-major:
//   r0  rgb, count          r1  normal xyz, material bits          r2  position xyz, valid bits
// A tap reads all three (48 B); the centre reads its beauty texel (16 B) and its AOV record (64 B) and writes 16 + 48 B.
#pragma once
#include "detmath.hpp"
#include "../../include/gmupt.h"

namespace gmupt {

constexpr uint32_t kTpTapBytes = 48;

struct TpParams { float cap, minCos, planeDist; };

// a previous camera, with the host-side products every projection shares (computed once by tp_camera, the same bits on both sides)
struct TpCam { f3 P, U, Hv, V, F; float ff, hh, vv, psx, psy; };

// the history a call integrates against: rec == nullptr means none
struct TpPrev { const float4* rec; int x0, y0, W, H; TpCam cam; };

GM_HD TpCam tp_camera(const gmupt_camera_buffer& c)
{
    TpCam t;
    t.P = mk3(c.position[0], c.position[1], c.position[2]);
    t.U = mk3(c.upperLeftCorner[0], c.upperLeftCorner[1], c.upperLeftCorner[2]);
    t.Hv = mk3(c.horizontal[0], c.horizontal[1], c.horizontal[2]);
    t.V = mk3(c.vertical[0], c.vertical[1], c.vertical[2]);
    t.F = (t.U + t.Hv * 0.5f) - t.V * 0.5f;
    t.ff = dot3(t.F, t.F); t.hh = dot3(t.Hv, t.Hv); t.vv = dot3(t.V, t.V);
    t.psx = c.pixelSize[0]; t.psy = c.pixelSize[1];
    return t;
}

// whole-frame pixel coordinates (u, v) of world point X in camera c; false when X is not in front of it (lambda not > 0)
GM_HD bool tp_project(const TpCam& c, const f3 X, float& u, float& v)
{
    const f3 d = X - c.P;
    const float lambda = dot3(d, c.F) / c.ff;
    if (!(lambda > 0.0f)) return false;
    const f3 e = mk3(d.x / lambda, d.y / lambda, d.z / lambda) - c.U;
    u = (dot3(e, c.Hv) / c.hh) / c.psx;
    v = (-dot3(e, c.V) / c.vv) / c.psy;
    return true;
}

GM_HD int tp_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// pixel p: beauty texel b and AOV record a0..a3 -> integrated texel `out` and new record r0..r2.  The four tap records are loaded
// together, at addresses clamped into the previous rectangle, before any of them is tested (a load whose tap is outside is made and
// ignored).  A projection whose taps all lie outside the previous rectangle loads nothing: no tap could count.
// MV: m is the pixel's gmupt_motion record; with flags == 1 the point that is projected and that the taps' plane test measures from is
// prev_position, where the surface point was when the history was written.  The new record keeps x_p, the current pose.
template <bool MV>
GM_HD void tp_pixel_t(const float4 b, const float4 a0, const float4 a1, const float4 a2, const float4 a3, const float4 m, const TpPrev& pv,
                      const TpParams& prm, float4& out, float4& r0, float4& r1, float4& r2)
{
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int32_t tri = (int32_t)f2u(a3.x);
    const uint32_t mat = f2u(a3.y), light = f2u(a3.z);
    const f3 nraw = mk3(a1.x, a1.y, a1.z);
    if (!(tri != -1 && light == 0u && length3(nraw) > 0.0f)) {   // not a surface pixel: the beauty texel, an empty record
        out = b; r0 = zero; r1 = zero; r2 = zero;
        return;
    }
    const f3 np = normalize3(nraw), xp = mk3(a2.x, a2.y, a2.z);
    f3 xh = xp;                                                   // the point in the history's pose
    if constexpr (MV) { if (f2u(m.w) == 1u) xh = mk3(m.x, m.y, m.z); }
    float nh = 0.0f, hr = 0.0f, hg = 0.0f, hb = 0.0f;
    float u, v;
    if (pv.rec && tp_project(pv.cam, xh, u, v)) {
        const float ul = u - (float)pv.x0, vl = v - (float)pv.y0;
        const float fu = __builtin_floorf(ul), fv = __builtin_floorf(vl);
        if (fu >= -1.0f && fu <= (float)(pv.W - 1) && fv >= -1.0f && fv <= (float)(pv.H - 1)) {
            const float fx = ul - fu, fy = vl - fv;
            const int ix = (int)fu, iy = (int)fv;
            float4 q0[4], q1[4], q2[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const size_t q = 3 * ((size_t)tp_clamp(iy + (k >> 1), pv.H - 1) * pv.W + tp_clamp(ix + (k & 1), pv.W - 1));
                q0[k] = pv.rec[q]; q1[k] = pv.rec[q + 1]; q2[k] = pv.rec[q + 2];
            }
            const float gx = 1.0f - fx, gy = 1.0f - fy;
            const float w[4] = { gx * gy, fx * gy, gx * fy, fx * fy };
            const float lim = prm.planeDist * a0.w;
            float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sn = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int qx = ix + (k & 1), qy = iy + (k >> 1);
                if (qx < 0 || qx >= pv.W || qy < 0 || qy >= pv.H) continue;
                if (f2u(q2[k].w) != 1u || !(q0[k].w > 0.0f) || f2u(q1[k].w) != mat) continue;
                if (!(dot3(np, mk3(q1[k].x, q1[k].y, q1[k].z)) >= prm.minCos)) continue;
                if (!(dabs(dot3(np, mk3(q2[k].x, q2[k].y, q2[k].z) - xh)) <= lim)) continue;
                sw = sw + w[k];
                sr = sr + w[k] * q0[k].x; sg = sg + w[k] * q0[k].y; sb = sb + w[k] * q0[k].z;
                sn = sn + w[k] * q0[k].w;
            }
            if (sw > 0.0f) {
                hr = sr / sw; hg = sg / sw; hb = sb / sw;
                nh = hmin(prm.cap, sn / sw);
            }
        }
    }
    const uint32_t n = f2u(b.w);
    const float nf = (float)n;
    float count = nf;
    if (nh == 0.0f) {
        out = b;
    } else if (n == 0u) {
        out = make_float4(hr, hg, hb, u2f((uint32_t)__builtin_ceilf(nh)));
        count = nh + nf;
    } else {
        const float den = nh + nf;
        out = make_float4(((nh * hr) + (nf * b.x)) / den, ((nh * hg) + (nf * b.y)) / den, ((nh * hb) + (nf * b.z)) / den,
                          u2f(n + (uint32_t)__builtin_ceilf(nh)));
        count = den;
    }
    r0 = make_float4(out.x, out.y, out.z, count);
    r1 = make_float4(np.x, np.y, np.z, u2f(mat));
    r2 = make_float4(xp.x, xp.y, xp.z, u2f(count > 0.0f ? 1u : 0u));
}

GM_HD void tp_pixel(const float4 b, const float4 a0, const float4 a1, const float4 a2, const float4 a3, const TpPrev& pv, const TpParams& prm,
                    float4& out, float4& r0, float4& r1, float4& r2)
{
    tp_pixel_t<false>(b, a0, a1, a2, a3, make_float4(0.0f, 0.0f, 0.0f, 0.0f), pv, prm, out, r0, r1, r2);
}

void temporal_host(const float* beauty, const void* aov, const void* motion, int W, int H, const void* prev, const gmupt_camera_buffer* prevCam, int px0, int py0,
                   int pW, int pH, const TpParams& prm, float* out, void* outHist, int threads);   // pt_temporal.cpp

} // namespace gmupt
