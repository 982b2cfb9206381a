// The arithmetic of the convergence monitor (include/gmupt.h "Convergence" states the rule), shared by gmupt_converge_host
// (pt_converge.cpp) and the k_cv_* kernels (pt_converge.hip): the update of one pixel's batch-mean state from its RGBA32F value, the
// pixel's error, what a pixel contributes to the summary, how two partial summaries combine and the step from the totals to the
// public fields.  One copy, so that host and device run the same statements: binary64 except where the rule says binary32, nothing
// contracted (build.py).  The ORDER in which the errors are summed -- runs of 256, stride halving, level by level, the one "Tree cost"
// states -- is the other half of the rule: pt_ordered_sum.hpp, which both callers hand cv_zero and cv_combine to.
#pragma once
#include "pt_device.hpp"
#include "detmath.hpp"
#include "pt_denoise.hpp"      // dn_luminance: the one definition of the luminance
#include "pt_ordered_sum.hpp"

namespace gmupt {

// the state of one pixel in registers (the device keeps it as planes, the host as gmupt_converge_pixel records)
struct CvState { uint32_t n, k, w; double s, mean, m2; };

struct CvParams { float threshold; uint32_t minBatches, allowPixels; };

// What a pixel, a run, or the whole image amounts to.  32 bytes: the records of the device scratch.
struct CvPartial {
    double sumError;
    uint32_t unsampled, known, nonfinite, below;
    float maxError; uint32_t pad;
};
static_assert(sizeof(CvPartial) == 32, "CvPartial layout");

GM_HD bool cv_finite(float x) { return (f2u(x) & 0x7F800000u) != 0x7F800000u; }

// "Update" of the rule, steps 1 to 4: returns n1
GM_HD uint32_t cv_update(CvState& st, float r, float g, float b, float a)
{
    const uint32_t n1 = f2u(a);
    const float y = dn_luminance(r, g, b);
    if (n1 < st.n) { st.n = 0; st.k = 0; st.w = 0; st.s = 0.0; st.mean = 0.0; st.m2 = 0.0; }
    const uint32_t bsz = n1 - st.n;
    if (bsz == 0) return n1;
    const double s1 = (double)n1 * (double)y;
    const double t = s1 - st.s;
    const double B = t / (double)bsz;
    const uint32_t w1 = st.w + bsz;
    const double d = B - st.mean;
    const double mean1 = st.mean + ((double)bsz / (double)w1) * d;
    st.m2 = st.m2 + ((double)bsz * d) * (B - mean1);
    st.mean = mean1; st.s = s1; st.n = n1; st.w = w1; st.k = st.k + 1;
    return n1;
}

// step 5: the error of the pixel, -1 while it is unknown
GM_HD float cv_error(const CvState& st)
{
    if (st.k < 2) return -1.0f;
    double v = (st.m2 / (double)(st.k - 1)) / (double)st.w;
    if (v < 0.0) v = 0.0;
    return dsqrt((float)v);
}

// the entry of one pixel in the summary; cv_zero() is the padding entry of a run
GM_HD CvPartial cv_zero() { return CvPartial{ 0.0, 0u, 0u, 0u, 0u, 0.0f, 0u }; }
GM_HD CvPartial cv_pixel(const CvState& st, uint32_t n1, float err, const CvParams& prm)
{
    CvPartial p = cv_zero();
    p.unsampled = n1 == 0 ? 1u : 0u;
    if (st.k < 2) return p;
    p.known = 1;
    if (!cv_finite(err)) { p.nonfinite = 1; return p; }
    p.sumError = (double)err; p.maxError = err;
    p.below = (st.k >= prm.minBatches && err <= prm.threshold) ? 1u : 0u;
    return p;
}

// x[i] += x[i + s] of the rule; the counts and the maximum are order-free
GM_HD void cv_combine(CvPartial& x, const CvPartial& y)
{
    x.sumError = x.sumError + y.sumError;
    x.unsampled += y.unsampled; x.known += y.known; x.nonfinite += y.nonfinite; x.below += y.below;
    x.maxError = y.maxError > x.maxError ? y.maxError : x.maxError;
}

// the public fields from the totals (ms stays as it is)
inline void cv_fill_info(const CvPartial& t, uint32_t pixels, const CvParams& prm, gmupt_converge_info* info)
{
    info->pixels = pixels; info->unsampled = t.unsampled; info->known = t.known; info->nonfinite = t.nonfinite; info->below = t.below;
    info->converged = (pixels - t.below <= prm.allowPixels) ? 1u : 0u;
    info->max_error = t.maxError; info->pad = 0;
    info->sum_error = t.sumError;
    const uint32_t m = t.known - t.nonfinite;
    info->mean_error = m ? t.sumError / (double)m : 0.0;
}

// ---- host reference (pt_converge.cpp): the rule over n >= 1 pixels; error may be null
CvPartial converge_host(gmupt_converge_pixel* state, const float* rgba, size_t n, const CvParams& prm, float* error);

// ---- device side (pt_converge.hip).  The state planes of `cap` pixels and the partials of every level are parts of one allocation.
struct CvPlanes { uint32_t* n; uint32_t* k; uint32_t* w; double* s; double* mean; double* m2; CvPartial* partials; };
size_t converge_carve(void* base, size_t cap, CvPlanes* out);    // the bytes of the allocation; base == nullptr only adds them up
size_t converge_state_bytes(size_t cap);                          // its leading bytes that hold the state (what a restart zeroes)
const CvPartial* launch_converge(const float4* rgba, size_t n, const CvPlanes& pl, const CvParams& prm, float* error, hipStream_t s);

} // namespace gmupt
