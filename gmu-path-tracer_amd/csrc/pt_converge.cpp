// gmupt_converge_host: the rule of include/gmupt.h ("Convergence") on host arrays, the reference of the device path (pt_converge.hip).
// The arithmetic is pt_converge.hpp, shared with the kernels.  A run of 256 entries is reduced with the strides of the rule, the
// levels above hold 1/256 of the entries each; everything runs on the calling thread.
#include "pt_converge.hpp"

#include <vector>

namespace gmupt {

// the stride halving of one run: x holds kCvRun entries, the padding included; the result is x[0]
static CvPartial cv_reduce_run(CvPartial* x)
{
    for (uint32_t s = kCvRun / 2; s > 0; s >>= 1)
        for (uint32_t i = 0; i < s; i++) cv_combine(x[i], x[i + s]);
    return x[0];
}

CvPartial converge_host(gmupt_converge_pixel* state, const float* rgba, size_t n, const CvParams& prm, float* error)
{
    std::vector<CvPartial> level(cv_runs(n));
    CvPartial x[kCvRun];
    for (size_t run = 0; run < level.size(); run++) {
        for (uint32_t i = 0; i < kCvRun; i++) {
            const size_t p = run * kCvRun + i;
            if (p >= n) { x[i] = cv_zero(); continue; }
            gmupt_converge_pixel& rec = state[p];
            CvState st = { rec.n, rec.k, rec.w, rec.s, rec.mean, rec.m2 };
            const uint32_t n1 = cv_update(st, rgba[4 * p], rgba[4 * p + 1], rgba[4 * p + 2], rgba[4 * p + 3]);
            rec.n = st.n; rec.k = st.k; rec.w = st.w; rec.pad = 0; rec.s = st.s; rec.mean = st.mean; rec.m2 = st.m2;
            const float err = cv_error(st);
            if (error) error[p] = err;
            x[i] = cv_pixel(st, n1, err, prm);
        }
        level[run] = cv_reduce_run(x);
    }
    while (level.size() > 1) {
        std::vector<CvPartial> next(cv_runs(level.size()));
        for (size_t run = 0; run < next.size(); run++) {
            for (uint32_t i = 0; i < kCvRun; i++) {
                const size_t p = run * kCvRun + i;
                x[i] = p < level.size() ? level[p] : cv_zero();
            }
            next[run] = cv_reduce_run(x);
        }
        level.swap(next);
    }
    return level[0];
}

} // namespace gmupt
