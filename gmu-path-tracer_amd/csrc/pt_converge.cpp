// gmupt_converge_host: the rule of include/gmupt.h ("Convergence") on host arrays, the reference of the device path (pt_converge.hip).
// The arithmetic is pt_converge.hpp, shared with the kernels; the order of the sum is pt_ordered_sum.hpp.  Everything runs on the calling
// thread: a pixel's entry is its update, so it is taken once per pixel, in ascending order.
#include "pt_converge.hpp"

namespace gmupt {

CvPartial converge_host(gmupt_converge_pixel* state, const float* rgba, size_t n, const CvParams& prm, float* error)
{
    const auto entry = [&](size_t p) {
        gmupt_converge_pixel& rec = state[p];
        CvState st = { rec.n, rec.k, rec.w, rec.s, rec.mean, rec.m2 };
        const uint32_t n1 = cv_update(st, rgba[4 * p], rgba[4 * p + 1], rgba[4 * p + 2], rgba[4 * p + 3]);
        rec.n = st.n; rec.k = st.k; rec.w = st.w; rec.pad = 0; rec.s = st.s; rec.mean = st.mean; rec.m2 = st.m2;
        const float err = cv_error(st);
        if (error) error[p] = err;
        return cv_pixel(st, n1, err, prm);
    };
    return ordered_sum_host<cv_zero, cv_combine>(n, 1, entry);
}

} // namespace gmupt
