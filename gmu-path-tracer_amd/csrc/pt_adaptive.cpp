// gmupt_adaptive_select_host: the selection of include/gmupt_adaptive.h on host arrays, the reference of the device path
// (pt_adaptive.hip).  The arithmetic is pt_adaptive.hpp, shared with the kernels; the sums are integers, so the pixels are simply walked
// in ascending order on the calling thread.
#include "pt_adaptive.hpp"

namespace gmupt {

AdPartial adaptive_select_host(const float* error, size_t n, const AdParams& prm, uint32_t* list, size_t capacity)
{
    AdPartial total = ad_zero();
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t rep = ad_rep(error[i], prm);
        ad_combine(total, ad_pixel(error[i], rep));
        for (uint32_t j = 0; j < rep; j++, at++) if (list && at < capacity) list[at] = (uint32_t)i;
    }
    return total;
}

} // namespace gmupt
