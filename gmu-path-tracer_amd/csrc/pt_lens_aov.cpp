// gmupt_aov_lens_ray: the rays of the lens-filtered AOV planes (include/gmupt_lens_aov.h) on the host, the reference of k_laov_raygen
// (pt_lens_aov.hip).  The arithmetic is pt_lens_aov.hpp, shared with the kernel.
#include "pt_lens_aov.hpp"

namespace gmupt {

void lens_aov_ray_host(const gmupt_camera_buffer& cam, const gmupt_lens& lens, uint32_t x, uint32_t y, uint32_t samples, uint32_t k, gmupt_ray* out)
{
    store_ray(lens_aov_ray(cam, lens.aperture_radius, lens.focus_distance, x, y, samples, k), out);
}

} // namespace gmupt
