// gmupt_lens_ray_host and the depth of gmupt_lens_focus_at: the rule of include/gmupt_lens.h on the host, the reference of the device
// path (pt_lens.hip).  The arithmetic is pt_lens.hpp, shared with the kernel.
#include "pt_lens.hpp"

namespace gmupt {

void lens_ray_host(const gmupt_camera_buffer& cam, const gmupt_lens& lens, uint32_t q, uint32_t cx, uint32_t cy, gmupt_ray* out)
{
    store_ray(lens_ray(cam, lens.aperture_radius, lens.focus_distance, q, cx, cy), out);
}

float lens_focus_depth(const gmupt_camera_buffer& cam, const float dir[3], float t)
{
    const f3 ulc = mk3(cam.upperLeftCorner[0], cam.upperLeftCorner[1], cam.upperLeftCorner[2]);
    const f3 hor = mk3(cam.horizontal[0], cam.horizontal[1], cam.horizontal[2]);
    const f3 ver = mk3(cam.vertical[0], cam.vertical[1], cam.vertical[2]);
    const f3 fn = normalize3((ulc + hor * 0.5f) - ver * 0.5f);      // step 3 of the rule
    return t * dot3(mk3(dir[0], dir[1], dir[2]), fn);
}

} // namespace gmupt
