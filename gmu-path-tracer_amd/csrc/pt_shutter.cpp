// gmupt_shutter_ray_host, _camera_host and _time_host: the rule of include/gmupt_shutter.h on the host, the reference of the device path
// (pt_shutter.hip).  The arithmetic is pt_shutter.hpp, shared with the kernel.
#include "pt_shutter.hpp"

#include <cmath>

namespace gmupt {

const char* shutter_fault(const gmupt_shutter& sh)
{
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(sh.position[k]) || !std::isfinite(sh.upperLeftCorner[k]) || !std::isfinite(sh.horizontal[k]) || !std::isfinite(sh.vertical[k]))
            return "every component of the close pose must be finite";
    return nullptr;
}

void shutter_ray_host(const gmupt_camera_buffer& cam, const gmupt_shutter& sh, const gmupt_lens* lens, const gmupt_projection* proj, uint32_t q, uint32_t cx,
                      uint32_t cy, gmupt_ray* out)
{
    if (lens) store_ray(shutter_ray(cam, sh, ShutterLens{ lens->aperture_radius, lens->focus_distance }, q, cx, cy), out);
    else if (proj) store_ray(shutter_ray(cam, sh, ShutterProjection{ *proj }, q, cx, cy), out);
    else store_ray(shutter_ray(cam, sh, ShutterPinhole{}, q, cx, cy), out);
}

float shutter_time_host(const gmupt_camera_buffer& cam, uint32_t q) { return shutter_time(cam, q); }

void shutter_camera_host(const gmupt_camera_buffer& cam, const gmupt_shutter& sh, float t, gmupt_camera_buffer* out) { *out = shutter_camera(cam, sh, t); }

} // namespace gmupt
