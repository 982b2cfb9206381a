// The camera projections on the host (include/gmupt_projection.h): the argument checks and the inverse in binary64.  The rule itself, the
// reference of the device path (pt_projection.hip), is pt_projection.hpp, shared with the kernels and stored by store_ray.
#include "pt_projection.hpp"

#include <cmath>

namespace gmupt {

const char* projection_fault(const gmupt_projection& proj)
{
    switch (proj.kind) {
    case GMUPT_PROJ_PINHOLE: case GMUPT_PROJ_EQUIRECT: return nullptr;
    case GMUPT_PROJ_ORTHOGRAPHIC: return (std::isfinite(proj.extent) && proj.extent > 0.0f) ? nullptr : "extent must be finite and > 0";
    case GMUPT_PROJ_FISHEYE: return (std::isfinite(proj.fov) && proj.fov > 0.0f && proj.fov <= 6.28318548f) ? nullptr : "fov must be in (0, 2 pi]";
    default: return "unknown kind";
    }
}

bool projection_project(const gmupt_camera_buffer& cam, const gmupt_projection& proj, const float world[3], double* px, double* py)
{
    auto norm = [](const double v[3]) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
    auto dot = [](const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    double right[3], up[3], fwd[3], fn[3], rel[3];
    for (int k = 0; k < 3; k++) {
        right[k] = cam.horizontal[k]; up[k] = cam.vertical[k];
        fwd[k] = ((double)cam.upperLeftCorner[k] + 0.5 * cam.horizontal[k]) - 0.5 * cam.vertical[k];
        rel[k] = (double)world[k] - cam.position[k];
    }
    const double lh = norm(right), lv = norm(up), lf = norm(fwd);
    for (int k = 0; k < 3; k++) { right[k] /= lh; up[k] /= lv; fn[k] = fwd[k] / lf; }
    const double x = dot(rel, right), y = dot(rel, up), z = dot(rel, fn);
    const double Wf = 1.0 / (double)cam.pixelSize[0], Hf = 1.0 / (double)cam.pixelSize[1];
    double sx, sy;
    switch (proj.kind) {
    case GMUPT_PROJ_PINHOLE: {
        // rel * (lf / z) = fwd + hor*(u - 0.5) - ver*(v - 0.5): exact for the reference's frame, where fwd, hor and ver are orthogonal
        if (!(z > 0.0)) return false;
        sx = 2.0 * (x * (lf / z) / lh); sy = 2.0 * (y * (lf / z) / lv);
        break;
    }
    case GMUPT_PROJ_ORTHOGRAPHIC: {
        if (!(z > 0.0)) return false;
        const double halfH = (double)proj.extent * 0.5, halfW = halfH * (Wf / Hf);
        sx = x / halfW; sy = y / halfH;
        break;
    }
    case GMUPT_PROJ_FISHEYE: {
        const double len = norm(rel);
        if (!(len > 0.0)) return false;
        const double theta = std::atan2(std::sqrt(x * x + y * y), z);
        const double r = theta / ((double)proj.fov * 0.5);
        if (r > 1.0) return false;
        const double phi = std::atan2(y, x), m = Wf < Hf ? Wf : Hf;
        sx = r * std::cos(phi) / (Wf / m); sy = r * std::sin(phi) / (Hf / m);
        break;
    }
    default: {
        const double len = norm(rel);
        if (!(len > 0.0)) return false;
        sx = std::atan2(x, z) / 3.14159274101257324; sy = std::asin(y / len) / 1.57079637050628662;   // the rule's binary32 constants
        break;
    }
    }
    *px = (sx + 1.0) * 0.5 * Wf;
    *py = (1.0 - sy) * 0.5 * Hf;
    return true;
}

} // namespace gmupt
