// Stand-alone driver of the host rule of the lens-filtered AOV planes (csrc/pt_lens_aov.cpp and pt_lens_aov.hpp, what gmupt_aov_lens_ray
// runs) for the sanitizer runs of tools/sanitize/run.sh: every ray of the corner and centre pixels of two frames at every sample count,
// with a closed, an open and a huge aperture, a focus of 1e-30 and of 1e30, the extreme lenses of tests/lens_extremes_util.py, and a camera whose frame vectors are degenerate (zero
// `horizontal`: the rule divides by a zero length and must still only compute, never trap or read outside its arguments).  For the
// well-formed cameras the directions must be unit vectors and the origins must lie within the aperture of the position.  CPU only;
// nothing here touches a device.
#include "../../gmu-path-tracer_amd/csrc/pt_lens_aov.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>

using namespace gmupt;

static gmupt_camera_buffer camera(uint32_t W, uint32_t H, bool degenerate)
{
    gmupt_camera_buffer c;
    std::memset(&c, 0, sizeof(c));
    const float aspect = (float)W / (float)H, halfH = 0.5f, halfW = aspect * halfH;
    c.position[0] = 1.0f; c.position[1] = 3.0f; c.position[2] = 8.0f;
    c.horizontal[0] = degenerate ? 0.0f : 2.0f * halfW;                                   // right = +x, up = +y, forward = -z
    c.vertical[1] = 2.0f * halfH;
    c.upperLeftCorner[0] = -halfW; c.upperLeftCorner[1] = halfH; c.upperLeftCorner[2] = -1.0f;
    c.pixelSize[0] = 1.0f / (float)W; c.pixelSize[1] = 1.0f / (float)H;
    return c;
}

int main()
{
    const uint32_t sizes[][2] = { { 32, 18 }, { 1920, 1080 } };
    const float fltMax = 3.402823466e+38f;
    const gmupt_lens lenses[] = { { 0.0f, 1.0f }, { 0.3f, 13.0f }, { 1.0e6f, 2.0f }, { 0.3f, 1.0e-30f }, { 0.3f, 1.0e30f },
        // the extreme lenses of tests/lens_extremes_util.py (LENS_CLASSES): zero and NaN directions, denormal offsets, origins 1e18 away
        { 1.0e-45f, 13.0f }, { 1.0e-38f, 13.0f }, { 1.0e18f, 13.0f }, { 1.5e19f, 13.0f }, { 3.0e19f, 13.0f }, { 1.0e30f, 13.0f }, { fltMax, 13.0f },
        { 0.3f, 1.0e-45f }, { 0.3f, 1.0e19f }, { 0.3f, 1.5e19f }, { 0.3f, 3.0e38f }, { 0.3f, fltMax }, { 1.0e-45f, 1.0e-45f } };
    size_t rays = 0, checked = 0;
    for (int degenerate = 0; degenerate < 2; degenerate++) for (const auto& wh : sizes) {
        const uint32_t W = wh[0], H = wh[1];
        const gmupt_camera_buffer cam = camera(W, H, degenerate != 0);
        const uint32_t px[][2] = { { 0, 0 }, { W - 1, 0 }, { 0, H - 1 }, { W - 1, H - 1 }, { W / 2, H / 2 }, { 0xFFFFFFFFu, 0xFFFFFFFFu } };
        for (const gmupt_lens& lens : lenses) for (uint32_t s = 1; s <= GMUPT_AOV_MAX_SAMPLES; s++) for (const auto& p : px) for (uint32_t k = 0; k < s * s; k++) {
            gmupt_ray ray;
            std::memset(&ray, 0xAB, sizeof(ray));
            lens_aov_ray_host(cam, lens, p[0], p[1], s, k, &ray);
            rays++;
            if (ray.tmax != 3.402823466e+38f) { std::fprintf(stderr, "tmax is not FLT_MAX\n"); return 1; }
            uint32_t pad; std::memcpy(&pad, reinterpret_cast<const char*>(&ray) + 28, 4);
            if (pad != 0) { std::fprintf(stderr, "the pad word is not 0\n"); return 1; }
            if (degenerate || p[0] == 0xFFFFFFFFu || lens.focus_distance < 1.0e-20f || lens.focus_distance > 1.0e19f || lens.aperture_radius > 1.0e19f) continue;   // (beyond: zero and NaN directions by design)
            const double len = std::sqrt((double)ray.direction[0] * ray.direction[0] + (double)ray.direction[1] * ray.direction[1] + (double)ray.direction[2] * ray.direction[2]);
            const double off = std::sqrt(std::pow((double)ray.origin[0] - cam.position[0], 2) + std::pow((double)ray.origin[1] - cam.position[1], 2) + std::pow((double)ray.origin[2] - cam.position[2], 2));
            if (!(std::fabs(len - 1.0) < 1e-5) || !(off <= (double)lens.aperture_radius * (1.0 + 1e-5)) || ray.origin[2] != cam.position[2]) {
                std::fprintf(stderr, "%ux%u s %u k %u aperture %g: |direction| %.9g, origin %g from the position\n", W, H, s, k, (double)lens.aperture_radius, len, off);
                return 1;
            }
            checked++;
        }
    }
    std::printf("lens aov rays: %zu computed, %zu checked\n", rays, checked);
    return 0;
}
