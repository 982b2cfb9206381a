// Stand-alone driver of the host rule of the thin lens (csrc/pt_lens.cpp and pt_lens.hpp, what gmupt_lens_ray_host runs) for the sanitizer
// runs of tools/sanitize/run.sh: q = 0 .. 4095 over the pixels of a 32 x 18 frame and the corners of a 1920 x 1080 one, the largest q and
// pixel words, with every lens of tests/lens_extremes_util.py (LENS_CLASSES) -- denormal, huge and FLT_MAX apertures and focus distances,
// whose rays have zero or NaN directions by design -- and a camera whose frame vectors are degenerate.  The rule must only compute:
// never trap, never read outside its arguments; tmax = FLT_MAX, pad = 0, a finite origin for a well-formed camera, and a direction that
// is a unit vector, (0, 0, 0) or NaN.  CPU only; nothing here touches a device.
#include "../../gmu-path-tracer_amd/csrc/pt_lens.hpp"

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
    c.randomSeed[0] = 0.3172f; c.randomSeed[1] = 0.8141f;
    return c;
}

int main()
{
    const float fltMax = 3.402823466e+38f;
    const gmupt_lens lenses[] = { { 0.0f, 1.0f }, { 0.3f, 13.0f }, { 1.0e-45f, 13.0f }, { 1.0e-38f, 13.0f }, { 1.0e18f, 13.0f }, { 1.5e19f, 13.0f }, { 3.0e19f, 13.0f },
        { 1.0e30f, 13.0f }, { fltMax, 13.0f }, { 0.3f, 1.0e-45f }, { 0.3f, 1.0e-30f }, { 0.3f, 1.0e19f }, { 0.3f, 1.5e19f }, { 0.3f, 1.0e30f }, { 0.3f, 3.0e38f },
        { 0.3f, fltMax }, { 1.0e-45f, 1.0e-45f } };
    size_t rays = 0, unit = 0, zero = 0, nan = 0;
    for (int degenerate = 0; degenerate < 2; degenerate++) for (const gmupt_lens& lens : lenses) {
        for (uint32_t i = 0; i < 4096u + 6u; i++) {
            const bool big = i >= 4096u;
            const gmupt_camera_buffer cam = big ? camera(1920, 1080, degenerate != 0) : camera(32, 18, degenerate != 0);
            const uint32_t edge[][3] = { { 0, 0, 0 }, { (1u << 21) - 1u, 1919, 1079 }, { 0xFFFFFFFFu, 0, 1079 }, { 7, 1919, 0 }, { 1, 0xFFFFFFFFu, 0xFFFFFFFFu }, { 0xFFFFFFFFu, 0xFFFFFFFFu, 0 } };
            const uint32_t q = big ? edge[i - 4096u][0] : i, cx = big ? edge[i - 4096u][1] : i % 32u, cy = big ? edge[i - 4096u][2] : (i / 32u) % 18u;
            gmupt_ray ray;
            std::memset(&ray, 0xAB, sizeof(ray));
            lens_ray_host(cam, lens, q, cx, cy, &ray);
            rays++;
            if (ray.tmax != fltMax) { std::fprintf(stderr, "tmax is not FLT_MAX\n"); return 1; }
            uint32_t pad; std::memcpy(&pad, reinterpret_cast<const char*>(&ray) + 28, 4);
            if (pad != 0) { std::fprintf(stderr, "the pad word is not 0\n"); return 1; }
            if (degenerate || cx == 0xFFFFFFFFu) continue;
            const float* d = ray.direction;
            if (!std::isfinite(ray.origin[0]) || !std::isfinite(ray.origin[1]) || !std::isfinite(ray.origin[2])) { std::fprintf(stderr, "aperture %g focus %g q %u: a non-finite origin\n", (double)lens.aperture_radius, (double)lens.focus_distance, q); return 1; }
            const double len = std::sqrt((double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2]);
            if (std::isnan(d[0]) || std::isnan(d[1]) || std::isnan(d[2])) nan++;
            else if (d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f) zero++;
            else if (std::fabs(len - 1.0) < 1e-3) unit++;
            else { std::fprintf(stderr, "aperture %g focus %g q %u: direction (%g, %g, %g) is neither a unit vector, nor zero, nor NaN\n", (double)lens.aperture_radius, (double)lens.focus_distance, q, (double)d[0], (double)d[1], (double)d[2]); return 1; }
        }
    }
    if (!unit || !zero || !nan) { std::fprintf(stderr, "a kind of direction did not occur: %zu unit, %zu zero, %zu NaN\n", unit, zero, nan); return 1; }
    std::printf("lens rays: %zu computed; directions of the well-formed camera: %zu unit, %zu zero, %zu NaN\n", rays, unit, zero, nan);
    return 0;
}
