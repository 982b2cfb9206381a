// Stand-alone driver of the image stages' host rules (csrc/pt_denoise.cpp, pt_infill.cpp, pt_temporal.cpp) for the sanitizer runs of
// tools/sanitize/run.sh: seeded synthetic frames of 1x1, 5x40 and 37x23 pixels -- a plane seen by a pinhole camera, with misses, lights,
// zero normals, pixels without samples, two materials and NaN / inf colours mixed in -- through denoise_host, infill_host and
// temporal_host (without a previous record set, and against the frame's own records with and without a motion plane), at 1 and 8
// threads, which must agree in every byte.  The arrays are handed over 4-byte aligned only, as a caller may.  CPU only; nothing here
// touches a device.
#include "../../gmu-path-tracer_amd/csrc/pt_denoise.hpp"
#include "../../gmu-path-tracer_amd/csrc/pt_infill.hpp"
#include "../../gmu-path-tracer_amd/csrc/pt_temporal.hpp"

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace gmupt;

static uint32_t g_state = 88172645u;
static uint32_t rnd() { g_state = g_state * 1664525u + 1013904223u; return g_state >> 8; }
static float unit() { return (float)rnd() / 16777216.0f; }

// n bytes of `src` at an address that is 4 past a multiple of 16: aligned for a float, not for a float4
struct Odd {
    std::vector<char> mem;
    Odd(const void* src, size_t n) : mem(n + 20) { if (src) std::memcpy(data(), src, n); }
    char* data() { return mem.data() + (20 - (uintptr_t)mem.data() % 16) % 16; }
};

static bool same(const std::vector<char>& a, const std::vector<char>& b, const char* what, int W, int H)
{
    if (a == b) return true;
    std::fprintf(stderr, "image: %s at %dx%d: 8 threads differ from 1\n", what, W, H);
    return false;
}

int main()
{
    const int sizes[3][2] = { { 1, 1 }, { 5, 40 }, { 37, 23 } };
    for (const auto& wh : sizes) {
        const int W = wh[0], H = wh[1];
        const size_t n = (size_t)W * H;
        std::vector<float> beauty(4 * n);
        std::vector<gmupt_aov> aov(n);
        std::vector<gmupt_motion> motion(n);
        for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
            const size_t i = (size_t)y * W + x;
            gmupt_aov& a = aov[i];
            std::memset(&a, 0, sizeof(a));
            const float z = 4.0f + unit();
            a.depth = z;
            a.position[0] = (((float)x + 0.5f) / (float)W - 0.5f) * z; a.position[1] = (0.5f - ((float)y + 0.5f) / (float)H) * z; a.position[2] = z;
            a.normal[0] = 0.1f * unit(); a.normal[1] = 0.1f * unit(); a.normal[2] = -1.0f;
            for (int c = 0; c < 3; c++) { a.albedo[c] = 0.5f + 0.1f * unit(); beauty[4 * i + c] = unit(); }
            a.triangle = (int32_t)(rnd() % 100u); a.material = x < W / 2 ? 1u : 2u;
            uint32_t count = 1u + rnd() % 8u;
            switch (rnd() % 16u) {
            case 0: a.triangle = -1; break;                                             // a miss
            case 1: a.light = 1u; break;
            case 2: a.normal[0] = a.normal[1] = a.normal[2] = 0.0f; break;
            case 3: case 4: case 5: count = 0u; break;                                  // a hole
            case 6: beauty[4 * i] = std::numeric_limits<float>::quiet_NaN(); break;
            case 7: beauty[4 * i + 1] = std::numeric_limits<float>::infinity(); break;
            default: break;
            }
            std::memcpy(&beauty[4 * i + 3], &count, 4);
            for (int c = 0; c < 3; c++) motion[i].prev_position[c] = a.position[c] + 0.01f * (unit() - 0.5f);
            motion[i].flags = rnd() % 4u ? 1u : 0u;
        }
        gmupt_camera_buffer cam;
        std::memset(&cam, 0, sizeof(cam));
        cam.upperLeftCorner[0] = -0.5f; cam.upperLeftCorner[1] = 0.5f; cam.upperLeftCorner[2] = 1.0f;
        cam.horizontal[0] = 1.0f; cam.vertical[1] = 1.0f;
        cam.pixelSize[0] = 1.0f / (float)W; cam.pixelSize[1] = 1.0f / (float)H;
        Odd b(beauty.data(), n * 16), a(aov.data(), n * 64), m(motion.data(), n * 16);
        const DnParams dn = { 5, 4.0f, 128.0f, 0.02f, 0.1f };
        const IfParams inf = { 6, 32.0f, 0.02f, 0.1f };
        const TpParams tp = { 32.0f, 0.9f, 0.02f };

        std::vector<char> ref[5];                           // denoise | infill | temporal: no history | history | history + motion
        IfCounters counts1{};
        for (int threads : { 1, 8 }) {
            std::vector<char> got[5];
            Odd o(nullptr, n * 16), h(nullptr, n * 48);
            denoise_host(reinterpret_cast<const float*>(b.data()), a.data(), W, H, dn, reinterpret_cast<float*>(o.data()), threads);
            got[0].assign(o.data(), o.data() + n * 16);
            IfCounters counts{};
            infill_host(reinterpret_cast<const float*>(b.data()), a.data(), W, H, inf, reinterpret_cast<float*>(o.data()), &counts, threads);
            got[1].assign(o.data(), o.data() + n * 16);
            got[1].insert(got[1].end(), reinterpret_cast<char*>(&counts), reinterpret_cast<char*>(&counts) + sizeof(counts));
            if (threads == 1) counts1 = counts;
            temporal_host(reinterpret_cast<const float*>(b.data()), a.data(), nullptr, W, H, nullptr, nullptr, 0, 0, 0, 0, tp, reinterpret_cast<float*>(o.data()),
                          h.data(), threads);
            got[2].assign(o.data(), o.data() + n * 16);
            got[2].insert(got[2].end(), h.data(), h.data() + n * 48);
            Odd prev(h.data(), n * 48);                     // this frame's records as the history of the next: the taps find records
            for (int mv = 0; mv < 2; mv++) {
                temporal_host(reinterpret_cast<const float*>(b.data()), a.data(), mv ? m.data() : nullptr, W, H, prev.data(), &cam, 0, 0, W, H, tp,
                              reinterpret_cast<float*>(o.data()), h.data(), threads);
                got[3 + mv].assign(o.data(), o.data() + n * 16);
                got[3 + mv].insert(got[3 + mv].end(), h.data(), h.data() + n * 48);
            }
            const char* names[5] = { "denoise_host", "infill_host", "temporal_host", "temporal_host with a history", "temporal_host with a history and motion" };
            for (int k = 0; k < 5; k++) {
                if (threads == 1) ref[k] = got[k];
                else if (!same(ref[k], got[k], names[k], W, H)) return 1;
            }
        }
        if (n > 1 && (ref[3] == ref[2] || ref[4] == ref[3])) { std::fprintf(stderr, "image: %dx%d: the history or the motion plane reached no pixel\n", W, H); return 1; }
        std::printf("image %dx%d: %u sources, %u holes, %u filled, %u left open\n", W, H, counts1.sources, counts1.holes, counts1.filled, counts1.openLeft);
    }
    return 0;
}
