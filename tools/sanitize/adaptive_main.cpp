// Stand-alone driver of the host rules of adaptive sampling (csrc/pt_adaptive.cpp and pt_adaptive.hpp, what gmupt_adaptive_select_host and
// gmupt_adaptive_pixel_host run) for the sanitizer runs of tools/sanitize/run.sh: the selection at the ragged sizes around the run and
// level boundaries, with unknown, zero, non-finite, huge and denormal errors mixed in, into a list of exactly the counted size, into
// one that is too small, and without a list; then the mapping across the wrap of k.  CPU only; nothing here touches a device.
#include "../../gmu-path-tracer_amd/csrc/pt_adaptive.hpp"

#include <cstdio>
#include <limits>
#include <vector>

using namespace gmupt;

static uint32_t g_state = 2463534242u;
static uint32_t rnd() { g_state = g_state * 1664525u + 1013904223u; return g_state >> 8; }
static float unit() { return (float)rnd() / 16777216.0f; }

int main()
{
    const size_t sizes[] = { 1, 255, 256, 257, 67 * 19, 65536, 65537, 257 * 257 };
    const uint32_t repeats[] = { 1u, 3u, 64u };
    const float T = 0.0078125f;
    for (size_t n : sizes) for (uint32_t mr : repeats) {
        std::vector<float> err(n);
        for (size_t i = 0; i < n; i++) {
            err[i] = unit() * unit() * 12.0f * T;
            switch (rnd() % 24u) {
            case 0: err[i] = std::numeric_limits<float>::quiet_NaN(); break;
            case 1: err[i] = std::numeric_limits<float>::infinity(); break;
            case 2: err[i] = -std::numeric_limits<float>::infinity(); break;
            case 3: err[i] = 3e38f; break;
            case 4: err[i] = -1.0f; break;
            case 5: err[i] = 1e-40f; break;
            case 6: err[i] = T; break;
            case 7: err[i] = 8.0f * T; break;
            default: break;
            }
        }
        const AdParams prm = { T, mr };
        const AdPartial counted = adaptive_select_host(err.data(), n, prm, nullptr, 0);
        std::vector<uint32_t> list(counted.entries), small(counted.entries / 2);
        const AdPartial full = adaptive_select_host(err.data(), n, prm, list.data(), list.size());
        const AdPartial half = adaptive_select_host(err.data(), n, prm, small.data(), small.size());
        if (full.entries != counted.entries || half.entries != counted.entries || counted.maxRep > mr || counted.active > n) {
            std::fprintf(stderr, "adaptive: %zu pixels, max_repeat %u: inconsistent counts\n", n, mr); return 1;
        }
        for (size_t j = 0; j < list.size(); j++)
            if (list[j] >= n || (j && list[j] < list[j - 1]) || (j < small.size() && small[j] != list[j])) {
                std::fprintf(stderr, "adaptive: %zu pixels, max_repeat %u: entry %zu out of order or range\n", n, mr, j); return 1;
            }
        if (!list.empty()) {
            const uint32_t ks[] = { 0u, 1u, 0xFFFFFFFEu, 0xFFFFFFFFu, rnd(), rnd() << 8 };
            for (uint32_t every : { 0u, 1u, 7u }) for (uint32_t k : ks)
                if (ad_pixel_of(list.data(), (uint32_t)list.size(), every, (uint32_t)n, k) >= n) {
                    std::fprintf(stderr, "adaptive: %zu pixels: path %u goes outside\n", n, k); return 1;
                }
        }
        std::printf("adaptive %zu pixels, max_repeat %u: active %u, entries %u, nonfinite %u, max_rep %u\n", n, mr, counted.active, counted.entries,
                    counted.nonfinite, counted.maxRep);
    }
    return 0;
}
