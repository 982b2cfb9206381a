// Stand-alone driver of the host convergence rule (csrc/pt_converge.cpp, what gmupt_converge_host runs) for the sanitizer runs of
// tools/sanitize/run.sh: six chained updates at the ragged sizes around the run and level boundaries of the rule, with pixels that never
// get a sample, counts that stand still, drop or are all ones, and NaN / inf / 3e38 colours mixed in; with and without the error plane,
// which must not change a bit of the state or the summary.  CPU only; nothing here touches a device.
#include "../../gmu-path-tracer_amd/csrc/pt_converge.hpp"

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace gmupt;

static uint32_t g_state = 2463534242u;
static uint32_t rnd() { g_state = g_state * 1664525u + 1013904223u; return g_state >> 8; }
static float unit() { return (float)rnd() / 16777216.0f; }

int main()
{
    const size_t sizes[] = { 1, 37 * 5, 255, 256, 257, 67 * 19, 65536, 65537, 257 * 257 };
    for (size_t n : sizes) {
        std::vector<gmupt_converge_pixel> a(n), b(n);                   // value-initialised: the initial state
        std::vector<float> rgba(4 * n), err(n);
        std::vector<uint32_t> count(n, 0u);
        gmupt_converge_info info{};
        for (int u = 0; u < 6; u++) {
            for (size_t i = 0; i < n; i++) {
                for (int c = 0; c < 3; c++) rgba[4 * i + c] = unit();
                uint32_t cnt = count[i] + rnd() % 10u;                  // 0: the count stands still
                switch (rnd() % 32u) {
                case 0: rgba[4 * i] = std::numeric_limits<float>::quiet_NaN(); break;
                case 1: rgba[4 * i + 1] = std::numeric_limits<float>::infinity(); break;
                case 2: rgba[4 * i + 2] = (u & 1) ? 3e38f : -3e38f; break;
                case 3: cnt = 0xFFFFFFFFu; break;
                case 4: cnt = count[i] / 2u; break;                     // a restart
                default: break;
                }
                if (i % 11u == 0) cnt = 0;                              // never sampled
                count[i] = cnt;
                std::memcpy(&rgba[4 * i + 3], &cnt, 4);
            }
            const CvParams prm = { 0.05f, 2u + (uint32_t)(u & 1), (uint32_t)(n / 3) };
            const CvPartial with = converge_host(a.data(), rgba.data(), n, prm, err.data());
            const CvPartial without = converge_host(b.data(), rgba.data(), n, prm, nullptr);
            if (std::memcmp(&with, &without, sizeof(with)) != 0 || std::memcmp(a.data(), b.data(), n * sizeof(a[0])) != 0) {
                std::fprintf(stderr, "converge: %zu pixels, update %d: the error plane changes the result\n", n, u); return 1;
            }
            cv_fill_info(with, (uint32_t)n, prm, &info);
            if (info.known > n || info.below > info.known || info.nonfinite > info.known || info.unsampled > n) {
                std::fprintf(stderr, "converge: %zu pixels, update %d: inconsistent counts\n", n, u); return 1;
            }
        }
        std::printf("converge %zu pixels: known %u, nonfinite %u, below %u, max %.9g, sum %.17g\n", n, info.known, info.nonfinite, info.below,
                    (double)info.max_error, info.sum_error);
    }
    return 0;
}
