// The host rule of the guided infill (gmupt_infill_host): the phases of pt_infill.hip over row bands of std::threads.  Every pixel of a
// phase reads only the previous phase's buffers, and the counts are integer sums, so neither the bands nor the thread count can change a
// bit of the result.
#include "pt_infill.hpp"
#include "pt_bands.hpp"

#include <atomic>

namespace gmupt {

// beauty / out: W*H RGBA float texels, aov: W*H 64-byte records; any alignment (copied into aligned buffers)
void infill_host(const float* beauty, const void* aov, int W, int H, const IfParams& prm, float* out, IfCounters* counts, int threads)
{
    const size_t n = (size_t)W * H;
    const std::vector<float4> in = host_words(beauty, n), rec = host_words(aov, 4 * n);
    std::vector<float4> scratch((n * kGdScratchBytes + 15) / 16), res(n);   // the device's layout, without the counters
    float4 *A, *B;
    const GdPlanes g = gd_carve(scratch.data(), 0, n, A, B);
    std::atomic<uint32_t> sources(0), holes(0), filled(0), openLeft(0);
    host_bands(H, threads, [&](int y0, int y1) {
        uint32_t ns = 0, nh = 0;
        for (size_t i = (size_t)y0 * W; i < (size_t)y1 * W; i++) {
            A[i] = if_prepare(in[i], rec[4 * i], rec[4 * i + 1], rec[4 * i + 2], rec[4 * i + 3], g, i);
            ns += if_state(A[i]) == kIfSource; nh += if_state(A[i]) == kIfOpen;
        }
        sources += ns; holes += nh;
    });
    for (int k = 0; k < prm.passes; k++) {
        const bool last = k == prm.passes - 1;
        const float4* src = (k & 1) ? B : A;
        float4* dst = last ? res.data() : ((k & 1) ? A : B);
        host_bands(H, threads, [&](int y0, int y1) {
            uint32_t nf = 0, no = 0;
            for (int y = y0; y < y1; y++) for (int x = 0; x < W; x++) {
                const size_t p = (size_t)y * W + x;
                float4 c = src[p];
                if (if_state(c) == kIfOpen) {
                    c = if_fill(src, g, W, H, x, y, 1 << k, prm);
                    if (if_state(c) == kIfFilled) nf++; else no++;
                }
                dst[p] = last ? if_output(c, in[p]) : c;
            }
            filled += nf; if (last) openLeft += no;
        });
    }
    std::memcpy(out, res.data(), n * 16);
    if (counts) { counts->sources = sources; counts->holes = holes; counts->filled = filled; counts->openLeft = openLeft; }
}

} // namespace gmupt
