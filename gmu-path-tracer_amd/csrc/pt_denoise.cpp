// The host filter of the denoiser (gmupt_denoise_host): the phases of pt_denoise.hip over row bands of std::threads.  Every pixel of a
// phase reads only the previous phase's buffers, so neither the bands nor the thread count can change a bit of the result.
#include "pt_denoise.hpp"
#include "pt_bands.hpp"

namespace gmupt {

// beauty / out: W*H RGBA float texels, aov: W*H 64-byte records; any alignment (copied into aligned buffers)
void denoise_host(const float* beauty, const void* aov, int W, int H, const DnParams& prm, float* out, int threads)
{
    const size_t n = (size_t)W * H;
    const std::vector<float4> in = host_words(beauty, n), rec = host_words(aov, 4 * n);
    std::vector<float4> scratch((n * kGdScratchBytes + 15) / 16), res(n);   // the device's layout
    float4 *A, *B;
    const GdPlanes g = gd_carve(scratch.data(), 0, n, A, B);
    host_bands(H, threads, [&](int y0, int y1) {
        for (size_t i = (size_t)y0 * W; i < (size_t)y1 * W; i++) A[i] = dn_prepare(in[i], rec[4 * i], rec[4 * i + 1], rec[4 * i + 2], rec[4 * i + 3], g, i);
    });
    host_bands(H, threads, [&](int y0, int y1) {
        for (int y = y0; y < y1; y++) for (int x = 0; x < W; x++) {
            const size_t p = (size_t)y * W + x;
            const float4 c = A[p];
            B[p] = dn_valid(c.w) ? make_float4(c.x, c.y, c.z, dn_initial_variance(A, g.nw, W, H, x, y)) : c;
        }
    });
    for (int k = 0; k < prm.passes; k++) {
        const bool last = k == prm.passes - 1;
        const float4* src = (k & 1) ? A : B;
        float4* dst = last ? res.data() : ((k & 1) ? B : A);
        host_bands(H, threads, [&](int y0, int y1) {
            for (int y = y0; y < y1; y++) for (int x = 0; x < W; x++) {
                const size_t p = (size_t)y * W + x;
                const float4 c = src[p];
                if (!dn_valid(c.w)) { dst[p] = last ? in[p] : c; continue; }
                float4 r = dn_atrous(src, g, W, H, x, y, 1 << k, prm);
                if (last) r.w = in[p].w;
                dst[p] = r;
            }
        });
    }
    std::memcpy(out, res.data(), n * 16);
}

} // namespace gmupt
