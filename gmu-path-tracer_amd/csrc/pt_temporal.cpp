// The host integration of temporal reuse (gmupt_temporal_integrate_host, gmupt_temporal_integrate_motion_host): k_tp_integrate's pixel rule
// (pt_temporal.hpp) over row bands of std::threads.  Every pixel reads only the inputs, so the bands cannot change a bit.
#include "pt_temporal.hpp"
#include "pt_bands.hpp"

namespace gmupt {

// beauty / out: W*H RGBA float texels, aov: W*H 64-byte records, prev / outHist: 48-byte records, motion: W*H 16-byte records or nullptr;
// any alignment (copied into aligned buffers)
void temporal_host(const float* beauty, const void* aov, const void* motion, int W, int H, const void* prev, const gmupt_camera_buffer* prevCam, int px0, int py0,
                   int pW, int pH, const TpParams& prm, float* out, void* outHist, int threads)
{
    const size_t n = (size_t)W * H;
    const std::vector<float4> in = host_words(beauty, n), rec = host_words(aov, 4 * n), old = host_words(prev, 3 * (size_t)pW * pH), mv = host_words(motion, n);
    std::vector<float4> res(n), hist(3 * n);
    TpPrev pv{};
    if (prev) { pv.rec = old.data(); pv.x0 = px0; pv.y0 = py0; pv.W = pW; pv.H = pH; pv.cam = tp_camera(*prevCam); }
    host_bands(H, threads, [&](int y0, int y1) {
        for (size_t i = (size_t)y0 * W; i < (size_t)y1 * W; i++)
            if (motion) tp_pixel_t<true>(in[i], rec[4 * i], rec[4 * i + 1], rec[4 * i + 2], rec[4 * i + 3], mv[i], pv, prm, res[i], hist[3 * i], hist[3 * i + 1], hist[3 * i + 2]);
            else tp_pixel(in[i], rec[4 * i], rec[4 * i + 1], rec[4 * i + 2], rec[4 * i + 3], pv, prm, res[i], hist[3 * i], hist[3 * i + 1], hist[3 * i + 2]);
    });
    std::memcpy(out, res.data(), n * 16);
    std::memcpy(outHist, hist.data(), n * 48);
}

} // namespace gmupt
