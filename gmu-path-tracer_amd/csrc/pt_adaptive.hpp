// The rule of adaptive sampling (include/gmupt_adaptive.h states it), shared by the host functions (pt_adaptive.cpp) and the
// k_ad_* kernels (pt_adaptive.hip): how many list entries a pixel's error is worth, what a pixel contributes to the summary, how two
// partial summaries combine, and which pixel the fresh camera path k goes to.  One copy, so that host and device run the same
// statements: binary32 where the rule says so, nothing contracted (build.py).  All sums are integers, exact in any order.
#pragma once
#include "pt_device.hpp"
#include "../../include/gmupt_adaptive.h"
#include "detmath.hpp"
#include "pt_converge.hpp"     // cv_finite: the monitor's test for a finite error
#include "pt_ordered_sum.hpp"  // kSumRun, sum_runs: pixels per run == threads per block, and the records of the level above

namespace gmupt {

constexpr uint32_t kAdMaxRepeat = 64;
constexpr uint64_t kAdMaxEntries = 1ull << 28;         // the largest list (1 GiB of pixel indices)
constexpr uint32_t kAdMaxLevels = 3;                   // scan levels over the run totals: 2^32 pixels are 2^24 runs, 2^16, 2^8 totals

struct AdParams { float threshold; uint32_t maxRepeat; };

// What a pixel, a run, or the whole image amounts to.  16 bytes: the records of the device scratch.
struct AdPartial { uint32_t entries, active, nonfinite, maxRep; };
static_assert(sizeof(AdPartial) == 16, "AdPartial layout");

// "Selection" of the rule: the entries of one pixel.  The monitor counts a pixel as below with `err <= threshold` (cv_pixel,
// pt_converge.hpp: `p.below = (st.k >= prm.minBatches && err <= prm.threshold)`) after the same finite test; a negative error is
// "unknown", which the monitor never counts as below, so it is asked first.
GM_HD uint32_t ad_rep(float err, const AdParams& prm)
{
    if (!cv_finite(err)) return 0u;
    if (err < 0.0f) return 1u;
    if (err <= prm.threshold) return 0u;
    const float q = err / prm.threshold;
    const float m = q * q;
    if (m >= (float)prm.maxRepeat) return prm.maxRepeat;
    const uint32_t c = (uint32_t)__builtin_ceilf(m);
    return c > 1u ? c : 1u;
}

GM_HD AdPartial ad_zero() { return AdPartial{ 0u, 0u, 0u, 0u }; }
GM_HD AdPartial ad_pixel(float err, uint32_t rep)
{
    return AdPartial{ rep, rep ? 1u : 0u, cv_finite(err) ? 0u : 1u, rep };
}
GM_HD void ad_combine(AdPartial& x, const AdPartial& y)
{
    x.entries += y.entries; x.active += y.active; x.nonfinite += y.nonfinite;
    x.maxRep = y.maxRep > x.maxRep ? y.maxRep : x.maxRep;
}

// "Where path k goes": the pixel of the w*h rectangle; count > 0
GM_HD uint32_t ad_pixel_of(const uint32_t* list, uint32_t count, uint32_t uniformEvery, uint32_t pixels, uint32_t k)
{
    if (uniformEvery != 0u && k % uniformEvery == 0u) return k % pixels;      // the reference's pixel, newPath.hlsl:33
    return list[k % count];
}

inline void ad_fill_info(const AdPartial& t, uint32_t pixels, gmupt_adaptive_info* info)
{
    info->pixels = pixels; info->active = t.active; info->entries = t.entries; info->skipped_nonfinite = t.nonfinite;
    info->max_rep = t.maxRep; info->pad = 0;
}

// ---- host reference (pt_adaptive.cpp): the selection over n >= 1 pixels.  list may be null (count only); entries beyond `capacity`
// are counted and not written
AdPartial adaptive_select_host(const float* error, size_t n, const AdParams& prm, uint32_t* list, size_t capacity);

// ---- device side (pt_adaptive.hip).  The list of `cap` entries, the run totals of every level and their scanned offsets are parts of
// one allocation.  total[0] / offset[0] have one record per run of pixels, level j + 1 one per 256 records of level j.
struct AdScratch { uint32_t* list; AdPartial* total[kAdMaxLevels + 1]; uint32_t* offset[kAdMaxLevels]; };
struct AdOffsets { const uint32_t* offset[kAdMaxLevels]; uint32_t levels; };     // what k_ad_emit adds up for its run
size_t adaptive_carve(void* base, size_t pixels, size_t cap, AdScratch* out);   // the bytes; base == nullptr only adds them up
const AdPartial* launch_adaptive_select(const float* error, size_t n, const AdParams& prm, const AdScratch& sc, size_t cap, hipStream_t s);
void launch_adaptive_retarget(const RenderParams& p, const uint32_t* list, uint32_t count, uint32_t uniformEvery, hipStream_t s);

} // namespace gmupt
