// Adaptive sampling on the device (include/gmupt_adaptive.h states the rule; pt_adaptive.hpp is its arithmetic).  No atomics,
// no fences, no block waiting for another: a level is a launch, and the stream orders the launches.
//   k_ad_count     one thread per pixel, one block per run of 256: the pixel's entries (ad_rep) and its summary entry, reduced over
//                  the block; one 16-byte total per run.  Reads 4 bytes per pixel.
//   k_ad_scan      one thread per total of a level, one block per 256 of them: the exclusive prefix of `entries` inside the block (one
//                  4-byte offset per total) and the block's combined total, the record of the level above.  Launched level by level
//                  until one total is left: at most three launches (2^24 runs, 2^16, 2^8).  Nothing is added back down: a run's
//                  position in the list is the sum of one offset per level, which k_ad_emit adds up itself.
//   k_ad_emit      one thread per pixel again: the pixel's entries are written at (offset of the run) + (rank inside the run), the rank
//                  being the entries of the earlier waves of the block (LDS) plus those of the lower lanes of the wave.  The entries of
//                  a lane are at most 64, seven bits: the lane prefix is seven ballots, each ranked by prefix_rank as k_material ranks its
//                  classes.  Store j of a wave writes the j-th entry of every lane that has one: the addresses ascend with the lane, a
//                  wave covers one contiguous range of the list in at most 64 such stores.
//   k_ad_retarget  between k_material and the ray cast: one thread per entry of the new-path queue.  Re-aims the fresh camera path at
//                  the pixel the plan gives it: F_SCR_X, F_SCR_Y and F_RAY_DX..DZ, nothing else; the jitter is the one stage_new_path
//                  drew: its lines for newPath.hlsl:27,36-39 are restated here (the same seed, the same two draws, the same
//                  expressions).  Sharing them through a header changed k_material's register allocation, so they are not shared.
// Every index is checked against its count: a thread beyond it holds the padding entry and stores nothing.
#include "pt_adaptive.hpp"
#include "pt_kernel_util.hpp"
#include "pt_scratch.hpp"
#include "pt_launch.hpp"

namespace gmupt {

static_assert(kSumRun == 256 && kSumRun == (uint32_t)kBlock, "the block steps below are written for four waves of 64");

__device__ __forceinline__ AdPartial ad_shfl_down(const AdPartial& v, int s)
{
    AdPartial o;
    o.entries = (uint32_t)__shfl_down((int)v.entries, s, 64); o.active = (uint32_t)__shfl_down((int)v.active, s, 64);
    o.nonfinite = (uint32_t)__shfl_down((int)v.nonfinite, s, 64); o.maxRep = (uint32_t)__shfl_down((int)v.maxRep, s, 64);
    return o;
}

// the combination of the block's 256 entries, in thread 0
__device__ __forceinline__ AdPartial ad_block_reduce(AdPartial v)
{
    __shared__ AdPartial sh[kSumRun / 64];
    for (int s = 32; s > 0; s >>= 1) ad_combine(v, ad_shfl_down(v, s));
    if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) for (uint32_t w = 1; w < kSumRun / 64; w++) ad_combine(v, sh[w]);
    return v;
}

__global__ __launch_bounds__(kSumRun) void k_ad_count(const float* __restrict__ error, size_t n, AdParams prm, AdPartial* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * kSumRun + threadIdx.x;
    AdPartial v = ad_zero();
    if (i < n) { const float e = error[i]; v = ad_pixel(e, ad_rep(e, prm)); }
    v = ad_block_reduce(v);
    if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// the sum of x over the lower lanes of the wave and, in *waveTotal, over all of them; x < 2^bits
__device__ __forceinline__ uint32_t ad_lane_prefix(uint32_t x, int bits, uint32_t* waveTotal)
{
    uint32_t pre = 0, tot = 0;
    for (int b = 0; b < bits; b++) {
        const unsigned long long m = __ballot((x >> b) & 1u);
        pre += prefix_rank(m) << b; tot += (uint32_t)__popcll(m) << b;
    }
    *waveTotal = tot;
    return pre;
}

// the sum of x over the lower threads of the block (x < 2^bits); every thread of the block calls it
__device__ __forceinline__ uint32_t ad_block_prefix(uint32_t x, int bits)
{
    __shared__ uint32_t s_wave[kSumRun / 64];
    uint32_t tot;
    uint32_t pre = ad_lane_prefix(x, bits, &tot);
    if ((threadIdx.x & 63u) == 0u) s_wave[threadIdx.x >> 6] = tot;
    __syncthreads();
    for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) pre += s_wave[w];
    return pre;
}

__global__ __launch_bounds__(kSumRun) void k_ad_scan(const AdPartial* __restrict__ in, size_t n, uint32_t* __restrict__ offset, AdPartial* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * kSumRun + threadIdx.x;
    AdPartial v = ad_zero();
    if (i < n) v = in[i];
    const uint32_t pre = ad_block_prefix(v.entries, 29);        // a total is at most kAdMaxEntries = 2^28
    if (i < n) offset[i] = pre;
    v = ad_block_reduce(v);
    if (threadIdx.x == 0) out[blockIdx.x] = v;
}

__global__ __launch_bounds__(kSumRun) void k_ad_emit(const float* __restrict__ error, size_t n, AdParams prm, AdOffsets off, uint32_t* __restrict__ list, size_t cap)
{
    const size_t i = (size_t)blockIdx.x * kSumRun + threadIdx.x;
    const uint32_t rep = i < n ? ad_rep(error[i], prm) : 0u;
    size_t at = ad_block_prefix(rep, 7);                         // rep <= kAdMaxRepeat = 64
    size_t run = blockIdx.x;
    for (uint32_t l = 0; l < off.levels; l++) { at += off.offset[l][run]; run >>= 8; }
    for (uint32_t j = 0; j < rep; j++) if (at + j < cap) list[at + j] = (uint32_t)i;
}

__global__ __launch_bounds__(kBlock) void k_ad_retarget(RenderParams p, const uint32_t* __restrict__ list, uint32_t count, uint32_t uniformEvery)
{
    const uint32_t queueIndex = blockIdx.x * kBlock + threadIdx.x;
    uint32_t index, lastPath;
    if (count == 0u || !fresh_path_slot(p, queueIndex, index, lastPath)) return;   // an empty plan re-aims nothing
    const uint32_t w = p.tileEnabled ? p.fbW : cam_width(p.cam), h = p.tileEnabled ? p.fbH : cam_height(p.cam);
    const uint32_t k = lastPath + queueIndex;
    // one rectangle for both cases: w x h as stage_new_path has it (run_iteration has checked the plan against it)
    const uint32_t pix = (uniformEvery != 0u && k % uniformEvery == 0u) ? k % (w * h) : list[k % count];   // :33, or the plan's pixel
    if (pix >= w * h) return;
    const uint32_t cx = (p.tileEnabled ? p.tileX0 : 0u) + pix % w, cy = (p.tileEnabled ? p.tileY0 : 0u) + pix / w; // :34
    // stage_new_path (pt_kernels.hip) restated statement by statement
    Rng g; g.seed(queueIndex, p.cam.randomSeed[0], p.cam.randomSeed[1]);   // :27
    const float jx = g.next() * 2.0f - 1.0f;                                 // :36
    const float jy = g.next() * 2.0f - 1.0f;
    const float u = ((float)cx + jx) * p.cam.pixelSize[0];                   // :37
    const float v = ((float)cy + jy) * p.cam.pixelSize[1];
    const f3 ulc = mk3(p.cam.upperLeftCorner[0], p.cam.upperLeftCorner[1], p.cam.upperLeftCorner[2]);
    const f3 hor = mk3(p.cam.horizontal[0], p.cam.horizontal[1], p.cam.horizontal[2]);
    const f3 ver = mk3(p.cam.vertical[0], p.cam.vertical[1], p.cam.vertical[2]);
    const f3 dir = normalize3((ulc + hor * u) - ver * v);                    // :39
    st3(p, F_RAY_DX, index, dir);                                         // :42
    stu(p, F_SCR_X, index, cx); stu(p, F_SCR_Y, index, cy);                  // :43
}

// ---- host side (gmupt_capi_adaptive.hip) ----

// the parts of the allocation: the list of `cap` entries, then per level the totals and the offsets
size_t adaptive_carve(void* base, size_t pixels, size_t cap, AdScratch* out)
{
    Scratch sc(base);
    AdScratch a{};
    a.list = sc.take<uint32_t>(cap);
    size_t m = sum_runs(pixels);
    for (uint32_t l = 0; ; l++) {
        a.total[l] = sc.take<AdPartial>(m);
        if (l == kAdMaxLevels) break;
        a.offset[l] = sc.take<uint32_t>(m);
        m = sum_runs(m);
    }
    if (out) *out = a;
    return sc.used;
}

// enqueues count, the scan levels and emit; returns where the total of the image will be
const AdPartial* launch_adaptive_select(const float* error, size_t n, const AdParams& prm, const AdScratch& sc, size_t cap, hipStream_t s)
{
    size_t m = sum_runs(n);
    const uint32_t runs = (uint32_t)m;
    hipLaunchKernelGGL(k_ad_count, dim3(runs), dim3(kSumRun), 0, s, error, n, prm, sc.total[0]);
    AdOffsets off{};
    do {
        const size_t next = sum_runs(m);
        hipLaunchKernelGGL(k_ad_scan, dim3((uint32_t)next), dim3(kSumRun), 0, s, (const AdPartial*)sc.total[off.levels], m, sc.offset[off.levels], sc.total[off.levels + 1]);
        off.offset[off.levels] = sc.offset[off.levels];
        off.levels++; m = next;
    } while (m > 1);
    hipLaunchKernelGGL(k_ad_emit, dim3(runs), dim3(kSumRun), 0, s, error, n, prm, off, sc.list, cap);
    return sc.total[off.levels];
}

void launch_adaptive_retarget(const RenderParams& p, const uint32_t* list, uint32_t count, uint32_t uniformEvery, hipStream_t s)
{
    hipLaunchKernelGGL(k_ad_retarget, dim3(p.nBlocks), dim3(kBlock), 0, s, p, list, count, uniformEvery);
}

} // namespace gmupt
