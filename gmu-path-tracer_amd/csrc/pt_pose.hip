// The pose stage on the device (gmupt_pose_*; include/gmupt.h "Pose" states the rule): linear-blend skinning and dense morph targets
// from a handle's own copy of the rig into the vertex buffer the renderer is bound to.  No float atomics; a vertex depends on no other.
//
// create, once per rig (one enqueue):
//   k_ps_pack    one thread per vertex: the caller's arrays (vertex-major) into the handle's planes (pt_pose.hpp: PsLayout), and rule 4 --
//                a joint number >= num_joints on a weight that is not zero sets a flag bit that create reads back
// update, per pose: two launches behind the copies of the matrices and target weights
//   k_ps_active  one block: the targets whose weight is not zero, ascending, with their weights, and their count.  A prologue on the
//                device so that host and device pointers take the same path and neither waits for the host
//   k_ps_pose    one thread per vertex, a block walks tiles of 256 vertices.  Every load is one element of a plane per lane in lane order
//                (whole 256-byte rows per wave; 128 for the joint numbers); only the planes of ACTIVE targets are touched, the list is
//                wave-uniform.  The joint matrices sit in LDS when there are at most kPsLdsJoints of them (filled once per block, which
//                is why a block walks several tiles), else they are gathered from global memory: the same statements either way.  The
//                result has a 12-byte stride in the renderer's buffer: a tile's 768 words go through LDS and leave as three stores per
//                thread of consecutive dwords in lane order.
// The rig is the handle's own copy, validated by create, and update refuses another vertex count: k_ps_pose follows the joint numbers of
// the influences it uses without a further check (an influence of weight zero is never followed).  All arithmetic is pt_pose.hpp, which
// gmupt_pose_host runs too.
#include "pt_pose.hpp"
#include "pt_launch.hpp"
#include "pt_scratch.hpp"

#include <algorithm>

namespace gmupt {

constexpr int kPsBlock = 256;
// blocks of k_ps_pose: 8 per CU; beyond that a block walks further tiles.  A first choice, like kPsLdsJoints (pt_pose.hpp): the kernel has
// been measured at these values only (DESIGN.md "Pose"), neither has been varied
constexpr uint32_t kPsMaxGrid = 2048;

__global__ __launch_bounds__(kPsBlock) void k_ps_pack(PsArgs a)
{
    const size_t v = (size_t)blockIdx.x * kPsBlock + threadIdx.x;
    if (v >= a.numVerts) return;
    const size_t S = a.stride, V = a.numVerts;
    for (int c = 0; c < 3; c++) a.rest[c * S + v] = a.srcRest[3 * v + c];
    if (a.numJoints) {
        const uint32_t K = a.influences;
        bool bad = false;
        for (uint32_t k = 0; k < K; k++) {
            const float w = a.srcWeights[v * K + k];
            const uint16_t j = a.srcJoints[v * K + k];
            bad = bad || (w != 0.0f && j >= a.numJoints);
            a.weights[k * S + v] = w;
            a.joints[k * S + v] = j;
        }
        if (bad) atomicOr(a.words, kPsFlagBadJoint);
    }
    for (size_t t = 0; t < a.numTargets; t++)
        for (int c = 0; c < 3; c++) a.deltas[(3 * t + c) * S + v] = a.srcDeltas[3 * (t * V + v) + c];
}

// at most kPsMaxTargets = kPsBlock targets: one thread each, positions by ballot within a wave and a four-entry sum across them
__global__ __launch_bounds__(kPsBlock) void k_ps_active(PsArgs a)
{
    __shared__ uint32_t waveCount[kPsBlock / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const float w = t < a.numTargets ? a.targetWeights[t] : 0.0f;
    const bool on = w != 0.0f;                       // a NaN weight is active
    const unsigned long long mask = __ballot(on);
    if (lane == 0) waveCount[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t base = 0, total = 0;
    for (uint32_t i = 0; i < kPsBlock / 64; i++) { if (i < wave) base += waveCount[i]; total += waveCount[i]; }
    if (on) {
        const uint32_t pos = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        a.actT[pos] = t; a.actA[pos] = w;
    }
    if (t == 0) a.words[1] = total;
}

template <bool kLds> __global__ __launch_bounds__(kPsBlock) void k_ps_pose(PsArgs a)
{
    extern __shared__ float ps_lds[];                // 3 * kPsBlock words of a tile's result, then (kLds) 12 words per joint
    float* stage = ps_lds;
    float* lmats = ps_lds + 3 * kPsBlock;
    const uint32_t tid = threadIdx.x;
    if (kLds) {
        for (uint32_t i = tid; i < 12u * a.numJoints; i += kPsBlock) lmats[i] = a.mats[i];
        __syncthreads();
    }
    const size_t S = a.stride, V = a.numVerts;
    const uint32_t nAct = a.words[1], K = a.numJoints ? a.influences : 0u;
    for (uint32_t tile = blockIdx.x; tile < a.numTiles; tile += gridDim.x) {
        const size_t base = (size_t)tile * kPsBlock, v = base + tid;
        PsVec r = { 0.0f, 0.0f, 0.0f };
        if (v < V) {
            PsVec m = { a.rest[v], a.rest[S + v], a.rest[2 * S + v] };
            for (uint32_t i = 0; i < nAct; i++) {
                const float* d = a.deltas + 3 * (size_t)a.actT[i] * S + v;
                ps_morph(m, a.actA[i], d[0], d[S], d[2 * S]);
            }
            PsVec p = { 0.0f, 0.0f, 0.0f };
            bool any = false;
            for (uint32_t k = 0; k < K; k++) {
                const float w = a.weights[k * S + v];
                const uint32_t j = a.joints[k * S + v];
                if (w != 0.0f) { ps_skin(p, (kLds ? lmats : a.mats) + 12 * (size_t)j, m, w); any = true; }
            }
            r = any ? p : m;
        }
        stage[3 * tid] = r.x; stage[3 * tid + 1] = r.y; stage[3 * tid + 2] = r.z;
        __syncthreads();
        const uint32_t n3 = 3u * (uint32_t)std::min((size_t)kPsBlock, V - base);
        float* out = a.verts + 3 * base;
        for (uint32_t i = tid; i < n3; i += kPsBlock) out[i] = stage[i];
        __syncthreads();                             // the next tile writes `stage` again
    }
}

static inline uint32_t ps_grid(size_t n) { return grid_for(n, kPsBlock); }

// ---- host side (gmupt_capi_pose.hip) ----

PsLayout pose_layout(uint32_t numVerts, uint32_t influences, uint32_t numJoints, uint32_t numTargets)
{
    PsLayout L{};
    L.stride = ((size_t)numVerts + 63) & ~(size_t)63;
    const size_t K = numJoints ? influences : 0;
    size_t total = 0;
    auto place = [&total](size_t& off, size_t bytes) { off = total; total += scratch_align(bytes); };
    place(L.words, kPsWords * 4);
    place(L.rest, 3 * L.stride * 4);
    place(L.weights, K * L.stride * 4);
    place(L.joints, K * L.stride * 2);
    place(L.deltas, 3 * (size_t)numTargets * L.stride * 4);
    place(L.mats, 12 * (size_t)numJoints * 4);
    place(L.targetWeights, (size_t)numTargets * 4);
    place(L.actT, (size_t)numTargets * 4);
    place(L.actA, (size_t)numTargets * 4);
    L.total = total;
    return L;
}

// enqueues the copy of the rig into the handle's planes; a.words (kPsWords words, cleared here) is read back by the caller afterwards
hipError_t launch_pose_create(const PsArgs& a, hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(a.words, 0, kPsWords * 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ps_pack, dim3(ps_grid(a.numVerts)), dim3(kPsBlock), 0, s, a);
    return hipGetLastError();
}

// a.mats and a.targetWeights hold this pose (copied on s before)
void launch_pose_update(const PsArgs& a0, hipStream_t s)
{
    PsArgs a = a0;
    a.numTiles = ps_grid(a.numVerts);
    hipLaunchKernelGGL(k_ps_active, dim3(1), dim3(kPsBlock), 0, s, a);
    const uint32_t grid = std::min(a.numTiles, kPsMaxGrid);
    const bool lds = a.numJoints > 0 && a.numJoints <= kPsLdsJoints;
    const size_t shared = 3 * kPsBlock * sizeof(float) + (lds ? 48 * (size_t)a.numJoints : 0);
    if (lds) hipLaunchKernelGGL(k_ps_pose<true>, dim3(grid), dim3(kPsBlock), shared, s, a);
    else hipLaunchKernelGGL(k_ps_pose<false>, dim3(grid), dim3(kPsBlock), shared, s, a);
}

} // namespace gmupt
