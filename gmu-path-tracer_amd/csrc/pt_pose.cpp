// gmupt_pose_host: the rule of include/gmupt.h ("Pose") on host arrays, the reference of the device path (pt_pose.hip).  The arithmetic is
// pt_pose.hpp, shared with the kernel.  A vertex depends on no other vertex, so the bands of the threads are independent and the result
// cannot depend on the thread count.
#include "pt_pose.hpp"
#include "pt_bands.hpp"

#include <algorithm>

namespace gmupt {

size_t pose_first_bad_joint(const uint16_t* joints, const float* weights, uint32_t influences, uint32_t numJoints, uint32_t numVerts)
{
    const size_t n = (size_t)numVerts * influences;
    for (size_t i = 0; i < n; i++)
        if (weights[i] != 0.0f && joints[i] >= numJoints) return i / influences;
    return numVerts;
}

void pose_host(const float* rest, uint32_t numVerts, const uint16_t* joints, const float* weights, uint32_t influences, const float* jointMats,
               uint32_t numJoints, const float* deltas, const float* targetWeights, uint32_t numTargets, float* vertsOut, int threads)
{
    constexpr size_t kChunk = 4096;
    const size_t V = numVerts, K = influences;
    host_bands((int)((V + kChunk - 1) / kChunk), threads, [&](int c0, int c1) {
        for (size_t v = (size_t)c0 * kChunk; v < std::min(V, (size_t)c1 * kChunk); v++) {
            PsVec m = { rest[3 * v], rest[3 * v + 1], rest[3 * v + 2] };
            for (size_t t = 0; t < numTargets; t++) {
                const float a = targetWeights[t];
                if (a != 0.0f) { const float* d = deltas + 3 * (t * V + v); ps_morph(m, a, d[0], d[1], d[2]); }
            }
            PsVec p = { 0.0f, 0.0f, 0.0f };
            bool any = false;
            if (numJoints)
                for (size_t k = 0; k < K; k++) {
                    const float w = weights[v * K + k];
                    if (w != 0.0f) { ps_skin(p, jointMats + 12 * (size_t)joints[v * K + k], m, w); any = true; }
                }
            const PsVec r = any ? p : m;
            vertsOut[3 * v] = r.x; vertsOut[3 * v + 1] = r.y; vertsOut[3 * v + 2] = r.z;
        }
    });
}

} // namespace gmupt
