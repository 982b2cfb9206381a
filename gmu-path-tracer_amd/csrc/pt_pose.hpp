// The arithmetic of the pose stage (include/gmupt.h "Pose" states the rule), shared by gmupt_pose_host (pt_pose.cpp) and k_ps_pose
// (pt_pose.hip): one morph step and one skinning influence.  One copy, so that host and device run the same binary32 statements; nothing
// is contracted (build.py).  The ORDER -- targets ascending, then influences ascending -- and the skip of zero weights are the other half
// of the rule; both callers walk their lists in that order and test the weight before they call.
#pragma once
#include "pt_device.hpp"
#include "detmath.hpp"

namespace gmupt {

constexpr uint32_t kPsMaxInfluences = 8, kPsMaxJoints = 65535, kPsMaxTargets = 256;
constexpr uint32_t kPsFlagBadJoint = 1u;
constexpr uint32_t kPsLdsJoints = 640;         // joint matrices the kernel keeps in LDS (30 KB of a block's share); more are read from global memory.  Chosen by the LDS arithmetic (four blocks per CU), not by a measurement
constexpr uint32_t kPsWords = 16;              // [0] kPsFlag*, [1] the number of active targets of the last update

struct PsVec { float x, y, z; };              // a vertex in three named floats: registers on the device

// rule 1, one target with a weight that is not zero: m = m + a * d
GM_HD void ps_morph(PsVec& m, float a, float dx, float dy, float dz)
{
    m.x = m.x + a * dx; m.y = m.y + a * dy; m.z = m.z + a * dz;
}

// rule 2, one influence with a weight that is not zero: q = M * (m, 1) row by row, p = p + w * q.  M: 3 rows x 4 columns, row-major
GM_HD void ps_skin(PsVec& p, const float* M, const PsVec& m, float w)
{
    const float q0 = ((M[0] * m.x + M[1] * m.y) + M[2] * m.z) + M[3];
    const float q1 = ((M[4] * m.x + M[5] * m.y) + M[6] * m.z) + M[7];
    const float q2 = ((M[8] * m.x + M[9] * m.y) + M[10] * m.z) + M[11];
    p.x = p.x + w * q0; p.y = p.y + w * q1; p.z = p.z + w * q2;
}

// Byte offsets of the parts of a gmupt_pose handle's device memory (one allocation, pt_pose.hip: pose_layout places them).  Everything
// per vertex is stored plane by plane -- one array of `stride` elements (the vertex count rounded up to 64) per component -- so that a
// wave reads 64 consecutive elements of a plane with one whole-dword (joints: half-dword) access per lane, in lane order:
//   rest     3 float planes (x, y, z)                         12 bytes per vertex
//   weights  K float planes, joints K uint16 planes            6 bytes per vertex and influence (none when num_joints == 0)
//   deltas   3 float planes per target                        12 bytes per vertex and target
// and, per update: mats (12 floats per joint), targetWeights (one float per target), actT / actA (the targets whose weight is not zero, in
// ascending order, with that weight: written by k_ps_active).
struct PsLayout { size_t words, rest, weights, joints, deltas, mats, targetWeights, actT, actA, total; size_t stride; };

// what the kernels of a handle work on
struct PsArgs {
    uint32_t numVerts, influences, numJoints, numTargets;
    size_t stride;                                 // elements per plane
    float* rest; float* weights; uint16_t* joints; float* deltas;
    float* mats; float* targetWeights; uint32_t* actT; float* actA;
    uint32_t* words;
    const float* srcRest; const uint16_t* srcJoints; const float* srcWeights; const float* srcDeltas;   // create only: the caller's arrays
    float* verts;                                  // update only: the vertex buffer the renderer is bound to
    uint32_t numTiles;
};

// ---- host reference (pt_pose.cpp) on validated input: vertsOut holds 3 floats per vertex
void pose_host(const float* rest, uint32_t numVerts, const uint16_t* joints, const float* weights, uint32_t influences, const float* jointMats,
               uint32_t numJoints, const float* deltas, const float* targetWeights, uint32_t numTargets, float* vertsOut, int threads);
// rule 4 on host arrays: the first vertex with a joint number >= numJoints on a weight that is not zero, or numVerts
size_t pose_first_bad_joint(const uint16_t* joints, const float* weights, uint32_t influences, uint32_t numJoints, uint32_t numVerts);

} // namespace gmupt
