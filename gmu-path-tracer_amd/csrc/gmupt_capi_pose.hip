// C-ABI of libgmupt.so: the pose stage on the device (gmupt_pose_*, pt_pose.hip) -- skinning and morph targets from a rig the handle
// keeps into the vertex buffer the renderer is bound to.  gmupt_pose_host, which needs no device, is in gmupt_capi_host.cpp.
#include "gmupt_internal.hpp"

static_assert(sizeof(gmupt_pose_info) == 16 && offsetof(gmupt_pose_info, ms) == 8, "gmupt_pose_info layout");

// the kernel argument of a handle; the src* pointers are filled in by create, verts by update
static PsArgs pose_args(const gmupt_pose* p)
{
    char* base = p->mem.as<char>();
    PsArgs a{};
    a.numVerts = p->numVerts; a.influences = p->influences; a.numJoints = p->numJoints; a.numTargets = p->numTargets; a.stride = p->off.stride;
    a.rest = (float*)(base + p->off.rest); a.weights = (float*)(base + p->off.weights); a.joints = (uint16_t*)(base + p->off.joints);
    a.deltas = (float*)(base + p->off.deltas); a.mats = (float*)(base + p->off.mats); a.targetWeights = (float*)(base + p->off.targetWeights);
    a.actT = (uint32_t*)(base + p->off.actT); a.actA = (float*)(base + p->off.actA); a.words = (uint32_t*)(base + p->off.words);
    return a;
}

extern "C" int gmupt_pose_create(gmupt_renderer* r, const float* device_rest, const uint16_t* device_joints, const float* device_weights, uint32_t influences,
                                 uint32_t num_joints, const float* device_deltas, uint32_t num_targets, gmupt_pose** out)
{
    if (out) *out = nullptr;
    if (!r || !device_rest || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_pose_create: null argument");
    if (!r->sceneBound) return fail(GMUPT_ERR_NOT_BOUND, "gmupt_pose_create: no scene bound");
    const size_t V = r->boundVerts->elems;
    if (V == 0 || V > 0x7FFFFFFFu) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_pose_create: %zu vertices (1 .. 2^31 - 1)", V);
    if (num_joints == 0 && num_targets == 0) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_pose_create: neither joints nor morph targets");
    if (num_joints > kPsMaxJoints || num_targets > kPsMaxTargets)
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_pose_create: %u joints (at most %u), %u targets (at most %u)", num_joints, kPsMaxJoints, num_targets, kPsMaxTargets);
    if (num_joints && (influences < 1 || influences > kPsMaxInfluences)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_pose_create: influences = %u (1..%u)", influences, kPsMaxInfluences);
    if (num_joints && (!device_joints || !device_weights)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_pose_create: %u joints without joint numbers or weights", num_joints);
    if (num_targets && !device_deltas) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_pose_create: %u targets without deltas", num_targets);
    if (((uintptr_t)device_rest & 3) || (num_joints && (((uintptr_t)device_weights & 3) || ((uintptr_t)device_joints & 1))) || (num_targets && ((uintptr_t)device_deltas & 3)))
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_pose_create: misaligned pointer");
    HIP_TRY(hipSetDevice(r->dev->id));
    gmupt_pose* p = new (std::nothrow) gmupt_pose();
    if (!p) return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_pose_create: out of host memory");
    p->r = r; p->numVerts = (uint32_t)V; p->influences = num_joints ? influences : 0; p->numJoints = num_joints; p->numTargets = num_targets;
    auto build = [&]() -> int {
        p->off = pose_layout(p->numVerts, p->influences, num_joints, num_targets);
        GMUPT_TRY(p->mem.grow(r->stream, p->off.total));
        GMUPT_TRY(p->staging.alloc((12 * (size_t)num_joints + num_targets) * sizeof(float)));
        GMUPT_TRY(p->staged.create());
        PsArgs a = pose_args(p);
        a.srcRest = device_rest; a.srcJoints = device_joints; a.srcWeights = device_weights; a.srcDeltas = device_deltas;
        HIP_TRY(launch_pose_create(a, r->stream));
        uint32_t flags = 0;
        GMUPT_TRY(copy_sync(&flags, a.words, sizeof(flags), hipMemcpyDeviceToHost, r->stream));
        if (flags & kPsFlagBadJoint) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_pose_create: an influence with a weight that is not zero names a joint outside the %u joints", num_joints);
        return GMUPT_OK;
    };
    const int rc = build();
    if (rc != GMUPT_OK) { (void)hipStreamSynchronize(r->stream); delete p; return rc; }
    *out = p;
    return GMUPT_OK;
}

extern "C" void gmupt_pose_destroy(gmupt_pose* p)
{
    if (!p) return;
    (void)hipSetDevice(p->r->dev->id);
    (void)hipStreamSynchronize(p->r->stream);
    delete p;
}

// both updates: the checks, the copy of this pose's matrices and target weights into the handle (from the pinned staging area when
// they come from the host), the two launches, and the timing when the caller asks for it
static int pose_update(gmupt_pose* p, const char* fn, const float* joint_mats, const float* target_weights, bool fromHost, gmupt_pose_info* info)
{
    if (!p) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null handle", fn);
    if (info) *info = gmupt_pose_info{};
    gmupt_renderer* r = p->r;
    if ((p->numJoints && !joint_mats) || (p->numTargets && !target_weights)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
    if (!fromHost && (((uintptr_t)joint_mats | (uintptr_t)target_weights) & 3)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: misaligned pointer", fn);
    if (!r->sceneBound) return fail(GMUPT_ERR_NOT_BOUND, "%s: no scene bound", fn);
    if (r->boundVerts->elems != p->numVerts)
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: the bound vertex buffer holds %zu vertices, the handle was created for %u", fn, r->boundVerts->elems, p->numVerts);
    HIP_TRY(hipSetDevice(r->dev->id));
    PsArgs a = pose_args(p);
    a.verts = (float*)r->boundVerts->dptr;
    const size_t matBytes = 12 * (size_t)p->numJoints * sizeof(float), twBytes = (size_t)p->numTargets * sizeof(float);
    if (info) GMUPT_TRY(p->ev.start(r->stream));
    if (fromHost) {
        // the staging area is the handle's only one: the copies of the call before must have read it (they are a few kilobytes, long done
        // unless the stream is far behind)
        if (p->stagingBusy) { HIP_TRY(hipEventSynchronize(p->staged.e[0])); p->stagingBusy = false; }
        char* st = p->staging.as<char>();
        if (matBytes) std::memcpy(st, joint_mats, matBytes);
        if (twBytes) std::memcpy(st + matBytes, target_weights, twBytes);
        if (matBytes) HIP_TRY(hipMemcpyAsync(a.mats, st, matBytes, hipMemcpyHostToDevice, r->stream));
        if (twBytes) HIP_TRY(hipMemcpyAsync(a.targetWeights, st + matBytes, twBytes, hipMemcpyHostToDevice, r->stream));
        HIP_TRY(hipEventRecord(p->staged.e[0], r->stream));
        p->stagingBusy = true;
    } else {
        if (matBytes) HIP_TRY(hipMemcpyAsync(a.mats, joint_mats, matBytes, hipMemcpyDeviceToDevice, r->stream));
        if (twBytes) HIP_TRY(hipMemcpyAsync(a.targetWeights, target_weights, twBytes, hipMemcpyDeviceToDevice, r->stream));
    }
    launch_pose_update(a, r->stream);
    HIP_TRY(hipGetLastError());
    if (!info) return GMUPT_OK;
    GMUPT_TRY(p->ev.stop(r->stream));
    uint32_t active = 0;
    GMUPT_TRY(copy_sync(&active, a.words + 1, sizeof(active), hipMemcpyDeviceToHost, r->stream));
    float ms = 0.0f;
    GMUPT_TRY(p->ev.elapsed_ms(&ms));
    info->num_verts = p->numVerts; info->active_targets = active; info->ms = (double)ms;
    return GMUPT_OK;
}

extern "C" int gmupt_pose_update(gmupt_pose* p, const float* joint_mats, const float* target_weights, gmupt_pose_info* info)
{
    return pose_update(p, "gmupt_pose_update", joint_mats, target_weights, true, info);
}

extern "C" int gmupt_pose_update_device(gmupt_pose* p, const float* device_joint_mats, const float* device_target_weights, gmupt_pose_info* info)
{
    return pose_update(p, "gmupt_pose_update_device", device_joint_mats, device_target_weights, false, info);
}
