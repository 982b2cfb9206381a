// The thin lens on the device (include/gmupt_lens.h states the rule; pt_lens.hpp is its arithmetic).
//   k_lens_retarget  between k_material (and k_ad_retarget, when a sampling plan is attached) and the ray cast: one thread per entry
//                    of the new-path queue.  Moves the origin of the fresh camera path onto the lens disk and aims it through the
//                    focal point of its pinhole ray: F_RAY_OX..OZ and F_RAY_DX..DZ, nothing else.  The pixel is read from F_SCR_X/Y
//                    of the slot, which already holds the tile origin and the pixel of an attached plan.  A streaming kernel: per
//                    fresh path it reads 4 bytes of the queue and 8 of the state and writes 24; no LDS, no atomics.  The guards are
//                    k_ad_retarget's, statement for statement.
#include "pt_lens.hpp"
#include "pt_kernel_util.hpp"

namespace gmupt {

__global__ __launch_bounds__(kBlock) void k_lens_retarget(RenderParams p, float apertureRadius, float focusDistance)
{
    const uint32_t queueIndex = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t qc0 = p.qc[QC_NEWPATH];
    const uint32_t nNew = qc0 < p.L ? qc0 : p.L;                              // newPath.hlsl:21-25, as k_material
    if (queueIndex >= nNew) return;
    const uint32_t index = p.queues[(size_t)Q_NEWPATH * p.P + queueIndex];
    if (index >= p.L) return;
    const uint32_t lastPath = p.qc[QC_LASTPATHCNT];                          // :19 -- the ray cast advances it, later
    if (p.budget && (uint32_t)(lastPath + queueIndex) >= p.budget) return;   // retired by stage_new_path
    const uint32_t cx = ldu(p, F_SCR_X, index), cy = ldu(p, F_SCR_Y, index);  // whole-frame pixel: the tile origin is in it
    const LensRay r = lens_ray(p.cam, apertureRadius, focusDistance, queueIndex, cx, cy);
    st3(p, F_RAY_OX, index, r.origin);
    st3(p, F_RAY_DX, index, r.direction);
}

void launch_lens_retarget(const RenderParams& p, float apertureRadius, float focusDistance, hipStream_t s)
{
    hipLaunchKernelGGL(k_lens_retarget, dim3(p.nBlocks), dim3(kBlock), 0, s, p, apertureRadius, focusDistance);
}

} // namespace gmupt
