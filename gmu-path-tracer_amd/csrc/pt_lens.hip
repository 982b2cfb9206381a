// The thin lens on the device (include/gmupt_lens.h states the rule; pt_lens.hpp is its arithmetic).
//   k_lens_retarget  between k_material (and k_ad_retarget, when a sampling plan is attached) and the ray cast: one thread per entry
//                    of the new-path queue.  Moves the origin of the fresh camera path onto the lens disk and aims it through the
//                    focal point of its pinhole ray: F_RAY_OX..OZ and F_RAY_DX..DZ, nothing else.  The pixel is read from F_SCR_X/Y
//                    of the slot, which already holds the tile origin and the pixel of an attached plan.  A streaming kernel: per
//                    fresh path it reads 4 bytes of the queue and 8 of the state and writes 24; no LDS, no atomics.  The guards are
//                    fresh_path_slot (pt_kernel_util.hpp), shared with k_ad_retarget and k_proj_retarget.
#include "pt_lens.hpp"
#include "pt_kernel_util.hpp"

namespace gmupt {

__global__ __launch_bounds__(kBlock) void k_lens_retarget(RenderParams p, float apertureRadius, float focusDistance)
{
    const uint32_t queueIndex = blockIdx.x * kBlock + threadIdx.x;
    uint32_t index, lastPath;
    if (!fresh_path_slot(p, queueIndex, index, lastPath)) return;
    const uint32_t cx = ldu(p, F_SCR_X, index), cy = ldu(p, F_SCR_Y, index);  // whole-frame pixel: the tile origin is in it
    const CamRay r = lens_ray(p.cam, apertureRadius, focusDistance, queueIndex, cx, cy);
    st3(p, F_RAY_OX, index, r.origin);
    st3(p, F_RAY_DX, index, r.direction);
}

void launch_lens_retarget(const RenderParams& p, float apertureRadius, float focusDistance, hipStream_t s)
{
    hipLaunchKernelGGL(k_lens_retarget, dim3(p.nBlocks), dim3(kBlock), 0, s, p, apertureRadius, focusDistance);
}

} // namespace gmupt
