// The shutter on the device (include/gmupt_shutter.h states the rule; pt_shutter.hpp is its arithmetic).
//   k_shutter_retarget_{pinhole,lens,proj}
//                    between k_material (and k_ad_retarget, when a sampling plan is attached) and the ray cast, in place of
//                    k_lens_retarget / k_proj_retarget: one thread per entry of the new-path queue.  Draws the path's time, interpolates
//                    the camera to it and gives the fresh camera path the ray of the attached rule on that camera: F_RAY_OX..OZ and
//                    F_RAY_DX..DZ, nothing else.  The pixel is read from F_SCR_X/Y of the slot, which already holds the tile origin and
//                    the pixel of an attached plan.  A streaming kernel: per fresh path it reads 4 bytes of the queue and 8 of the state
//                    and writes 24; no LDS, no atomics.  Which rule runs is wave-uniform: three thin __global__ wrappers around the one
//                    body, as the ray generation of pt_camera_rays.hpp.  The guards are fresh_path_slot (pt_kernel_util.hpp), shared
//                    with k_ad_retarget, k_lens_retarget and k_proj_retarget.
#include "pt_shutter.hpp"
#include "pt_kernel_util.hpp"

namespace gmupt {

template <class Rule> __device__ __forceinline__ void shutter_retarget(const RenderParams& p, const gmupt_shutter& sh, const Rule& rule)
{
    const uint32_t queueIndex = blockIdx.x * kBlock + threadIdx.x;
    uint32_t index, lastPath;
    if (!fresh_path_slot(p, queueIndex, index, lastPath)) return;
    const uint32_t cx = ldu(p, F_SCR_X, index), cy = ldu(p, F_SCR_Y, index);  // whole-frame pixel: the tile origin is in it
    const CamRay r = shutter_ray(p.cam, sh, rule, queueIndex, cx, cy);
    st3(p, F_RAY_OX, index, r.origin);
    st3(p, F_RAY_DX, index, r.direction);
}

__global__ __launch_bounds__(kBlock) void k_shutter_retarget_pinhole(RenderParams p, gmupt_shutter sh, ShutterPinhole rule) { shutter_retarget(p, sh, rule); }
__global__ __launch_bounds__(kBlock) void k_shutter_retarget_lens(RenderParams p, gmupt_shutter sh, ShutterLens rule) { shutter_retarget(p, sh, rule); }
__global__ __launch_bounds__(kBlock) void k_shutter_retarget_proj(RenderParams p, gmupt_shutter sh, ShutterProjection rule) { shutter_retarget(p, sh, rule); }

void launch_shutter_retarget(const RenderParams& p, const gmupt_shutter& sh, const gmupt_lens& lens, const gmupt_projection& proj, hipStream_t s)
{
    const dim3 grid(p.nBlocks), block(kBlock);
    if (lens.aperture_radius > 0.0f)
        hipLaunchKernelGGL(k_shutter_retarget_lens, grid, block, 0, s, p, sh, ShutterLens{ lens.aperture_radius, lens.focus_distance });
    else if (proj.kind != GMUPT_PROJ_PINHOLE)
        hipLaunchKernelGGL(k_shutter_retarget_proj, grid, block, 0, s, p, sh, ShutterProjection{ proj });
    else
        hipLaunchKernelGGL(k_shutter_retarget_pinhole, grid, block, 0, s, p, sh, ShutterPinhole{});
}

} // namespace gmupt
