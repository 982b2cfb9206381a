// The camera projections on the device (include/gmupt_projection.h states the rule; pt_projection.hpp is its arithmetic).
//   k_proj_retarget  between k_material (and k_ad_retarget, when a sampling plan is attached) and the ray cast: one thread per entry
//                    of the new-path queue.  Gives the fresh camera path the ray of the attached projection: F_RAY_OX..OZ and
//                    F_RAY_DX..DZ, nothing else.  The pixel is read from F_SCR_X/Y of the slot, which already holds the tile origin
//                    and the pixel of an attached plan.  A streaming kernel: per fresh path it reads 4 bytes of the queue and 8 of
//                    the state and writes 24; no LDS, no atomics.  The kind is wave-uniform (a launch argument).  The guards are
//                    fresh_path_slot (pt_kernel_util.hpp), shared with k_ad_retarget and k_lens_retarget.
//   k_paov_raygen    one thread per ray of a chunk of gmupt_render_aovs_projected: the R = s*s stratified rays of every pixel as
//                    gmupt_ray records, pixel-major -- aov_raygen (pt_camera_rays.hpp) with this file's rule, where k_laov_raygen
//                    has the lens rule; the wide ray cast and k_laov_resolve follow unchanged.
#include "pt_projection.hpp"
#include "pt_kernel_util.hpp"

namespace gmupt {

__global__ __launch_bounds__(kBlock) void k_proj_retarget(RenderParams p, gmupt_projection proj)
{
    const uint32_t queueIndex = blockIdx.x * kBlock + threadIdx.x;
    uint32_t index, lastPath;
    if (!fresh_path_slot(p, queueIndex, index, lastPath)) return;
    const uint32_t cx = ldu(p, F_SCR_X, index), cy = ldu(p, F_SCR_Y, index);  // whole-frame pixel: the tile origin is in it
    const CamRay r = projection_fresh_ray(p.cam, proj, queueIndex, cx, cy);
    st3(p, F_RAY_OX, index, r.origin);
    st3(p, F_RAY_DX, index, r.direction);
}

void launch_proj_retarget(const RenderParams& p, const gmupt_projection& proj, hipStream_t s)
{
    hipLaunchKernelGGL(k_proj_retarget, dim3(p.nBlocks), dim3(kBlock), 0, s, p, proj);
}

struct ProjectedAovRule {
    gmupt_camera_buffer cam;
    gmupt_projection proj;
    __device__ __forceinline__ CamRay operator()(uint32_t x, uint32_t y, uint32_t s, uint32_t k) const { return projection_aov_ray(cam, proj, x, y, s, k); }
};

__global__ __launch_bounds__(kBlock) void k_paov_raygen(AovRaygen<ProjectedAovRule> g) { aov_raygen(g.chunk, g.rule); }

void launch_paov_raygen(const gmupt_camera_buffer& cam, const gmupt_projection& proj, uint32_t x0, uint32_t y0, uint32_t width, uint32_t rows, uint32_t samples,
                        gmupt_ray* rays, hipStream_t s)
{
    launch_raygen_kernel(k_paov_raygen, ProjectedAovRule{ cam, proj }, x0, y0, width, rows, samples, samples * samples, rays, s);
}

} // namespace gmupt
