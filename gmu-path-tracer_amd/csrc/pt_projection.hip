// The camera projections on the device (include/gmupt_projection.h states the rule; pt_projection.hpp is its arithmetic).
//   k_proj_retarget  between k_material (and k_ad_retarget, when a sampling plan is attached) and the ray cast: one thread per entry
//                    of the new-path queue.  Gives the fresh camera path the ray of the attached projection: F_RAY_OX..OZ and
//                    F_RAY_DX..DZ, nothing else.  The pixel is read from F_SCR_X/Y of the slot, which already holds the tile origin
//                    and the pixel of an attached plan.  A streaming kernel: per fresh path it reads 4 bytes of the queue and 8 of
//                    the state and writes 24; no LDS, no atomics.  The kind is wave-uniform (a launch argument).  The guards are
//                    k_lens_retarget's, statement for statement.
//   k_paov_raygen    one thread per ray of a chunk of gmupt_render_aovs_projected: the R = s*s stratified rays of every pixel as
//                    gmupt_ray records, pixel-major, where k_laov_raygen writes the lens rays; the wide ray cast and k_laov_resolve
//                    follow unchanged.
#include "pt_projection.hpp"
#include "pt_kernel_util.hpp"

namespace gmupt {

__global__ __launch_bounds__(kBlock) void k_proj_retarget(RenderParams p, gmupt_projection proj)
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
    const ProjRay r = projection_fresh_ray(p.cam, proj, queueIndex, cx, cy);
    st3(p, F_RAY_OX, index, r.origin);
    st3(p, F_RAY_DX, index, r.direction);
}

void launch_proj_retarget(const RenderParams& p, const gmupt_projection& proj, hipStream_t s)
{
    hipLaunchKernelGGL(k_proj_retarget, dim3(p.nBlocks), dim3(kBlock), 0, s, p, proj);
}

struct PaovRaygen {
    gmupt_camera_buffer cam;
    gmupt_projection proj;
    uint32_t x0, y0;     // whole-frame coordinates of the chunk's first pixel
    uint32_t width;      // pixels per row
    uint32_t samples, R; // s, rays per pixel (s*s)
    uint32_t n;          // rays of the chunk (rows * width * R <= GMUPT_AOV_CHUNK_RAYS)
    float4* rays;        // 2 float4 per gmupt_ray
};

__global__ __launch_bounds__(kBlock) void k_paov_raygen(PaovRaygen g)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= g.n) return;
    const uint32_t pix = i / g.R, k = i - pix * g.R;
    const uint32_t ly = pix / g.width, lx = pix - ly * g.width;
    const ProjRay r = projection_aov_ray(g.cam, g.proj, g.x0 + lx, g.y0 + ly, g.samples, k);
    g.rays[2 * (size_t)i] = make_float4(r.origin.x, r.origin.y, r.origin.z, kFltMax);   // tmax = FLT_MAX
    g.rays[2 * (size_t)i + 1] = make_float4(r.direction.x, r.direction.y, r.direction.z, 0.0f);
}

void launch_paov_raygen(const gmupt_camera_buffer& cam, const gmupt_projection& proj, uint32_t x0, uint32_t y0, uint32_t width, uint32_t rows, uint32_t samples,
                        gmupt_ray* rays, hipStream_t s)
{
    PaovRaygen g;
    g.cam = cam; g.proj = proj;
    g.x0 = x0; g.y0 = y0; g.width = width; g.samples = samples; g.R = samples * samples; g.n = rows * width * g.R;
    g.rays = reinterpret_cast<float4*>(rays);
    if (g.n) hipLaunchKernelGGL(k_paov_raygen, dim3((g.n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, g);
}

} // namespace gmupt
