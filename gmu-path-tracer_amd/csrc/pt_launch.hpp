// Host-side entry points of the kernel files, as the C-API units (gmupt_capi*.hip) call them.  Every file that defines one of these
// includes this header, so that the compiler checks the definition against the declaration.  (The host rules, the *_host functions of
// the pt_*.cpp files, are each declared in their feature's pt_*.hpp.)
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "../../include/gmupt.h"

namespace gmupt {
struct RenderParams; struct SceneView; struct DnParams; struct IfParams; struct IfCounters; struct TpParams; struct TpPrev; struct RfArgs; struct LbStaging; struct NmLayout; struct NmArgs; struct TcPartial; struct PsLayout; struct PsArgs;   // pt_*.hpp

void launch_clear(const RenderParams& p, hipStream_t s);
void launch_logic(const RenderParams& p, hipStream_t s);
void launch_material(const RenderParams& p, int clearFrame, hipStream_t s);
void launch_detmath(int fn, const float* x, const float* y, float* out, uint32_t n, hipStream_t s);
uint32_t launch_extend(const RenderParams& p, uint32_t blocks, bool stats, int mode, hipStream_t s);   // the launch_* of the ray casts return GMUPT_STAT_* bits of what they launched
uint32_t launch_shadow(const RenderParams& p, uint32_t blocks, bool stats, int mode, hipStream_t s);
uint32_t launch_cast(const RenderParams& p, bool stats, int mode, hipStream_t s);                      // 0: not launched, run the two separate casts
bool traversal_is_fused(int mode);
bool traversal_mode_available(int mode);
uint32_t traversal_block_threads();
uint32_t deferred_block_threads();
uint32_t traversal_overflow_entries();
uint32_t traversal_top_capacity(uint32_t maxDepth);
uint32_t traversal_wide_top_capacity();
void launch_trace_wide(const RenderParams& p, const gmupt_ray* closest, uint32_t nClosest, gmupt_hit* hits, const gmupt_ray* any, uint32_t nAny,
                       uint32_t* occluded, uint32_t lightCount, hipStream_t s);
void launch_aov_raygen(const gmupt_camera_buffer& cam, uint32_t x0, uint32_t y0, uint32_t width, uint32_t rows, uint32_t samples, uint32_t R,
                       gmupt_ray* rays, hipStream_t s);
void launch_aov_resolve(const RenderParams& p, uint32_t npix, uint32_t samples, uint32_t R, const gmupt_ray* rays, const gmupt_hit* hits,
                        gmupt_aov* out, hipStream_t s);
void launch_denoise(const float4* beauty, const float4* aov, int W, int H, const DnParams& prm, void* scratch, float4* out, hipStream_t s);
size_t infill_scratch_bytes(size_t npix);
hipError_t launch_infill(const float4* beauty, const float4* aov, int W, int H, const IfParams& prm, void* scratch, float4* out, hipStream_t s,
                         const IfCounters** countsOut);
void launch_temporal(const float4* beauty, const float4* aov, int W, int H, const TpPrev& prev, const TpParams& prm, float4* out, float4* hist,
                     hipStream_t s);
void launch_temporal_motion(const float4* beauty, const float4* aov, const float4* motion, int W, int H, const TpPrev& prev, const TpParams& prm,
                            float4* out, float4* hist, hipStream_t s);
void launch_mv_resolve(const SceneView& scene, const float* prevVerts, uint32_t npix, uint32_t R, const gmupt_hit* hits, const gmupt_aov* aov,
                       gmupt_motion* out, hipStream_t s);
void launch_refit_check(const RfArgs& a, hipStream_t s);
uint32_t launch_refit_boxes(const RfArgs& a, const std::vector<uint32_t>& levelOff, hipStream_t s);
void launch_refit_tables(const RfArgs& a, hipStream_t s);
hipError_t lbvh_sort_temp_bytes(uint32_t n, size_t* bytes);
size_t lbvh_scratch_bytes(uint32_t cap, size_t sortTemp);
hipError_t launch_lbvh(void* scratch, uint32_t cap, size_t sortTemp, const float* verts, uint32_t numVerts, const int32_t* indices, uint32_t n,
                       const uint32_t* vertexMaterial, uint32_t maxLeaf, hipStream_t s, LbStaging& st);
hipError_t normals_sort_temp_bytes(uint32_t numTris, uint32_t numVerts, size_t* bytes);
NmLayout normals_layout(uint32_t numTris, uint32_t numVerts, size_t sortTemp);
hipError_t launch_normals_create(const NmArgs& a, void* sortTemp, size_t sortTempBytes, hipStream_t s);
void launch_normals_update(const NmArgs& a, hipStream_t s);
PsLayout pose_layout(uint32_t numVerts, uint32_t influences, uint32_t numJoints, uint32_t numTargets);
hipError_t launch_pose_create(const PsArgs& a, hipStream_t s);
void launch_pose_update(const PsArgs& a, hipStream_t s);
size_t tree_cost_scratch_partials(uint32_t n);
const TcPartial* launch_tree_cost(const gmupt_bvh_node* nodes, uint32_t n, TcPartial* scratch, hipStream_t s);
hipError_t treeopt_sort_temp_bytes(uint32_t n, size_t* bytes);
size_t treeopt_scratch_bytes(uint32_t cap, size_t sortTemp);
hipError_t launch_treeopt(void* scratch, uint32_t cap, size_t sortTemp, const gmupt_bvh_node* nodes, uint32_t n, uint32_t passes, hipStream_t s,
                          const void** words, const void** staged);
}
