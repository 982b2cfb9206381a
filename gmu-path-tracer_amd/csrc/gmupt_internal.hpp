// What the C-API units of libgmupt.so (gmupt_capi*.hip, gmupt_capi_host.cpp) share: the error return, the handle structs, the two types
// that own device memory and events, and the checks more than one unit makes.  Not installed; nothing in here is exported.
#pragma once
#include "pt_shading.hpp"
#include "pt_denoise.hpp"
#include "pt_infill.hpp"
#include "pt_temporal.hpp"
#include "pt_motion.hpp"
#include "pt_travtables.hpp"
#include "pt_lbvh.hpp"                // and with it pt_refit.hpp, pt_device.hpp, detmath.hpp
#include "pt_normals.hpp"
#include "pt_treecost.hpp"
#include "pt_treeopt.hpp"
#include "pt_pose.hpp"
#include "pt_converge.hpp"
#include "pt_adaptive.hpp"
#include "pt_lens.hpp"
#include "pt_lens_aov.hpp"
#include "pt_projection.hpp"
#include "pt_shutter.hpp"
#include "pt_launch.hpp"
#include "../host/sbvh_builder.hpp"
#include "../host/Camera.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <new>
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)
using namespace gmupt;

// ------------------------------------------------------------------------------------------------ errors
extern thread_local std::string g_lastError;                 // gmupt_capi.hip, what gmupt_last_error() returns
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(GMUPT_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)
#define GMUPT_TRY(expr) do { const int rc_ = (expr); if (rc_ != GMUPT_OK) return rc_; } while (0)   // for what has called fail() itself

// ------------------------------------------------------------------------------------------------ owners
// Device memory of one handle, freed with it.  Freeing does not wait for the stream: whoever lets go of memory a launch may still use
// synchronises first (grow() does, and so do the destroy functions, gmupt_resize, gmupt_temporal_reset and build_traversal_copy).
struct DevMem {
    void* ptr = nullptr; size_t bytes = 0; DevMem() = default;
    DevMem(DevMem&& o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr; o.bytes = 0; }
    DevMem& operator=(DevMem&& o) noexcept { std::swap(ptr, o.ptr); std::swap(bytes, o.bytes); return *this; }   // o frees what this held
    ~DevMem() { if (ptr) (void)hipFree(ptr); }
    template <class T> T* as() const { return static_cast<T*>(ptr); }
    // at least `need` bytes, kept between calls; the old contents are not kept when it grows
    int grow(hipStream_t s, size_t need)
    {
        if (bytes >= need) return GMUPT_OK;
        if (ptr) { HIP_TRY(hipStreamSynchronize(s)); HIP_TRY(hipFree(ptr)); ptr = nullptr; bytes = 0; }
        HIP_TRY(hipMalloc(&ptr, need));
        bytes = need;
        return GMUPT_OK;
    }
    // `n` bytes (16 at least) that s fills with `fill`; the owner keeps what it had when either step fails
    int alloc(size_t n, int fill, hipStream_t s)
    {
        DevMem m;
        m.bytes = n ? n : 16;
        HIP_TRY(hipMalloc(&m.ptr, m.bytes));
        HIP_TRY(hipMemsetAsync(m.ptr, fill, m.bytes, s));
        *this = std::move(m);
        return GMUPT_OK;
    }
};

// Pinned host memory of one handle (the staging area of a small per-call upload), freed with it
struct PinnedMem {
    void* ptr = nullptr; size_t bytes = 0; PinnedMem() = default;
    PinnedMem(const PinnedMem&) = delete; PinnedMem& operator=(const PinnedMem&) = delete;
    ~PinnedMem() { if (ptr) (void)hipHostFree(ptr); }
    template <class T> T* as() const { return static_cast<T*>(ptr); }
    int alloc(size_t n) { HIP_TRY(hipHostMalloc(&ptr, n ? n : 16, hipHostMallocDefault)); bytes = n ? n : 16; return GMUPT_OK; }
};

// N events of one handle, created on first use and destroyed with it
template <int N> struct DevEvents {
    hipEvent_t e[N] = {}; DevEvents() = default;
    DevEvents(DevEvents&& o) noexcept { for (int k = 0; k < N; k++) { e[k] = o.e[k]; o.e[k] = nullptr; } }
    ~DevEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    int create() { for (hipEvent_t& x : e) if (!x) HIP_TRY(hipEventCreate(&x)); return GMUPT_OK; }
};
struct EventPair : DevEvents<2> {   // the two ends of one timed span on a stream; elapsed_ms() after the stream was synchronised
    int start(hipStream_t s) { GMUPT_TRY(create()); HIP_TRY(hipEventRecord(e[0], s)); return GMUPT_OK; }
    int stop(hipStream_t s) { HIP_TRY(hipEventRecord(e[1], s)); return GMUPT_OK; }
    int elapsed_ms(float* ms) const { HIP_TRY(hipEventElapsedTime(ms, e[0], e[1])); return GMUPT_OK; }
};
struct StageEvents : DevEvents<5> { bool extOnly = false; };   // logic | material | ray cast (extension) | shadow

// ------------------------------------------------------------------------------------------------ handles
struct gmupt_device { int id; hipDeviceProp_t prop; };
struct gmupt_buffer { gmupt_device* dev; gmupt_buffer_kind kind; void* dptr; size_t bytes; size_t elems; uint32_t texSize = 0, texLayers = 0; };
struct gmupt_camera { Camera cam; gmupt_camera(uint32_t w, uint32_t h) : cam(w, h) {} };
struct gmupt_sbvh { gmupt::SbvhBuilder* b; };
struct gmupt_travtables { TravTables t; };

struct gmupt_adaptive;

enum TravTable { TT_NODES, TT_TRIS, TT_RECS, TT_WIDE, TT_PAIRS, TT_PAIRREF, TT_COUNT };   // the renderer's six device tables, in the order build_traversal_copy fills them

struct gmupt_renderer {
    gmupt_device* dev = nullptr;
    gmupt_renderer_desc desc{};
    hipStream_t stream = nullptr;
    RenderParams p{};                // the kernel argument: raw pointers into the owners below and into the bound buffers
    bool sceneBound = false, cameraSet = false;
    uint64_t iterations = 0;
    uint32_t travBlocks = 0;
    // timing
    int timing = 0; // 0 off, 1 all stages, 2 only the extension ray cast (two events per iteration)
    std::vector<StageEvents> evPool; size_t evUsed = 0;
    double msStage[4] = { 0, 0, 0, 0 }; uint64_t timedIters = 0;
    std::vector<DevMem> pool;        // path state, queues, counters, statistics: allocated by gmupt_renderer_create
    DevMem fb, listHead;             // the accumulation target (gmupt_resize replaces both)
    // packed traversal copy of the bound scene; DevMem::bytes is what was uploaded to each (gmupt_debug_read_travtable)
    DevMem trav[TT_COUNT];
    int travMode = 70; // GMUPT_TRAVERSAL: "wide" (default) both ray casts in one launch over the 4-wide collapse | "cast0" the same over the binary tree | "def0" separate launches; the other rungs of the ladder exist in -DGMUPT_VARIANTS builds only
    uint32_t castFlags = 0; // GMUPT_STAT_* bits of the ray-cast kernels launched since the last reset
    // ray queries (gmupt_trace_rays): work counters + statistics of their own, allocated on first use; one ray + one hit for gmupt_pick
    DevMem queryCounters, queryStats, pickBuf;
    EventPair queryEv;
    // AOV buffers (gmupt_render_aovs): rays and hits of one chunk (GMUPT_AOV_CHUNK_RAYS each, 128 MiB), allocated on first use
    DevMem aovRays, aovHits;
    // denoiser (gmupt_denoise_image): the filter's scratch (kGdScratchBytes per pixel) and, for gmupt_render_denoised, the AOV records and
    // the framebuffer copy (80 bytes per pixel); allocated on first use, grown when a larger image comes
    DevMem dnScratch, dnInput;
    EventPair dnEv;
    // infill (gmupt_infill_image): the stage's scratch (256 bytes of counters, then kGdScratchBytes per pixel) and, for the chained entry
    // points, the filled image the denoiser reads (16 bytes per pixel); allocated on first use, grown when a larger image comes
    DevMem ifScratch, ifImage;
    EventPair ifEv;
    // temporal reuse (gmupt_render_denoised_temporal): advanced by an iteration that clears the frame and by gmupt_resize (host only)
    uint64_t accumGeneration = 0;
    // motion (gmupt_render_denoised_temporal_motion): which binding the renderer has and how many refits it has seen (host only)
    uint64_t bindingId = 0, geomGeneration = 0;
    // refit (gmupt_renderer_refit): the buffers of the binding with their element counts, and what build_trav_tables (pt_travtables.hpp) knows about the
    // topology of its tables -- host vectors, uploaded into one allocation (rfDev) by the first refit after a bind
    const gmupt_buffer* boundNodes = nullptr; const gmupt_buffer* boundTris = nullptr; const gmupt_buffer* boundVerts = nullptr;
    const gmupt_buffer* boundProps = nullptr;   // normals (gmupt_normals_update): the property buffer of the binding
    size_t boundElems[3] = { 0, 0, 0 };
    std::vector<uint32_t> rfLevelNodes, rfLevelOff, rfNodeMap, rfWideMap, rfOpened;
    DevMem rfDev;
    EventPair rfEv;
    // tree cost (gmupt_renderer_tree_cost): the partial results of every level, 48 bytes per 256 records; allocated on first use, grown on demand
    DevMem tcScratch;
    EventPair tcEv;
    // adaptive sampling (gmupt_renderer_set_adaptive): the attached plan, not owned; null = every iteration launches what it always did
    gmupt_adaptive* adaptive = nullptr;
    // thin lens (gmupt_renderer_set_lens): aperture_radius 0 = none attached, every iteration launches what it always did
    gmupt_lens lens{ 0.0f, 1.0f };
    // camera projection (gmupt_renderer_set_projection): kind GMUPT_PROJ_PINHOLE = none attached, every iteration launches what it always did
    gmupt_projection projection{ GMUPT_PROJ_PINHOLE, 3.14159274f, 1.0f, 0u };
    // shutter (gmupt_renderer_set_shutter): the camera pose at shutter close; not attached = every iteration launches what it always did
    gmupt_shutter shutter{};
    bool shutterAttached = false;

    __attribute__((visibility("default"))) ~gmupt_renderer() { if (stream) (void)hipStreamDestroy(stream); }   // gmupt_renderer_destroy has synchronised it; the library has always exported this symbol
    uint32_t tile_x0() const { return p.tileEnabled ? p.tileX0 : 0u; } uint32_t tile_y0() const { return p.tileEnabled ? p.tileY0 : 0u; }   // the origin of the rendered rectangle
};

// one record set with the camera and rectangle it was made for
struct TpSlot {
    DevMem rec;
    bool present = false;
    gmupt_camera_buffer cam{};
    uint32_t x0 = 0, y0 = 0, W = 0, H = 0;
    // the vertex pose the records were written in (gmupt_render_denoised_temporal_motion only): a device copy of the bound vertex buffer
    DevMem verts;
    bool hasPose = false; uint64_t binding = 0, geomGeneration = 0; uint32_t numVerts = 0;
};

struct gmupt_temporal {
    gmupt_renderer* r = nullptr;
    TpSlot frozen, last;                        // history of earlier accumulations; the records of the latest call
    DevMem integrated;                          // the integrated image the spatial filter reads (16 bytes per pixel)
    bool seen = false; uint64_t generation = 0; // the renderer's accumulation generation at the last gmupt_render_denoised_temporal
    EventPair ev;
};

// (the builder and optimiser handles, gmupt_lbvh and gmupt_treeopt: gmupt_work.hpp)

// the adjacency of one index list for a renderer's vertices (gmupt_normals_*): device memory laid out by normals_layout (pt_normals.hip)
struct gmupt_normals {
    gmupt_renderer* r = nullptr;
    uint32_t numVerts = 0, numTris = 0, maxValence = 0;
    DevMem mem; NmLayout off{};
    EventPair ev;
};

// the rig of one mesh for a renderer's vertices (gmupt_pose_*): device memory laid out by pose_layout (pt_pose.hip), and the pinned
// staging area of gmupt_pose_update with the event that tells when the stream has read it
struct gmupt_pose {
    gmupt_renderer* r = nullptr;
    uint32_t numVerts = 0, influences = 0, numJoints = 0, numTargets = 0;
    DevMem mem; PsLayout off{};
    PinnedMem staging; DevEvents<1> staged; bool stagingBusy = false;
    EventPair ev;
};

// the convergence monitor of one renderer (gmupt_converge_*): the state planes and partial summaries of a W x H image in one
// allocation (converge_carve, pt_converge.hip), and which accumulation of the renderer the state belongs to
struct gmupt_converge {
    gmupt_renderer* r = nullptr;
    uint32_t W = 0, H = 0;
    DevMem mem; CvPlanes pl{};
    bool seen = false; uint64_t generation = 0;   // the renderer's accumulation generation at the last gmupt_converge_update
    EventPair ev;
};

// the sampling plan of one renderer (gmupt_adaptive_*): the list, the run totals and their offsets of a W x H rectangle in one
// allocation (adaptive_carve, pt_adaptive.hip), carved for `pixels` and `cap` entries; the error plane of gmupt_render_adaptive; which
// accumulation of the renderer the plan was made from
struct gmupt_adaptive {
    gmupt_renderer* r = nullptr;
    uint32_t W = 0, H = 0, count = 0, uniformEvery = 0;
    DevMem mem; AdScratch sc{}; size_t pixels = 0, cap = 0;
    DevMem errPlane;
    uint64_t generation = 0;
    EventPair ev;
};

// ------------------------------------------------------------------------------------------------ shared between units
size_t kind_stride(gmupt_buffer_kind k);                                                                        // gmupt_capi.hip
gmupt_buffer* buffer_alloc(gmupt_device* dev, gmupt_buffer_kind kind, size_t elems, size_t bytes, hipError_t* e);
int build_traversal_copy(gmupt_renderer* r, const gmupt_buffer* nodesB, const gmupt_buffer* trisB, const gmupt_buffer* vertsB);   // gmupt_capi_accel.hip
int query_supported(gmupt_renderer* r, const char* fn);                                                         // gmupt_capi_query.hip
int query_buffers(gmupt_renderer* r);                                                                           // one timed span of cast queries on the query's own counters and statistics
int query_begin(gmupt_renderer* r, RenderParams* q);
int query_end(gmupt_renderer* r, const char* fn, const char* what, gmupt_trace_info* info);
int pick_ray_hit(gmupt_renderer* r, const gmupt_ray& ray, uint32_t light_count, gmupt_ray* ray_out, gmupt_hit* hit_out);   // gmupt_pick on a ray already made
int aov_chunk_scratch(gmupt_renderer* r);                                                                       // the rays and hits of one AOV chunk, on first use
int denoise_params(const char* fn, const gmupt_denoise_params* p, DnParams& out);                               // gmupt_capi_host.cpp
int image_args(const char* fn, const void* beauty, const void* aov, uint32_t W, uint32_t H, const void* out, size_t bytes, bool device);
int temporal_params(const char* fn, const gmupt_temporal_params* p, DnParams& dn, TpParams& tp);
int infill_params(const char* fn, const gmupt_infill_params* p, IfParams& out);
int converge_params(const char* fn, const gmupt_converge_params* p, CvParams& out);
int adaptive_params(const char* fn, const gmupt_adaptive_params* p, float monitorThreshold, AdParams& out);   // threshold 0 = monitorThreshold
int lens_params(const char* fn, const gmupt_lens* lens);                                                         // the argument errors of include/gmupt_lens.h
int projection_params(const char* fn, const gmupt_projection* proj);                                             // gmupt_capi_projection.hip: those of include/gmupt_projection.h
// gmupt_capi_denoise.hip: the chains behind the temporal entry points; infill == nullptr is the chain without the infill stage
int temporal_denoise(const char* fn, gmupt_temporal* t, const float* beauty_rgba, const gmupt_aov* aov, const gmupt_motion* motion,
                     const gmupt_camera_buffer* cam, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, int new_accumulation,
                     const gmupt_temporal_params* p, const IfParams* infill, float* out_rgba, size_t out_bytes, float* ms);
// the guide records of render_denoised: empty = gmupt_render_aovs, with its centre ray; otherwise what renders the s*s-ray records of a
// lens or a projection (render_aov_chunks with centre = false) into (out, bytes) under the caller's name
using AovGuides = std::function<int(gmupt_aov* out, size_t bytes, gmupt_trace_info* info)>;
int render_denoised(const char* fn, gmupt_renderer* r, uint32_t aov_samples, const gmupt_denoise_params* p, const IfParams* infill, float* out_rgba, size_t bytes,
                    gmupt_trace_info* info, const AovGuides& guides = nullptr);
// gmupt_capi_query.hip: the AOV records of the renderer's rectangle, chunk by chunk of whole pixel rows on the chunk scratch, as one timed
// span of cast queries; every gmupt_render_aovs* is a call of it.  fn: the name in its errors; centre: the sample plan (aov_sample_plan).
// Per chunk: raygen writes c.rays, the wide ray cast fills c.hits, after_cast resolves them into the records of rows c.row .. + c.rows
struct AovRows { uint32_t row, rows, W, R; gmupt_ray* rays; gmupt_hit* hits; };
using AovStage = std::function<void(const AovRows& c)>;
int render_aov_chunks(const char* fn, gmupt_renderer* r, uint32_t samples, bool centre, gmupt_aov* out, size_t bytes, gmupt_trace_info* info,
                      const AovStage& raygen, const AovStage& after_cast);
int render_denoised_temporal(const char* fn, bool poses, gmupt_renderer* r, gmupt_temporal* t, uint32_t aov_samples, const gmupt_temporal_params* p,
                             const IfParams* infill, float* out_rgba, size_t bytes, gmupt_trace_info* info);
// gmupt_capi_infill.hip: grows the renderer's infill scratch for the image (the one place that does) and enqueues the stage
int enqueue_infill(gmupt_renderer* r, const float4* beauty, const float4* aov, uint32_t W, uint32_t H, const IfParams& prm, float4* out, const IfCounters** counts);
int lbvh_leaf_size(const char* fn, const gmupt_lbvh_params* params, uint32_t* L);
void lbvh_fill_info(gmupt_lbvh_info* info, const LbResult& res, uint32_t numTris, double ms);
int treeopt_passes(const char* fn, const gmupt_treeopt_params* params, uint32_t* passes);
void treeopt_fill_info(gmupt_treeopt_info* info, const ToResult& res, double ms);

// one copy on a stream, waited for
inline int copy_sync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s)
{
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, s)); HIP_TRY(hipStreamSynchronize(s)); return GMUPT_OK;
}

// DevStats::stackOverflow as the GMUPT_STAT_* bits of gmupt_stats::flags and gmupt_trace_info::flags
inline uint32_t cast_fault_flags(const DevStats& ds)
{
    return ((ds.stackOverflow & 1u) ? GMUPT_STAT_STACK_OVERFLOW : 0u) | ((ds.stackOverflow & 2u) ? GMUPT_STAT_CAST_ABORTED : 0u);
}

// The rays per pixel of an AOV sample plan in *R (if asked for), or what gmupt_render_aovs refuses: `what` is the caller's name for
// `samples`, W the width of a row (a chunk of GMUPT_AOV_CHUNK_RAYS rays holds whole rows; 0 where there is no row).  centre = false:
// the plan of the lens records (include/gmupt_lens_aov.h), s*s rays and no centre ray
inline int aov_sample_plan(const char* fn, const char* what, uint32_t W, uint32_t samples, uint32_t* R, bool centre = true)
{
    if (samples < 1 || samples > GMUPT_AOV_MAX_SAMPLES) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: %s = %u (1..%d)", fn, what, samples, GMUPT_AOV_MAX_SAMPLES);
    const uint32_t n = !centre ? samples * samples : samples == 1 ? 1u : samples * samples + 1u;
    if ((uint64_t)W * n > GMUPT_AOV_CHUNK_RAYS) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: one row of %u pixels is %u rays at %s = %u (at most 2^21)", fn, W, W * n, what, samples);
    if (R) *R = n;
    return GMUPT_OK;
}
#pragma GCC visibility pop
