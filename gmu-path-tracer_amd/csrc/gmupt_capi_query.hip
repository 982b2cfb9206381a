// C-ABI of libgmupt.so: ray queries on the bound scene and the AOV buffers made of them.
#include "gmupt_internal.hpp"

// ------------------------------------------------------------------------------------------------ ray queries
static_assert(sizeof(gmupt_ray) == 32 && offsetof(gmupt_ray, tmax) == 12 && offsetof(gmupt_ray, direction) == 16, "gmupt_ray layout");
static_assert(sizeof(gmupt_hit) == 32 && offsetof(gmupt_hit, triangle) == 12 && offsetof(gmupt_hit, light) == 16 && offsetof(gmupt_hit, material) == 20, "gmupt_hit layout");
static_assert(sizeof(gmupt_trace_info) == 24 && offsetof(gmupt_trace_info, redo_rays) == 8 && offsetof(gmupt_trace_info, ms) == 16, "gmupt_trace_info layout");

// the wide collapse and the limits of k_cast_w's 32-bit buffer offsets, the rule launch_cast_wide applies (gmupt_trace_rays, gmupt_render_aovs)
int query_supported(gmupt_renderer* r, const char* fn)
{
    const RenderParams& p = r->p;
    if (!p.trav.wnodes || p.extendPrune || p.shadowPrune)
        return fail(GMUPT_ERR_UNSUPPORTED, "%s: the bound scene has no wide collapse (it needs GMUPT_TRAVERSAL=wide, no GMUPT_EXTEND_PRUNE / GMUPT_SHADOW_PRUNE, "
                    "and child boxes inside their parents)", fn);
    if (!wide_tables_addressable(p.trav.wideCount, p.scene.numTris, p.trav.numPairs))
        return fail(GMUPT_ERR_UNSUPPORTED, "%s: the wide tables of the bound scene exceed 2 GiB (%u nodes, %u references, %u pairs)", fn, p.trav.wideCount, p.scene.numTris, p.trav.numPairs);
    return GMUPT_OK;
}

// the query's own work counters and statistics, on first use
int query_buffers(gmupt_renderer* r)
{
    HIP_TRY(hipSetDevice(r->dev->id));
    if (r->queryStats.ptr) return GMUPT_OK;
    GMUPT_TRY(r->queryCounters.alloc(128, 0, r->stream));
    return r->queryStats.alloc(sizeof(DevStats), 0, r->stream);
}

// One timed span of cast queries on the renderer's stream, behind whatever the renderer has queued: *q is the kernel argument of its
// launches, with the query's counters and statistics (the renderer's are left alone).  Zeroes the statistics, records the first event.
int query_begin(gmupt_renderer* r, RenderParams* q)
{
    *q = r->p;
    q->travCounters = r->queryCounters.as<uint32_t>(); q->stats = r->queryStats.as<DevStats>();
    HIP_TRY(hipMemsetAsync(q->stats, 0, sizeof(DevStats), r->stream));
    return r->queryEv.start(r->stream);
}

// Records the second event, waits for the span and fills *info; a launch that flagged its `what` (results, records) as invalid is fn's error.
int query_end(gmupt_renderer* r, const char* fn, const char* what, gmupt_trace_info* info)
{
    GMUPT_TRY(r->queryEv.stop(r->stream));
    DevStats ds;
    GMUPT_TRY(copy_sync(&ds, r->queryStats.ptr, sizeof(ds), hipMemcpyDeviceToHost, r->stream));
    float ms = 0.0f;
    GMUPT_TRY(r->queryEv.elapsed_ms(&ms));
    if (info) { info->flags = GMUPT_STAT_FUSED_CAST | GMUPT_STAT_CAST_WIDE | cast_fault_flags(ds); info->redo_rays = ds.castRedoRays; info->ms = ms; }
    if (ds.stackOverflow & 2u) return fail(GMUPT_ERR_CAST_FAULT, "%s: a wave of the ray cast left its loop at the iteration limit (GMUPT_STAT_CAST_ABORTED): the %s are invalid", fn, what);
    if (ds.stackOverflow & 1u) return fail(GMUPT_ERR_CAST_FAULT, "%s: a traversal stack overflowed (GMUPT_STAT_STACK_OVERFLOW): the %s are invalid", fn, what);
    return GMUPT_OK;
}

extern "C" int gmupt_trace_rays(gmupt_renderer* r, const gmupt_ray* closest, uint32_t n_closest, gmupt_hit* hits,
                                const gmupt_ray* any, uint32_t n_any, uint32_t* occluded, uint32_t light_count, gmupt_trace_info* info)
{
    if (info) std::memset(info, 0, sizeof(*info));
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_trace_rays: null renderer");
    if (!r->sceneBound) return fail(GMUPT_ERR_NOT_BOUND, "gmupt_trace_rays: no scene bound");
    constexpr uint32_t kMaxBatch = 1u << 26;
    if (n_closest > kMaxBatch || n_any > kMaxBatch) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_trace_rays: %u closest-hit / %u any-hit rays (at most 2^26 per batch)", n_closest, n_any);
    if (n_closest && (!closest || !hits)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_trace_rays: null closest-hit rays or hits");
    if (n_any && (!any || !occluded)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_trace_rays: null any-hit rays or occluded flags");
    if ((n_closest && (((uintptr_t)closest | (uintptr_t)hits) & 15u)) || (n_any && (((uintptr_t)any & 15u) || ((uintptr_t)occluded & 3u))))
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_trace_rays: misaligned pointer (rays and hits need 16 bytes, occluded flags 4)");
    GMUPT_TRY(query_supported(r, "gmupt_trace_rays"));
    GMUPT_TRY(query_buffers(r));
    if (n_closest == 0 && n_any == 0) { HIP_TRY(hipStreamSynchronize(r->stream)); if (info) info->flags = GMUPT_STAT_FUSED_CAST | GMUPT_STAT_CAST_WIDE; return GMUPT_OK; }
    HIP_TRY(hipMemsetAsync(r->queryCounters.ptr, 0, 128, r->stream));
    RenderParams q;
    GMUPT_TRY(query_begin(r, &q));
    launch_trace_wide(q, closest, n_closest, hits, any, n_any, occluded, light_count, r->stream);
    HIP_TRY(hipGetLastError());
    return query_end(r, "gmupt_trace_rays", "results", info);
}

extern "C" int gmupt_camera_pick_ray(const gmupt_camera_buffer* cam, float px, float py, gmupt_ray* out)
{
    if (!cam || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_camera_pick_ray: null argument");
    // newPath.hlsl:36-39 with the jitter at 0: (x + 0) * pixelSize is x * pixelSize for every float x
    store_ray(mk3(cam->position[0], cam->position[1], cam->position[2]), camera_ray_direction(*cam, px, py), out);
    return GMUPT_OK;
}

// the closest hit of one host ray through the renderer's pick buffer: what gmupt_pick and gmupt_pick_projected do with their ray
int pick_ray_hit(gmupt_renderer* r, const gmupt_ray& ray, uint32_t light_count, gmupt_ray* ray_out, gmupt_hit* hit_out)
{
    HIP_TRY(hipSetDevice(r->dev->id));
    if (!r->pickBuf.ptr) GMUPT_TRY(r->pickBuf.alloc(64, 0, r->stream));
    gmupt_ray* dRay = r->pickBuf.as<gmupt_ray>();
    gmupt_hit* dHit = (gmupt_hit*)(r->pickBuf.as<char>() + 32);
    HIP_TRY(hipMemcpyAsync(dRay, &ray, sizeof(ray), hipMemcpyHostToDevice, r->stream));
    GMUPT_TRY(gmupt_trace_rays(r, dRay, 1, dHit, nullptr, 0, nullptr, light_count, nullptr));
    GMUPT_TRY(copy_sync(hit_out, dHit, sizeof(*hit_out), hipMemcpyDeviceToHost, r->stream));
    if (ray_out) *ray_out = ray;
    return GMUPT_OK;
}

extern "C" int gmupt_pick(gmupt_renderer* r, float px, float py, uint32_t light_count, gmupt_ray* ray_out, gmupt_hit* hit_out)
{
    if (!r || !hit_out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_pick: null argument");
    if (!r->cameraSet) return fail(GMUPT_ERR_NOT_BOUND, "gmupt_pick: no camera set");
    if (!r->sceneBound) return fail(GMUPT_ERR_NOT_BOUND, "gmupt_pick: no scene bound");
    gmupt_ray ray;
    GMUPT_TRY(gmupt_camera_pick_ray(&r->p.cam, px, py, &ray));
    return pick_ray_hit(r, ray, light_count, ray_out, hit_out);
}

// ------------------------------------------------------------------------------------------------ AOV buffers
static_assert(sizeof(gmupt_aov) == 64 && offsetof(gmupt_aov, depth) == 12 && offsetof(gmupt_aov, normal) == 16 && offsetof(gmupt_aov, roughness) == 28 &&
              offsetof(gmupt_aov, position) == 32 && offsetof(gmupt_aov, metallic) == 44 && offsetof(gmupt_aov, triangle) == 48 &&
              offsetof(gmupt_aov, material) == 52 && offsetof(gmupt_aov, light) == 56 && offsetof(gmupt_aov, coverage) == 60, "gmupt_aov layout");
static_assert(sizeof(gmupt_motion) == 16 && offsetof(gmupt_motion, flags) == 12, "gmupt_motion layout");

extern "C" int gmupt_aov_ray(const gmupt_camera_buffer* cam, uint32_t x, uint32_t y, uint32_t samples, uint32_t k, gmupt_ray* out)
{
    if (!cam || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_aov_ray: null argument");
    uint32_t R;
    GMUPT_TRY(aov_sample_plan("gmupt_aov_ray", "samples", 0, samples, &R));
    if (k >= R) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_aov_ray: ray %u of %u", k, R);
    float px, py;
    aov_ray_coords(x, y, samples, k, px, py);
    return gmupt_camera_pick_ray(cam, px, py, out);
}

int aov_chunk_scratch(gmupt_renderer* r)
{
    if (!r->aovHits.ptr) {
        GMUPT_TRY(r->aovRays.alloc((size_t)GMUPT_AOV_CHUNK_RAYS * sizeof(gmupt_ray), 0, r->stream));
        GMUPT_TRY(r->aovHits.alloc((size_t)GMUPT_AOV_CHUNK_RAYS * sizeof(gmupt_hit), 0, r->stream));
    }
    return GMUPT_OK;
}

// The one chunk loop behind every gmupt_render_aovs* (gmupt_internal.hpp states the contract).  The order of the checks is part of it.
int render_aov_chunks(const char* fn, gmupt_renderer* r, uint32_t samples, bool centre, gmupt_aov* out, size_t bytes, gmupt_trace_info* info,
                      const AovStage& raygen, const AovStage& after_cast)
{
    if (info) std::memset(info, 0, sizeof(*info));
    if (!r->sceneBound) return fail(GMUPT_ERR_NOT_BOUND, "%s: no scene bound", fn);
    if (!r->cameraSet) return fail(GMUPT_ERR_NOT_BOUND, "%s: no camera set", fn);
    if (!out || ((uintptr_t)out & 15u)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null or misaligned output (16 bytes)", fn);
    const uint32_t W = r->p.fbW, H = r->p.fbH;
    uint32_t R;
    GMUPT_TRY(aov_sample_plan(fn, "samples", W, samples, &R, centre));
    if (bytes < (size_t)W * H * sizeof(gmupt_aov)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: %zu bytes for %ux%u records of 64 bytes", fn, bytes, W, H);
    GMUPT_TRY(query_supported(r, fn));
    GMUPT_TRY(query_buffers(r));
    GMUPT_TRY(aov_chunk_scratch(r));
    const uint32_t rowsPerChunk = GMUPT_AOV_CHUNK_RAYS / (W * R);   // >= 1: aov_sample_plan admitted the row
    RenderParams q;
    GMUPT_TRY(query_begin(r, &q));
    for (uint32_t row = 0; row < H; row += rowsPerChunk) {
        const AovRows c{ row, std::min(rowsPerChunk, H - row), W, R, r->aovRays.as<gmupt_ray>(), r->aovHits.as<gmupt_hit>() };
        raygen(c);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(q.travCounters, 0, 128, r->stream));
        launch_trace_wide(q, c.rays, c.rows * W * R, c.hits, nullptr, 0, nullptr, r->p.cam.lightCount, r->stream);
        HIP_TRY(hipGetLastError());
        after_cast(c);
        HIP_TRY(hipGetLastError());
    }
    return query_end(r, fn, "records", info);
}

// gmupt_render_aovs, and with motion != nullptr gmupt_render_aovs_motion: k_mv_resolve follows k_aov_resolve on every chunk's hits
static int render_aovs(gmupt_renderer* r, uint32_t samples, gmupt_aov* out, size_t bytes, gmupt_trace_info* info, const float* prevVerts, gmupt_motion* motion)
{
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_render_aovs: null renderer");
    return render_aov_chunks("gmupt_render_aovs", r, samples, true, out, bytes, info,
        [&](const AovRows& c) { launch_aov_raygen(r->p.cam, r->tile_x0(), r->tile_y0() + c.row, c.W, c.rows, samples, c.R, c.rays, r->stream); },
        [&](const AovRows& c) {
            launch_aov_resolve(r->p, c.rows * c.W, samples, c.R, c.rays, c.hits, out + (size_t)c.row * c.W, r->stream);
            if (motion) launch_mv_resolve(r->p.scene, prevVerts, c.rows * c.W, c.R, c.hits, out + (size_t)c.row * c.W, motion + (size_t)c.row * c.W, r->stream);
        });
}

extern "C" int gmupt_render_aovs(gmupt_renderer* r, uint32_t samples, gmupt_aov* out, size_t bytes, gmupt_trace_info* info)
{
    if (info) std::memset(info, 0, sizeof(*info));
    return render_aovs(r, samples, out, bytes, info, nullptr, nullptr);
}

extern "C" int gmupt_render_aovs_motion(gmupt_renderer* r, uint32_t samples, const float* prev_verts, uint32_t num_verts, gmupt_aov* aov_out, size_t aov_bytes,
                                        gmupt_motion* motion_out, size_t motion_bytes, gmupt_trace_info* info)
{
    const char* fn = "gmupt_render_aovs_motion";
    if (info) std::memset(info, 0, sizeof(*info));
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null renderer", fn);
    if (!r->sceneBound) return fail(GMUPT_ERR_NOT_BOUND, "%s: no scene bound", fn);
    if (!prev_verts || ((uintptr_t)prev_verts & 3u)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null or misaligned previous vertices (4 bytes)", fn);
    if (!motion_out || ((uintptr_t)motion_out & 15u)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null or misaligned motion output (16 bytes)", fn);
    if (num_verts != r->p.scene.numVerts) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: %u previous vertices, the bound buffer holds %u", fn, num_verts, r->p.scene.numVerts);
    if (motion_bytes < (size_t)r->p.fbW * r->p.fbH * sizeof(gmupt_motion))
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: %zu bytes for %ux%u records of 16 bytes", fn, motion_bytes, r->p.fbW, r->p.fbH);
    return render_aovs(r, samples, aov_out, aov_bytes, info, prev_verts, motion_out);
}
