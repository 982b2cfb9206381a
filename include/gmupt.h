/*
 * include/gmupt.h -- C-ABI of the MI355X-native wavefront path tracer (libgmupt.so).
 *
 * This is the drop-in boundary for the hot path of WildBitangent/GMU-Path-Tracer:
 * it replaces the D3D11 / NVAPI calls inside the reference's Renderer and Scene
 * (there is no FFI layer in the reference; the boundary is the set of D3D11 calls
 * listed per entry point below).  All citations are relative to the reference tree.
 * Plain C, POD arguments, no HIP / torch types in any signature.
 *
 * Conventions
 *   - every function returns GMUPT_OK (0) or a negative gmupt_status;
 *     gmupt_last_error() returns a thread-local description of the last failure
 *     (reference: HRESULT != S_OK -> std::runtime_error(fmt::format(..)),
 *      Source/Renderer.cpp:286-297,424-429,484-497; the C++ wrappers in
 *      gmu-path-tracer_amd/host re-throw std::runtime_error);
 *   - creator owns, explicit *_destroy (reference: uni::UniqueHandle<T>::Release,
 *     Include/UniqueDX11.hpp:7-91); uploads copy, the caller may free at once;
 *   - *_create / upload functions are thread-safe per device (reference creates
 *     buffers from a BVH worker and 3 texture workers concurrently,
 *     Source/Scene.cpp:89,153-155); per-renderer functions are single-threaded;
 *   - gmupt_iterate() enqueues on the renderer's HIP stream and does not
 *     synchronise with the host (reference: Renderer::draw never reads back).
 */
#ifndef GMUPT_H
#define GMUPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GMUPT_MAX_LIGHTS 128    /* Include/Constants.hpp:15 MAX_LIGHTS (also the material cbuffer size, logic.hlsl:8) */
#define GMUPT_PATHCOUNT (1u << 21) /* Include/Constants.hpp:13 */
#define GMUPT_REF_GRID_THREADS (34u * 8u * 256u) /* NUM_SM*8 groups x NUM_THREADS, Constants.hpp:12-16 */
#define GMUPT_STATE_BYTES 248u  /* bytes per path of the reference path-state buffer, Source/Renderer.cpp:71 */

typedef enum {
    GMUPT_OK = 0,
    GMUPT_ERR_INVALID_ARGUMENT = -1,
    GMUPT_ERR_HIP = -2,          /* a HIP runtime call failed (no GPU, out of memory, launch failure) */
    GMUPT_ERR_OUT_OF_MEMORY = -3,
    GMUPT_ERR_NOT_BOUND = -4,    /* renderer used before a scene / camera was bound */
    GMUPT_ERR_UNSUPPORTED = -5,
    GMUPT_ERR_IO = -6,
    GMUPT_ERR_CAST_FAULT = -7    /* a ray-cast launch flagged its own results as invalid (GMUPT_STAT_STACK_OVERFLOW or GMUPT_STAT_CAST_ABORTED): returned by every
                                    call that hands out or waits for a frame -- gmupt_synchronize, gmupt_read_framebuffer, gmupt_copy_framebuffer_to_device,
                                    gmupt_get_stats (the statistics are still filled in), gmupt_render_budget -- until gmupt_reset_stats; the C++ Renderer throws,
                                    like the reference on a failed device call (Source/Renderer.cpp:286-297) */
} gmupt_status;

/* ---- POD layouts shared with the reference (sizes are static_assert'ed in the implementation) ---- */

/* Include/BVHWrapper.hpp:13-21 == Assets/Shaders/structs.h:182-194; 48 bytes.
 * inner node: children at left/right with right == left + 1 (Source/BVHWrapper.cpp:87-91);
 * leaf: [left, right) is a range of the triangle array. */
typedef struct { float min[3]; float pad0; float max[3]; float pad1; int32_t left; int32_t right; int32_t isLeaf; float pad2; } gmupt_bvh_node;
/* Include/BVHWrapper.hpp:23-27 == structs.h:196-200; 16 bytes, one per SBVH reference */
typedef struct { int32_t v[3]; uint32_t materialID; } gmupt_triangle;
/* Include/BVHWrapper.hpp:29-34 == structs.h:202-210; 32 bytes, one per VERTEX */
typedef struct { float normal[3]; float pad0; float uv[2]; uint32_t materialID; float pad1; } gmupt_tri_props;
/* Include/Scene.hpp:13-19 == structs.h:155-161; 32 bytes */
typedef struct { float position[3]; float falloff; float emission[3]; float radius; } gmupt_light;
/* Include/Scene.hpp:43-68 == structs.h:219-233; 48 bytes */
typedef struct { float color[4]; float metallic; float roughness; float refractIndex; float transmittance; int32_t textureIndices[3]; uint32_t materialType; } gmupt_material;
/* Include/Camera.hpp:8-22 == structs.h:163-180; 112 bytes, uploaded every frame (Source/Renderer.cpp:161) */
typedef struct {
    float position[4]; float upperLeftCorner[4]; float horizontal[4]; float vertical[4];
    float pixelSize[2]; float randomSeed[2]; float envColor[4];
    int32_t iterationCounter; uint32_t lightCount; uint32_t sampleLights; uint32_t pad_;
} gmupt_camera_buffer;

enum { GMUPT_MATERIAL_UE4 = 0, GMUPT_MATERIAL_GLASS = 1 }; /* Scene.hpp:53-57 */

/* ---- device ---- */
typedef struct gmupt_device gmupt_device;
/* replaces Renderer::createDevice (Source/Renderer.cpp:252-301): selects a HIP device (one process per GPU) */
int gmupt_device_create(int hip_device, gmupt_device** out);
void gmupt_device_destroy(gmupt_device* dev);
const char* gmupt_last_error(void);
/* number of visible HIP devices, or a negative status (does not initialise a context) */
int gmupt_device_count(void);

/* ---- scene resources ---- */
typedef enum {
    GMUPT_BUFFER_BVH_NODES = 0,  /* 48 B elements; Scene.cpp:174 mBVHBuffer  (t0) */
    GMUPT_BUFFER_TRIANGLES = 1,  /* 16 B;          Scene.cpp:175 mIndexBuffer (t1) */
    GMUPT_BUFFER_VERTICES = 2,   /* 12 B float3;   Scene.cpp:176 mVertexBuffer (t2) */
    GMUPT_BUFFER_LIGHTS = 3,     /* 32 B x <=128;  Scene.cpp:305-329 mLightBuffer (t3); zero-padded to 128 entries */
    GMUPT_BUFFER_TRI_PROPS = 4,  /* 32 B;          Scene.cpp:177 mTriangleProperties (t4) */
    GMUPT_BUFFER_MATERIALS = 5,  /* 48 B x <=128;  Scene.cpp:194-207 mMaterialPropertyBuffer (b1) */
    GMUPT_BUFFER_TEXTURE_ARRAY = 6 /* R8G8B8A8_UNORM Texture2DArray, square layers; created with gmupt_texture_array_create */
} gmupt_buffer_kind;

typedef struct gmupt_buffer gmupt_buffer;
/* replaces createBuffer<T> (Include/Util.hpp:17-43) + ID3D11Device::CreateBuffer with initial data */
int gmupt_buffer_create(gmupt_device* dev, gmupt_buffer_kind kind, const void* data, size_t bytes, gmupt_buffer** out);
/* replaces the light-buffer re-upload of the GUI (Source/GUI.cpp:125-130): UpdateSubresource on an existing buffer.
 * After updating node / triangle / vertex buffers call gmupt_renderer_bind_scene again (it rebuilds the traversal copy); when only vertex
 * POSITIONS changed (same count, same triangle records), gmupt_renderer_refit does instead, without the host round trip. */
int gmupt_buffer_update(gmupt_buffer* buf, const void* data, size_t bytes);
/* synchronous device-to-host copy of the first `bytes` bytes of a buffer (bytes <= gmupt_buffer_size), after the device has finished */
int gmupt_buffer_read(const gmupt_buffer* buf, void* dst, size_t bytes);
void gmupt_buffer_destroy(gmupt_buffer* buf);
size_t gmupt_buffer_size(const gmupt_buffer* buf);
/* replaces Scene::createTextures (Source/Scene.cpp:247-303): `layers` square RGBA8 images of `size` x `size` texels, tightly packed
 * (the caller has already resized every layer to the common size, as the reference does with avir) */
int gmupt_texture_array_create(gmupt_device* dev, const uint8_t* rgba8, uint32_t size, uint32_t layers, gmupt_buffer** out);

/* Host-side image helpers for the texture path (no device work).
 * gmupt_image_decode_png replaces lodepng::decode(out, w, h, file) (Source/Scene.cpp:226): PNG file bytes -> tightly packed RGBA8;
 * *rgba is allocated by the library, release it with gmupt_image_free.
 * gmupt_image_resize_square replaces avir::CImageResizer<fpclass_float8_dil>(8)::resizeImage(src, n, n, 0, dst, m, m, 4, 0) on square RGBA8
 * layers (Scene.cpp:269-279): the same bytes as avir 2.4 (Include/avir/avir.h) for every size pair, pinned against avir compiled from the
 * reference tree (tests/golden/texture_ref.npz); equal sizes run avir's filters too, they are not a copy.  dst holds new_size * new_size * 4 bytes.
 * gmupt_texture_common_size is the reference's size rule (Scene.cpp:232-241): median of the DISTINCT layer byte sizes -> width. */
int gmupt_image_decode_png(const void* png, size_t bytes, uint32_t* width, uint32_t* height, uint8_t** rgba);
void gmupt_image_free(uint8_t* rgba);
int gmupt_image_resize_square(const uint8_t* rgba, uint32_t old_size, uint32_t new_size, uint8_t* dst);
uint32_t gmupt_texture_common_size(const size_t* layer_bytes, uint32_t layers);

/* ---- renderer ---- */
typedef struct {
    uint32_t width, height;      /* accumulation target (== tile size when tile_enabled); createRenderTexture, Renderer.cpp:110-142 */
    uint32_t pool_paths;         /* PATHCOUNT; 0 -> GMUPT_PATHCOUNT (Renderer.cpp:71,78) */
    uint32_t live_paths;         /* slots the stage loops reach; 0 -> pool_paths.
                                    Reference value: (pool/GMUPT_REF_GRID_THREADS)*GMUPT_REF_GRID_THREADS (quirk: ITERATIONS = 30) */
    /* extensions of this build; all zero = reference behaviour */
    uint32_t tile_enabled, tile_x0, tile_y0; /* multi-GPU: generate paths for this tile of the full frame only */
    uint32_t path_budget;        /* stop regenerating after this many paths (0 = progressive, never stops) */
    uint32_t max_depth;          /* terminate at this path length (0 = unbounded, the reference) */
    uint32_t collect_stats;      /* 1: traverse kernels also count inner-node visits / triangle tests (slower) */
} gmupt_renderer_desc;

typedef struct gmupt_renderer gmupt_renderer;
/* replaces Renderer::createBuffers + createRenderTexture (Renderer.cpp:58-142): path state, queues, counters, accumulation target (zero-filled) */
int gmupt_renderer_create(gmupt_device* dev, const gmupt_renderer_desc* desc, gmupt_renderer** out);
void gmupt_renderer_destroy(gmupt_renderer* r);
/* replaces CSSetShaderResources / CSSetConstantBuffers(b1) of Renderer::draw (Renderer.cpp:166-192).
 * The buffers must outlive the binding.  Builds the renderer's internal traversal copy of the BVH. */
int gmupt_renderer_bind_scene(gmupt_renderer* r, const gmupt_buffer* nodes, const gmupt_buffer* triangles, const gmupt_buffer* vertices,
                              const gmupt_buffer* lights, const gmupt_buffer* tri_props, const gmupt_buffer* materials);
/* replaces the t5..t7 / s0 slots of CSSetShaderResources + CSSetSamplers (Renderer.cpp:173-175,192): diffuse, metallicRoughness and
 * normal Texture2DArrays, each may be NULL (an unbound slot reads zero).  Sampling is bilinear + wrap at mip 0 on UNORM8 without sRGB
 * decode, as the reference's sampler (Scene.cpp:180-192); the filter arithmetic is stated in DESIGN.md. */
int gmupt_renderer_bind_textures(gmupt_renderer* r, const gmupt_buffer* diffuse, const gmupt_buffer* metallic_roughness, const gmupt_buffer* normals);
/* replaces UpdateSubresource(mCameraBuffer) (Renderer.cpp:161).  iterationCounter == 0 resets the accumulation on the next iterate. */
int gmupt_set_camera(gmupt_renderer* r, const gmupt_camera_buffer* cam);
/* replaces the six Dispatch(NUM_GROUPS,1,1) of Renderer::draw (Renderer.cpp:195-211): one wavefront iteration, asynchronous */
int gmupt_iterate(gmupt_renderer* r);
/* replaces Renderer::resize -> createRenderTexture (Renderer.cpp:408-413): new zeroed accumulation target */
int gmupt_resize(gmupt_renderer* r, uint32_t width, uint32_t height);
/* replaces captureScreen's staging copy + Map (Renderer.cpp:355-381): synchronous readback of width*height RGBA32F (a = sample count bits) */
int gmupt_read_framebuffer(gmupt_renderer* r, float* rgba, size_t bytes);
/* device-to-device copy of the accumulation target into caller-owned device memory (e.g. a torch tensor) on the renderer's stream,
 * followed by a stream synchronise -- used by the multi-GPU tile gather */
int gmupt_copy_framebuffer_to_device(gmupt_renderer* r, void* device_dst, size_t bytes);
/* the 8 queue counters (structs.h:62-68; [7] = live extension-queue entries), synchronous */
int gmupt_get_counters(gmupt_renderer* r, uint32_t out[8]);
int gmupt_synchronize(gmupt_renderer* r);

#define GMUPT_STAT_STACK_OVERFLOW 1u /* a traversal stack exceeded 64 entries (results invalid; never seen on a builder-made tree) */
#define GMUPT_STAT_FUSED_CAST 2u     /* both ray casts ran as one launch: ms_extend is the time of that launch, ms_shadow is 0 */
#define GMUPT_STAT_CAST_FETCH 4u     /* that launch was k_cast_f (the default kernel; it needs node / triangle arrays below 2 GiB each) */
#define GMUPT_STAT_CAST_ABORTED 16u  /* a wave of the fused ray cast left its loop at the iteration limit (2^20 loop iterations; a bench-scene wave runs
                                        ~150): a defect, results invalid -- the kernel ends whatever happens */
#define GMUPT_STAT_CAST_WIDE 32u     /* that launch was k_cast_w: the walk over the 4-wide collapse of the tree (GMUPT_TRAVERSAL=wide) */
#define GMUPT_STAT_STACK_SPILL 8u    /* the tree is deeper than the LDS part of the traversal stacks: the instantiation with the bounds-checked
                                        global spill ran (results are the same; GMUPT_STAT_STACK_OVERFLOW is the error flag) */
typedef struct {
    uint64_t iterations;
    uint64_t paths_generated;    /* new paths started (device counter) */
    uint64_t paths_completed;    /* paths accumulated into the framebuffer */
    uint64_t segments;           /* live-slot iterations (the reference overlay's "MP/s" unit, GUI.cpp:48) */
    uint32_t active_paths;       /* slots not retired by path_budget */
    uint32_t flags;              /* GMUPT_STAT_* bits; the ray-cast bits describe the launches since the last gmupt_reset_stats */
    /* collect_stats only */
    uint64_t ext_rays, ext_inner, ext_leaves, ext_tris;
    uint64_t sh_rays, sh_inner, sh_leaves, sh_tris;
    /* device time per stage group in ms, accumulated since the last reset (HIP events on the renderer's stream; timing must be enabled) */
    double ms_logic, ms_scan, ms_accumulate, ms_material, ms_extend, ms_shadow; /* ms_scan and ms_accumulate are always 0: the queue ranks
                                    are computed inside the logic / material kernels and the accumulation inside the material kernel */
    uint64_t timed_iterations;
    /* collect_stats only: wave-level loop iterations of the ray casts; SIMD efficiency = lane steps / (64 * wave iterations) */
    uint64_t ext_wave_inner, ext_wave_tris, sh_wave_inner, sh_wave_tris;
    uint64_t ext_depth_hist[32]; /* inner-node visits of the extension rays by node depth */
    /* collect_stats with the fused ray cast (GMUPT_STAT_FUSED_CAST) only */
    uint64_t lane_census[4];          /* lane-iterations: no ray / walking / holding a leaf for a full FIFO / walk done, leaves pending */
    uint64_t cast_waves, cast_wave_ticks, cast_wave_ticks_max; /* wave lifetimes in wall-clock ticks: count, sum, maximum */
    uint64_t cast_drain_ticks, cast_drain_iters, cast_drain_busy_lanes; /* after a wave found both queues empty: ticks, loop iterations, busy lanes summed over them */
    uint64_t cast_wave_end_hist[32];  /* wave lifetimes in 50-us buckets */
    uint64_t ray_inner_hist[32];      /* extension rays by inner nodes visited, 16 per bucket */
    uint64_t ext_top_inner, sh_top_inner; /* inner-node visits served by the LDS-resident top of the tree (k_cast_f, collect_stats) */
    uint64_t cast_helper_subtrees;        /* deferred subtrees walked by a finished lane for a lane still walking, in the drain of k_cast_f (collect_stats) */
    uint64_t cast_nested_helpers;         /* of those: subtrees a helper lane gave away in turn (collect_stats) */
    uint64_t cast_redo_rays;              /* wide ray cast: rays walked again in the reference's binary order (their closest hit was an exact tie in t between
                                             two triangles, or a traversal stack ran full) */
    uint64_t wide_nodes, wide_top_nodes, wide_stack_bound; /* the 4-wide collapse of the bound scene (GMUPT_TRAVERSAL=wide; 0 when none was built): 128-byte records,
                                             how many of them live in LDS, and the most entries the inner stack of a walk could hold (every slot hit on every level) */
    uint64_t wide_pairs, wide_pair_fetches; /* the leaves of that collapse as 80-byte triangle-pair records: how many there are; how many were fetched (collect_stats) */
    uint64_t wide_box_tests;              /* wide ray cast, collect_stats: occupied box slots tested */
    uint64_t wide_iterations, wide_general_iterations; /* wide ray cast, collect_stats: iterations of a wave (six steps each); of those: with the general slab test
                                             (a ray of the wave has an infinite or NaN 1 / d component: near / far plane not known from the sign) */
} gmupt_stats;
int gmupt_get_stats(gmupt_renderer* r, gmupt_stats* out); /* synchronises */
int gmupt_reset_stats(gmupt_renderer* r);
int gmupt_enable_timing(gmupt_renderer* r, int mode); /* hipEvent timing on the renderer's stream: 0 off (default), 1 every stage group, 2 only the extension ray cast */

/* render until path_budget paths have completed (desc.path_budget must be > 0).  Every frame does what the reference's
 * Window::loop does (Source/Window.cpp:86-87): Camera::update (new randomSeed pair, iterationCounter++), upload, iterate.
 * The drain check reads one device word every 8 iterations; the loop ends when no slot is active, or 512 iterations after the budget
 * ran out (2.5 x the ~205-iteration life of a healthy path; what is still alive then are the reference's NaN-throughput paths, which
 * end only when their ray happens to hit a light).  Returns the iterations run in *iters. */
typedef struct gmupt_camera gmupt_camera;
int gmupt_render_budget(gmupt_renderer* r, gmupt_camera* camera, uint32_t max_iterations, uint32_t* iters);

/* ---- ray queries: the wide ray cast (k_cast_w) on rays the caller supplies ----
 * One launch serves a batch of closest-hit rays and a batch of any-hit rays (either may be empty), with the traversal, the tie handling
 * and the arithmetic of the renderer's own ray cast: the answers are bit for bit what extensionRayCast.hlsl / shadowRayCast.hlsl give.
 *
 * Closest hit (extensionRayCast.hlsl:64-74,168-194): `distance` starts at tmax; a triangle counts if t >= 0 && t < distance (strict: among
 *   hits with bitwise equal t the reference's binary near-first order decides).  t is in units of |direction| (it need not be normalised).
 *   After the triangles the first light_count light spheres are tested; a sphere with 0 < t < distance sets `light` and `t`, while
 *   triangle / u / v / material still describe the nearest triangle.  On a miss of everything: t = tmax, triangle = -1, u = v = 0,
 *   light = material = 0.  With tmax = FLT_MAX the record is the reference's (hitDistance, baryCoord.yz, triangle, isEmitter).
 * Any hit (shadowRayCast.hlsl:41-45,89): occluded = 1 if some triangle has 1e-8 < t < 1e8 (EPSILON = 1e-8, structs.h:10) and
 *   |direction * t| < tmax -- tmax plays the reference's lightDistance; the light spheres are not tested.
 * Degenerate rays (tests/test_degenerate_rays_gpu.py asserts each sentence): rays are NOT validated.  Every bit pattern of origin, direction
 *   and tmax -- NaN, infinities, signed zeros, denormals (kept, never flushed), huge magnitudes -- gets the record the rules above give in
 *   binary32, comparisons with a NaN being false; it never faults, and it does not change the record of any other ray of the batch.
 *   A NaN or an infinity in one component of the origin or of the direction, a direction of all zeros (either sign), a direction scaled
 *   by 1e-30 (every determinant falls below EPSILON) or an origin 1e20 away is a miss of every triangle: the miss record / occluded = 0.
 *   A zero (either sign) or denormal direction component alone is an ordinary ray.
 *   tmax of a closest-hit ray, from `t >= 0 && t < distance` with distance starting at tmax:
 *     tmax <= 0 (-0.0 included) or NaN: no t passes, neither a triangle's nor a light sphere's: the miss record, with t = the bits of tmax;
 *     tmax = +inf: every hit that tmax = FLT_MAX accepts, with the same t, u, v, triangle, light and material; a miss has t = +inf.
 *   tmax of an any-hit ray, from `|direction * t| < tmax`:
 *     tmax <= 0 or NaN: occluded = 0 (a length is never below it);
 *     tmax = +inf: no distance limit -- any triangle with 1e-8 < t < 1e8 and a finite |direction * t| occludes.
 * Calling: rays and outputs are caller-owned DEVICE memory (hipMalloc, torch tensors), 16-byte aligned (occluded: 4); at most 2^26 rays per
 *   batch.  The call is enqueued on the renderer's stream behind any pending gmupt_iterate work, then synchronises and reads back its own
 *   fault flags: GMUPT_ERR_CAST_FAULT on a traversal stack overflow or an aborted wave (the outputs are then invalid).  The renderer's path
 *   state, queues, counters, framebuffer and gmupt_get_stats are not touched (the query has its own work counters and statistics).
 * Errors: GMUPT_ERR_NOT_BOUND without a scene; GMUPT_ERR_INVALID_ARGUMENT for a NULL or misaligned pointer of a non-empty batch or more
 *   than 2^26 rays; GMUPT_ERR_UNSUPPORTED when the bound scene has no usable wide collapse (GMUPT_TRAVERSAL other than wide, the opt-in
 *   GMUPT_EXTEND_PRUNE / GMUPT_SHADOW_PRUNE, a tree whose child boxes stick out of their parents, or tables beyond the 2 GiB limits of
 *   32-bit buffer offsets). */
typedef struct { float origin[3]; float tmax; float direction[3]; uint32_t pad; } gmupt_ray;   /* 32 bytes; pad is ignored */
typedef struct {
    float t, u, v;
    int32_t triangle;   /* reference index into the GMUPT_BUFFER_TRIANGLES array, -1: no triangle below tmax.  Of the references with the same
                           record (a triangle that spatial splits put into several leaves) always the lowest index: they tie, and the order in
                           which the parallel walk meets them would otherwise decide */
    uint32_t light;     /* 0, or 1 + index of a light sphere nearer than every triangle (the reference's isEmitter) */
    uint32_t material;  /* materialID of that triangle record (0 without a triangle) */
    uint32_t pad[2];
} gmupt_hit;            /* 32 bytes */
typedef struct {
    uint32_t flags;     /* GMUPT_STAT_* of the launch: GMUPT_STAT_FUSED_CAST | GMUPT_STAT_CAST_WIDE, plus the fault bits */
    uint32_t pad_;
    uint64_t redo_rays; /* rays walked again in the reference's binary order (exact ties in t, or a full stack) */
    double ms;          /* device time of the launch (hipEvents on the renderer's stream) */
} gmupt_trace_info;     /* 24 bytes */
int gmupt_trace_rays(gmupt_renderer* r, const gmupt_ray* closest, uint32_t n_closest, gmupt_hit* hits,
                     const gmupt_ray* any, uint32_t n_any, uint32_t* occluded, uint32_t light_count, gmupt_trace_info* info /* may be NULL */);
/* host only: the un-jittered primary ray of newPath.hlsl:36-39 (jitter 0) through whole-frame pixel coordinates (px, py) of the camera --
 * origin = position, direction = normalize(upperLeftCorner + horizontal * (px * pixelSize.x) - vertical * (py * pixelSize.y)),
 * tmax = FLT_MAX.  Tile renderers share the whole frame's camera, so the same coordinates hold in tile mode. */
int gmupt_camera_pick_ray(const gmupt_camera_buffer* cam, float px, float py, gmupt_ray* out);
/* picking: gmupt_camera_pick_ray on the renderer's current camera, then a one-ray closest-hit gmupt_trace_rays (synchronous).
 * GMUPT_ERR_NOT_BOUND also when no camera was set.  ray_out may be NULL. */
int gmupt_pick(gmupt_renderer* r, float px, float py, uint32_t light_count, gmupt_ray* ray_out, gmupt_hit* hit_out);

/* ---- AOV buffers: the per-pixel G-buffer of the camera rays (albedo, normal, depth, position, ids) ----
 * One 64-byte gmupt_aov record per pixel of the renderer's framebuffer rectangle (the tile in tile mode), row-major, for a denoiser's guide
 * images, compositing and masks.  The hit shading is the renderer's own (the setMaterialHitProperties code of k_logic, logic.hlsl:79-133):
 * every value below is bit for bit what the logic stage computes for the same ray.
 *
 * Rays: samples = s in 1..8.  Pixel (x, y) in whole-frame coordinates (tile origin added) has R = 1 (s = 1) or s*s + 1 rays:
 *   k = 0            the centre ray, bit for bit gmupt_camera_pick_ray(cam, x, y);
 *   k = 1 + b*s + a  (a, b in 0..s-1, s > 1) the stratified ray through ((float)x + o(a), (float)y + o(b)), o(i) = (float)(2*i + 1) / (float)s - 1.0f,
 *                    which spans newPath's jitter range [-1, 1] (newPath.hlsl:36-37): the filtered planes share the beauty image's pixel filter.
 *   gmupt_aov_ray returns exactly these rays (host only).
 * Per ray, the closest hit with the light spheres up to the camera's lightCount (the renderer's extension cast):
 *   triangle hit, no nearer light: albedo / metallic / roughness / normal = what k_logic writes to matColor, matMR, normal for that ray --
 *                                  texture samples, the normal map (oriented by the ray direction), the normal not renormalised;
 *   light sphere nearer:           albedo = emission / max(emission) (sampleLight, logic.hlsl:192-197); normal, metallic, roughness 0;
 *   miss:                          albedo = cam.envColor.rgb; normal, metallic, roughness 0.
 * Filtered planes (albedo, normal): s = 1 the centre ray's values; s > 1 per component sum = 0.0f, then += the s*s stratified values in k
 *   order, then sum / (float)(s*s).  Every other field is the centre ray's.
 * Calling: `out` is caller-owned DEVICE memory, 16-byte aligned, bytes >= width * height * 64.  The call is enqueued on the renderer's stream
 *   behind pending gmupt_iterate work and synchronises; it reads back its own fault flags (GMUPT_ERR_CAST_FAULT as gmupt_trace_rays).  The
 *   frame, path state, queues, counters and gmupt_get_stats are not touched (the ray-query counters and statistics are used).  The rays are
 *   cast in chunks of whole pixel rows of at most 2^21 rays; the scratch of one chunk (64 MiB of rays, 64 MiB of hits) is allocated on the
 *   first call and kept until gmupt_renderer_destroy, whatever the image size or s.
 * Errors: GMUPT_ERR_NOT_BOUND without a scene or a camera; GMUPT_ERR_INVALID_ARGUMENT for a NULL or misaligned out, too few bytes, samples
 *   outside 1..8, or one row of more than 2^21 rays (width * R); GMUPT_ERR_UNSUPPORTED where gmupt_trace_rays returns it.  info (may be
 *   NULL): flags and redo_rays summed over the chunks, ms = device time of the whole call. */
typedef struct {
    float albedo[3];   float depth;       /* depth = t of the centre ray (FLT_MAX on a miss) */
    float normal[3];   float roughness;   /* roughness after max(0.014, .) (logic.hlsl:126), centre ray */
    float position[3]; float metallic;    /* position = o + d * t of the centre ray (surfacePoint of finish_extension_ray); 0 on a miss */
    int32_t triangle; uint32_t material; uint32_t light; uint32_t coverage;   /* triangle / material / light exactly as gmupt_hit of the centre ray;
                                                                                  coverage = filtered samples that hit a triangle and no light */
} gmupt_aov;           /* 64 bytes */
#define GMUPT_AOV_MAX_SAMPLES 8
#define GMUPT_AOV_CHUNK_RAYS (1u << 21)
int gmupt_render_aovs(gmupt_renderer* r, uint32_t samples, gmupt_aov* out, size_t bytes, gmupt_trace_info* info /* may be NULL */);
/* host only: ray k (0 .. R-1) of whole-frame pixel (x, y) at `samples` = s, as stated above; tmax = FLT_MAX */
int gmupt_aov_ray(const gmupt_camera_buffer* cam, uint32_t x, uint32_t y, uint32_t samples, uint32_t k, gmupt_ray* out);

/* ---- denoiser: edge-avoiding a-trous wavelet filter guided by the AOV buffers (Dammertz et al. 2010, with the variance steering of
 * SVGF, Schied et al. 2017, sections 4.3-4.4; the temporal part is gmupt_temporal_* below) ----
 * Inputs per pixel: the beauty RGBA32F texel of an accumulation target (rgb = running mean of tonemapped samples, a = sample count as
 * uint bits) and its gmupt_aov record.  All arithmetic is binary32 in the order stated here, no contraction; dpow / dexp2 / dsqrt are the
 * deterministic functions of DESIGN.md ("Deterministic math"), normalize3(v) = v * (1 / sqrt((v.x*v.x + v.y*v.y) + v.z*v.z)).
 *
 * Valid pixel: sample count > 0, aov.triangle != -1, aov.light == 0 and sqrt(dot3(aov.normal, aov.normal)) > 0.  Invalid pixels (misses,
 *   light spheres, pixels without samples) are copied to the output bit for bit and have weight 0 as a neighbour.  A valid pixel has
 *   n = normalize3(aov.normal), z = aov.depth, x = aov.position, a = aov.albedo, l = (0.2126f*r + 0.7152f*g) + 0.0722f*b of its beauty.
 *   The filter works on the stored (tonemapped) values: there is no albedo demodulation, albedo is an edge-stopping guide.
 * Initial variance of a valid p: over the valid pixels q of p's 3x3 neighbourhood inside the image (p included), row-major (dy outer),
 *   S1 = sum l_q, S2 = sum l_q*l_q from 0.0f, m1 = S1 / (float)count, m2 = S2 / (float)count, v_p = max(0, m2 - m1*m1).
 * Pass k = 0 .. passes-1, step s = 1 << k, colour c and variance v of the previous pass (pass 0: the beauty rgb and v_p); per valid p:
 *   g_p = sum (h3[dx] * h3[dy]) * v_q / sum h3[dx] * h3[dy] over the valid q = p + (dx, dy) of the 3x3 neighbourhood inside the image,
 *         h3 = {0.25, 0.5, 0.25}, both sums from 0.0f in row-major order, one division;
 *   taps q = p + s * (i, j), j = -2..2 outer, i = -2..2 inner, skipped when outside the image or invalid (the centre is a tap):
 *     w   = ((h[i] * h[j]) * w_n) * E,  h = {1/16, 1/4, 3/8, 1/4, 1/16}
 *     w_n = dpow(max(0, dot3(n_p, n_q)), sigma_normal)
 *     E   = dexp2(-((d_l + d_x) + d_a) * 1.44269504f)
 *     d_l = |l_p - l_q| / (sigma_color * dsqrt(g_p) + 1e-6f)
 *     d_x = |dot3(n_p, x_q - x_p)| / (sigma_plane * z_p)
 *     d_a = ((|a_q.r - a_p.r| + |a_q.g - a_p.g|) + |a_q.b - a_p.b|) / sigma_albedo
 *   W = sum w, C = sum w * c_q (per channel), V = sum (w * w) * v_q, all from 0.0f in tap order; c'_p = C / W, v'_p = V / (W * W).
 *   (W > 0 whenever the centre weight is: with sane sigmas always.  If W is not > 0 the pixel keeps c_p and v_p.)
 * Output: RGBA32F, rgb = the last pass's colour of a valid pixel, alpha = the input alpha bits; an invalid pixel is its input texel.
 *   The PNG / PFM writers and progressive.to_rgba8 take it unchanged.
 * Non-finite and extreme input is no error: pixels are not validated, the arithmetic above decides, on the device and on the host alike.
 *   A colour channel that is +-inf: the pixel keeps its texel at every pass (its centre tap has d_l = NaN, so W is NaN and not > 0), and
 *   every valid pixel with a chain of taps back to it takes a NaN in THAT channel (d_l = inf, E = 0, w = 0, C += 0 * inf): the poison
 *   reaches 2 * (2^passes - 1) pixels per axis, 62 at five passes.  A NaN colour channel, position or albedo poisons nobody:
 *   whoever taps such a pixel (the pixel itself included) has a NaN W in that pass and keeps its previous colour and variance.  A NaN
 *   or zero depth (read for the centre only; 0 / 0 at the centre tap) makes the pixel's own W NaN and is invisible to others.  An
 *   infinite albedo difference weighs 0 (d_a = inf, E = 0).  An infinite position component gives an infinite d_x, which weighs 0, or
 *   a NaN d_x where the centre normal's component on that axis is exactly 0 (0 * inf), which freezes the tapping pixel for that pass;
 *   the pixel that holds it has inf - inf = NaN at its own centre tap and keeps its colour.  A negative depth makes d_x negative
 *   and weights above 1.  A normal
 *   with a NaN component, or whose dot3 underflows to 0, makes the pixel invalid (copied bit for bit); one whose dot3 overflows
 *   normalises to 0 and one with an infinite component to (NaN, 0, 0): max(0, .) drops the NaN, all its weights are 0 or NaN and it keeps
 *   its colour.  Denormal colours and guides are kept, never flushed.  Sample-count and alpha words are opaque bits: any non-zero word
 *   counts as sampled (0x80000000, NaN patterns) and comes through bit for bit.  The sign and payload of a NaN that the arithmetic
 *   generates are not part of the rule (x86 and gfx950 differ there); which words are NaN, every finite word, every infinity and every
 *   zero with its sign are.
 * Parameters: passes 1..5, every sigma finite and > 0, else GMUPT_ERR_INVALID_ARGUMENT. */
typedef struct {
    uint32_t passes;      /* a-trous passes (steps 1, 2, 4, ..); default 5 */
    float sigma_color;    /* luminance edge stop, in units of the local standard deviation; default 4 */
    float sigma_normal;   /* exponent of the normal cosine; default 128 */
    float sigma_plane;    /* distance from p's tangent plane, relative to p's depth; default 0.02 */
    float sigma_albedo;   /* L1 albedo difference; default 0.1 */
} gmupt_denoise_params;   /* 20 bytes */
#define GMUPT_DENOISE_MAX_PASSES 5
void gmupt_denoise_default_params(gmupt_denoise_params* p);
/* beauty_rgba (width * height RGBA32F texels), aov (width * height records) and out_rgba are caller-owned DEVICE memory, 16-byte aligned,
 * row-major; any size (e.g. a gathered whole frame).  out_rgba must not overlap beauty_rgba (the last pass reads other pixels' beauty
 * texels while it writes).  Enqueued on the renderer's stream behind pending work,
 * then synchronises; the renderer's frame, state and statistics are not touched.  The filter's scratch (76 bytes per pixel) is allocated
 * on first use, grown when a larger image comes, and kept until gmupt_renderer_destroy.  ms (may be NULL): device time of the filter.
 * p may be NULL (the defaults).  Errors: GMUPT_ERR_INVALID_ARGUMENT for a NULL or misaligned pointer, an output overlapping the beauty,
 * out_bytes < width * height * 16, an empty image or bad parameters. */
int gmupt_denoise_image(gmupt_renderer* r, const float* beauty_rgba, const gmupt_aov* aov, uint32_t width, uint32_t height,
                        const gmupt_denoise_params* p, float* out_rgba, size_t out_bytes, float* ms /* may be NULL */);
/* The renderer's framebuffer rectangle (the tile in tile mode; tile edges are image edges, so a tile's result differs from a whole-frame
 * denoise near the seams): gmupt_render_aovs(r, aov_samples) into internal scratch, a copy of the framebuffer, then gmupt_denoise_image
 * into out (device memory, 16-byte aligned, bytes >= width * height * 16).  Errors of gmupt_render_aovs (GMUPT_ERR_NOT_BOUND,
 * GMUPT_ERR_UNSUPPORTED, GMUPT_ERR_CAST_FAULT ...) and of gmupt_copy_framebuffer_to_device are returned as they are; the ones that need no
 * device work are checked before the internal scratch (80 bytes per pixel) is allocated or grown.  The frame, path
 * state, queues, counters and statistics are not touched.  info (may be NULL): as gmupt_render_aovs, ms = AOV time + filter time. */
int gmupt_render_denoised(gmupt_renderer* r, uint32_t aov_samples, const gmupt_denoise_params* p, float* out_rgba, size_t bytes,
                          gmupt_trace_info* info /* may be NULL */);
/* The same filter on host arrays (the same binary32 sequence, bit for bit the device result), in row bands on up to `threads` std::threads
 * (0 -> 1, at most 16); the result does not depend on the thread count.  out_rgba must not overlap beauty_rgba.  Errors as
 * gmupt_denoise_image. */
int gmupt_denoise_host(const float* beauty_rgba, const gmupt_aov* aov, uint32_t width, uint32_t height, const gmupt_denoise_params* p,
                       float* out_rgba, size_t out_bytes, uint32_t threads);

/* ---- temporal reuse: the denoiser's input integrated with the reprojected history of earlier accumulations (the temporal part of SVGF,
 * Schied et al. 2017, section 4.1, on the unfiltered colour) ----
 * History record (gmupt_history, 48 bytes, one per pixel of a rectangle): the INTEGRATED, UNFILTERED colour of the pixel, its effective
 * sample count, and the guides of the consistency tests.  Filtered colour is never fed back, so blur does not compound from call to call.
 * All arithmetic is binary32 in the order stated here, no contraction (as the denoiser).
 *
 * Projection of a world point X into a previous camera (P, U, Hv, V, ps = its position, upperLeftCorner, horizontal, vertical, pixelSize):
 *   F = (U + 0.5f*Hv) - 0.5f*V (per component); d = X - P; lambda = dot3(d, F) / dot3(F, F); behind the camera unless lambda > 0;
 *   r = d / lambda (per component); e = r - U;
 *   u = (dot3(e, Hv) / dot3(Hv, Hv)) / ps.x, v = (-dot3(e, V) / dot3(V, V)) / ps.y   (whole-frame pixel coordinates, centres at integers).
 *   This inverts the primary ray normalize(U + Hv*(px*ps.x) - V*(py*ps.y)) of newPath.hlsl:36-39 / gmupt_camera_pick_ray; it needs
 *   Hv, V and F mutually orthogonal, which the host camera guarantees (Camera.cpp:92-94 builds them from one orthonormal frame).
 * Integration of pixel p of the current rectangle (W x H; beauty texel: rgb B, sample count n = alpha bits, nf = (float)n; record aov):
 *   Surface pixel: aov.triangle != -1, aov.light == 0, sqrt(dot3(aov.normal, aov.normal)) > 0 (the denoiser's test without n > 0);
 *     n_p = normalize3(aov.normal), x_p = aov.position, z_p = aov.depth.
 *   Any other pixel: the integrated texel is the beauty texel bit for bit; its new record is all zero (valid = 0).
 *   Surface pixel: (u, v) = the projection of x_p into the previous camera, minus the previous rectangle's origin; fu = floorf(u),
 *     fv = floorf(v), fx = u - fu, fy = v - fv; taps k = 0..3 at (fu, fv), (fu+1, fv), (fu, fv+1), (fu+1, fv+1) with weights
 *     (1-fx)*(1-fy), fx*(1-fy), (1-fx)*fy, fx*fy.  Tap q counts when it lies inside the previous rectangle, its record has valid == 1 and
 *     count > 0, material_q == aov.material, dot3(n_p, n_q) >= min_normal_cos and |dot3(n_p, x_q - x_p)| <= plane_dist * z_p.
 *     Over the counted taps in k order, sums from 0.0f: Sw = sum w, Sc = sum w*color_q (per channel), Sn = sum w*count_q;
 *     Hc = Sc / Sw, N_h = min(history_cap, Sn / Sw).  N_h = 0 when the point is behind the previous camera, when Sw is not > 0, or
 *     without a previous record set.
 *     N_h == 0: the integrated texel is the beauty texel bit for bit;
 *     n == 0:   rgb = Hc, alpha = the bits of (uint32_t)ceilf(N_h);
 *     else:     rgb = ((N_h*Hc) + (nf*B)) / (N_h + nf) per channel, alpha = the bits of n + (uint32_t)ceilf(N_h).
 *     New record: color = the integrated rgb, count = N_h + nf (nf when N_h == 0), normal = n_p, material = aov.material,
 *     position = x_p, valid = (count > 0).
 * Output = gmupt_denoise_image of the integrated image with the spatial parameters.  Hence, bit for bit: (a) without history (first call,
 *   after gmupt_temporal_reset, history_cap = 0) the output is gmupt_denoise_image(beauty, aov); (b) always, the output is
 *   gmupt_denoise_image(integrated, aov) with the integrated image of gmupt_temporal_integrate_host.  The output alpha is therefore the
 *   effective count word, not the frame's sample count (progressive.to_rgba8 and the PNG / PFM writers ignore alpha).
 * Accumulation epochs (no double counting): while the camera stands still the beauty keeps accumulating, so the last call's records
 *   are already contained in the frame.  A handle keeps two record sets, each with its camera and rectangle: FROZEN, the history of
 *   earlier accumulations, and LAST, the records of the latest call.  A call with new_accumulation != 0 first moves LAST into FROZEN (a
 *   pointer swap); every call integrates against FROZEN and then replaces LAST with its own records.  The samples drawn between the last
 *   call of an accumulation and its restart are not in the history.  The previous rectangle may have any size and origin (reprojection
 *   needs no matching size), so a resize keeps the history.
 * Non-finite and extreme input is no error; neither pixels, records nor cameras are validated.  The guard -1 <= fu <= W - 1 (fv likewise)
 *   is false for NaN and +-inf, so a projection that is NaN, infinite or far outside (lambda 0, NaN or so small that d / lambda
 *   overflows; dot3(F, F) = 0; pixelSize = 0; a NaN or infinite position) takes no history: N_h = 0, the beauty texel bit for bit,
 *   count = nf.  fu = -1 with fx = 0 is inside the guard, but all weight lies on the column outside: Sw = 0, no history.  A tap whose
 *   count is NaN or not > 0, whose valid word is not 1, or whose normal or position makes a test NaN does not count.  Non-finite colours
 *   of counted taps propagate into the integrated texel and the new record (w * inf, and NaN where w is 0); a count of +inf gives
 *   N_h = history_cap (min drops a NaN).  n is an integer word: nf = (float)n, and n + (uint32_t)ceilf(N_h) wraps modulo 2^32.  A
 *   normal with a NaN component, or whose dot3 underflows to 0, makes the pixel no surface pixel.  The denoiser's paragraph holds for
 *   the filter that follows, for generated NaNs and for alpha words.
 * Parameters: the spatial ones as gmupt_denoise_params; history_cap in [0, 65536]; min_normal_cos finite and <= 1; plane_dist finite
 *   and >= 0; else GMUPT_ERR_INVALID_ARGUMENT. */
typedef struct {
    float color[3];    float count;        /* integrated unfiltered rgb; effective sample count */
    float normal[3];   uint32_t material;  /* normalised guide normal; aov.material */
    float position[3]; uint32_t valid;     /* aov.position; 1 when count > 0, else 0 */
} gmupt_history;       /* 48 bytes */
typedef struct {
    gmupt_denoise_params spatial;   /* the filter run on the integrated image; default gmupt_denoise_default_params */
    float history_cap;              /* most samples the history may stand for; default 32 */
    float min_normal_cos;           /* tap test: dot3(n_p, n_q) >= this; default 0.9 */
    float plane_dist;               /* tap test: distance from p's tangent plane, relative to p's depth; default 0.02 */
} gmupt_temporal_params;            /* 32 bytes */
#define GMUPT_TEMPORAL_MAX_CAP 65536.0f
void gmupt_temporal_default_params(gmupt_temporal_params* p);
/* A history handle of a renderer: its device and stream, its spatial scratch, and two record sets allocated on first use and grown for
 * larger images.  It must not outlive its renderer.  gmupt_temporal_reset drops both record sets (the next output is consequence (a)). */
typedef struct gmupt_temporal gmupt_temporal;
int gmupt_temporal_create(gmupt_renderer* r, gmupt_temporal** out);
void gmupt_temporal_destroy(gmupt_temporal* t);
int gmupt_temporal_reset(gmupt_temporal* t);
/* beauty_rgba, aov, out_rgba: caller-owned DEVICE memory as for gmupt_denoise_image (any size, e.g. a gathered whole frame; out must not
 * overlap beauty).  cam: the camera the image was rendered with (host memory); (x0, y0): the image's origin in that camera's whole frame.
 * Both are stored with the new records.  Enqueued on the renderer's stream: k_tp_integrate, then the denoiser's launches, no host
 * synchronisation between them; then synchronises.  ms (may be NULL): device time of the whole call.  p may be NULL (the defaults).
 * Errors: those of gmupt_denoise_image, a NULL handle or camera, bad parameters (GMUPT_ERR_INVALID_ARGUMENT). */
int gmupt_temporal_denoise_image(gmupt_temporal* t, const float* beauty_rgba, const gmupt_aov* aov, const gmupt_camera_buffer* cam,
                                 uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, int new_accumulation,
                                 const gmupt_temporal_params* p, float* out_rgba, size_t out_bytes, float* ms /* may be NULL */);
/* gmupt_render_denoised with temporal reuse, on the renderer t was created for: gmupt_render_aovs(aov_samples) and a copy of the
 * framebuffer into internal scratch, then gmupt_temporal_denoise_image with the renderer's current camera and rectangle (the tile in tile
 * mode).  new_accumulation is set from the renderer's accumulation generation, which an iteration that clears the frame
 * (iterationCounter == 0) and gmupt_resize advance: the first call after such an event folds.  That generation is host bookkeeping; the
 * frame, path state, queues, counters and statistics are not touched.  Errors and info as gmupt_render_denoised; t of another renderer
 * is GMUPT_ERR_INVALID_ARGUMENT. */
int gmupt_render_denoised_temporal(gmupt_renderer* r, gmupt_temporal* t, uint32_t aov_samples, const gmupt_temporal_params* p,
                                   float* out_rgba, size_t bytes, gmupt_trace_info* info /* may be NULL */);
/* The integration step on host arrays (the same binary32 sequence as k_tp_integrate, bit for bit), in row bands on up to `threads`
 * std::threads (0 -> 1, at most 16; the result does not depend on the count).  beauty_rgba / aov: width * height texels / records of the
 * current image.  prev: prev_width * prev_height records with origin (prev_x0, prev_y0) in prev_cam's whole frame, or NULL (no history;
 * prev_cam may then be NULL too).  Outputs: out_rgba (width * height RGBA32F, the integrated image) and out_history (width * height
 * records).  Together with gmupt_denoise_host it is the reference of gmupt_temporal_denoise_image.  Errors: NULL or overlapping
 * arrays, an empty image, more than 2^28 pixels, bad parameters (GMUPT_ERR_INVALID_ARGUMENT). */
int gmupt_temporal_integrate_host(const float* beauty_rgba, const gmupt_aov* aov, uint32_t width, uint32_t height,
                                  const gmupt_history* prev, const gmupt_camera_buffer* prev_cam, uint32_t prev_x0, uint32_t prev_y0,
                                  uint32_t prev_width, uint32_t prev_height, const gmupt_temporal_params* p,
                                  float* out_rgba, gmupt_history* out_history, uint32_t threads);

/* ---- refit: moved vertices without a rebuild or a rebind (an extension; the reference has no moving geometry) ----
 * After the caller has updated the vertex buffer (same vertex count, same triangle records), every box of the bound tree is recomputed
 * bottom-up and every traversal table of the renderer is rewritten in place, on the GPU.  The topology stays: the same nodes, leaves,
 * reference order, 4-wide collapse, numbering and tie words.
 *
 * Box rule (binary32; gmupt_bvh_refit_host and the kernels run the same statements, csrc/pt_refit.hpp):
 *   lo(a, b) = b < a ? b : a, hi(a, b) = b > a ? b : a, per component.
 *   Leaf [left, right) with right > left: start from vertex v[0] of reference `left`, fold in v[1], v[2], then the three vertices of each
 *     further reference in index order (min = lo(min, p), max = hi(max, p)).  The box is that of the WHOLE triangles: a reference that a
 *     spatial split of the builder had clipped gets a looser box than the builder gave it.  That is correct (the triangle test decides
 *     the hit) and is the price of refitting an SBVH.
 *   Empty leaf (right == left): its box is left as it is.
 *   Inner node: min = lo(left child's min, right child's min), max = hi(left child's max, right child's max).  Children have larger
 *     indices than their parent (bind validates this), so any order in which a node comes after its children is valid; the device
 *     runs one launch per node height, lowest first.
 *   pad0 / pad1 / pad2, left, right, isLeaf are not written.
 * gmupt_bvh_refit_host: the rule on host arrays, in place.  Leaves on up to `threads` std::threads (0 -> 1, at most 16; the result does
 *   not depend on the count).  Errors, with the nodes untouched: NULL arrays, no nodes, an inner node with a child index not above its
 *   own or outside the array, a leaf range outside [0, num_tris], a triangle record with a vertex index outside [0, num_verts)
 *   (GMUPT_ERR_INVALID_ARGUMENT).
 * gmupt_renderer_refit, in this order:
 *   1. GMUPT_ERR_NOT_BOUND without a bound scene.  The renderer remembers the node, triangle and vertex buffers it was bound to (they
 *      must outlive the binding); element counts other than at bind time: GMUPT_ERR_INVALID_ARGUMENT.
 *   2. Waits for the renderer's stream.  k_rf_finite checks that every vertex a triangle record uses is finite; one word is read back.
 *      A non-finite vertex: GMUPT_ERR_INVALID_ARGUMENT, nothing has been written.  A vertex no record uses may hold anything.
 *   3. On the renderer's stream, no host synchronisation in between: the node boxes in the caller's GMUPT_BUFFER_BVH_NODES buffer
 *      (leaves in one launch, then one launch per height: `levels`), then Tri48 (v0, e1 = v1 - v0, e2 = v2 - v0; flag and
 *      first-equal-reference words kept), TriPair, Node64 (filler records untouched), WNode planes (links, aux, NaN slots kept), and
 *      rootMin / rootMax.  A renderer without a wide copy (GMUPT_TRAVERSAL other than wide, or a bound tree whose child boxes stuck out of
 *      their parents) skips the TriPair / WNode parts and step 4; the wide copy appears only with the next bind.
 *   4. The wide walk equals the binary one only if no OPENED node (one whose own slot the collapse replaced by its children) has a child
 *      that is flat on an axis, on which the node is not flat, in the plane of one of the node's faces.  Bind chose what to open by that
 *      rule on the old boxes; the WNode kernel evaluates it for every opened node on the new boxes.
 *   5. One small readback (flag, root box).  Flag clear: rebuilt = 0.  Flag set: the host pass of gmupt_renderer_bind_scene runs on the
 *      refitted node buffer, exactly what a fresh bind of these buffers would do: rebuilt = 1, reason = GMUPT_REFIT_FLAT_CHILD.  A
 *      -DGMUPT_VARIANTS build (it also keeps Rec64 records) always takes this path, reason = GMUPT_REFIT_VARIANTS_BUILD.  Either way
 *      the results are those of a fresh renderer bound to the same buffers.
 *   6. ms = device time of step 3 (hipEvents on the stream); opened_nodes = size of the checked list.
 * Refit does not touch the frame, path state, queues or statistics.  Paths in flight carry hits of the old geometry: restart the
 * accumulation (iterationCounter = 0) as after a light edit.  Shading normals live in the GMUPT_BUFFER_TRI_PROPS buffer, whose pointer is
 * bound: update it with gmupt_buffer_update, or recompute smooth normals on the device with gmupt_normals_update; no refit involved.  Several renderers bound to the same buffers each call refit; the node
 * boxes are recomputed to the same bytes each time.
 * What stays as bind left it: which nodes live in LDS, the line pairing of Node64 and the collapse choices were made by surface area of
 * the OLD boxes.  They affect speed only.  A caller whose mesh has moved far rebuilds the SBVH and rebinds; refit is for the frames in
 * between. */
#define GMUPT_REFIT_FLAT_CHILD 1u      /* an opened node of the 4-wide collapse got a flat child in one of its face planes */
#define GMUPT_REFIT_VARIANTS_BUILD 2u  /* a -DGMUPT_VARIANTS build: the tables always come from the host pass */
typedef struct { uint32_t rebuilt; uint32_t reason; uint32_t levels; uint32_t opened_nodes; double ms; } gmupt_refit_info;   /* 24 bytes */
int gmupt_bvh_refit_host(gmupt_bvh_node* nodes, uint32_t num_nodes, const gmupt_triangle* tris, uint32_t num_tris,
                         const float* verts, uint32_t num_verts, uint32_t threads);
int gmupt_renderer_refit(gmupt_renderer* r, gmupt_refit_info* info /* may be NULL */);

/* ---- motion: temporal reuse across refits -- the history is looked up where the surface point WAS (the other half of SVGF's temporal
 * stage, Schied et al. 2017, section 4.1).  Opt-in: every entry point above behaves as before. ----
 * Motion record (gmupt_motion, 16 bytes, one per pixel of the renderer's rectangle).  For a pixel whose centre ray (k = 0 of gmupt_aov_ray)
 * hits triangle record T with barycentrics (u, v) and no nearer light sphere, p0, p1, p2 the vertices T.v[0..2] of the bound vertex buffer
 * and q0, q1, q2 the same indices of the caller's array of PREVIOUS vertices, binary32, no contraction, per component:
 *     w      = (1.0f - u) - v
 *     b_now  = (w * p0 + u * p1) + v * p2
 *     b_prev = (w * q0 + u * q1) + v * q2
 *     prev_position = (b_prev == b_now) ? aov.position : aov.position + (b_prev - b_now)
 *     flags  = 1
 *   Every other pixel (miss, light sphere): all zero.  The displacement form makes a triangle whose vertices did not move give
 *   prev_position == aov.position bit for bit (the ?: also keeps a -0.0f component): an unmoved scene takes exactly the existing path.
 *   Non-finite and extreme input is no error: previous vertices are not validated.  A NaN in b_prev fails b_prev == b_now and propagates
 *   into that component of prev_position; an infinite one gives +-inf, or NaN where a barycentric weight is 0 (0 * inf).  The sign and
 *   payload of such a NaN are not part of the rule.  In the integration a record counts as moved only when its flags word is exactly 1;
 *   with a non-finite prev_position the projection is NaN or outside the guard and the pixel takes no history.
 * gmupt_render_aovs_motion: gmupt_render_aovs (k_aov_raygen, the ray cast, k_aov_resolve, all unchanged; aov_out is bit for bit that
 *   call's output) plus k_mv_resolve per chunk on the same hits.  prev_verts: DEVICE memory, 3 floats per vertex, 4-byte aligned; num_verts
 *   must equal the bound vertex count.  motion_out: DEVICE memory, 16-byte aligned, motion_bytes >= width * height * 16.  Errors follow
 *   gmupt_render_aovs; a NULL or misaligned prev_verts / motion_out, too few bytes or another vertex count: GMUPT_ERR_INVALID_ARGUMENT.
 * gmupt_motion_host: the rule on host arrays, the reference of the kernel.  hits: the n centre-ray hits (gmupt_trace_rays on the
 *   gmupt_aov_ray rays gives the AOV's own), aov: their records.  Errors: NULL arrays, a hit triangle outside [0, num_tris), a vertex index
 *   of a hit triangle outside [0, num_verts) (GMUPT_ERR_INVALID_ARGUMENT).
 * Integration with a motion plane: with a record of flags == 1 the integration of gmupt_temporal_* above changes in two places and nowhere
 *   else: the point projected into the previous camera is prev_position instead of x_p, and the plane test of a tap is
 *   |dot3(n_p, x_q - prev_position)| <= plane_dist * z_p (the tap's record holds its position in the previous pose; the current normal
 *   stands in for the previous one, and min_normal_cos bounds what is accepted).  The new record still stores x_p, the current pose, so
 *   the next call's motion plane lines up with it.  With flags == 0, or without a motion plane, the pixel is the arithmetic above.
 *   gmupt_temporal_integrate_motion_host: gmupt_temporal_integrate_host plus `motion` (width * height records; NULL = that function, bit
 *   for bit).  gmupt_temporal_denoise_image_motion: gmupt_temporal_denoise_image plus a DEVICE `motion` pointer (16-byte aligned; NULL =
 *   that function), for callers who bring gathered frames and their own motion plane; k_tp_integrate_mv takes the place of k_tp_integrate.
 *   The epoch rule is unchanged; the motion plane must describe the step from the pose of the FROZEN set to the image's pose.
 * gmupt_render_denoised_temporal_motion: gmupt_render_denoised_temporal that keeps the vertex pose of each record set.
 *   The renderer has a geometry generation (host bookkeeping): gmupt_renderer_refit advances it, gmupt_renderer_bind_scene starts a new
 *   binding.  FROZEN and LAST each carry the generation and a device snapshot of the bound vertex buffer (12 bytes per vertex) taken by the
 *   call that wrote their records; the fold swaps the snapshots with the record sets.  A snapshot is a device-to-device copy on the
 *   renderer's stream, taken only when LAST's generation differs from the renderer's: once per refit, not per call.  When FROZEN's
 *   generation differs from the renderer's, the call runs gmupt_render_aovs_motion against FROZEN's snapshot and integrates with the
 *   motion plane (16 more bytes per pixel of scratch); when it is equal the call is exactly gmupt_render_denoised_temporal.  A FROZEN set
 *   without a snapshot (written by gmupt_render_denoised_temporal or gmupt_temporal_denoise_image), of another binding or of another
 *   vertex count integrates without a motion plane.  gmupt_temporal_reset and gmupt_temporal_destroy free the snapshots.  The frame, path
 *   state, queues, counters and gmupt_get_stats stay untouched.  Errors and info as gmupt_render_denoised_temporal. */
typedef struct { float prev_position[3]; uint32_t flags; } gmupt_motion;   /* 16 bytes */
int gmupt_render_aovs_motion(gmupt_renderer* r, uint32_t samples, const float* prev_verts, uint32_t num_verts, gmupt_aov* aov_out, size_t aov_bytes,
                             gmupt_motion* motion_out, size_t motion_bytes, gmupt_trace_info* info /* may be NULL */);
int gmupt_motion_host(const gmupt_hit* hits, const gmupt_aov* aov, size_t n, const gmupt_triangle* tris, uint32_t num_tris,
                      const float* verts_now, const float* verts_prev, uint32_t num_verts, gmupt_motion* out);
int gmupt_temporal_integrate_motion_host(const float* beauty_rgba, const gmupt_aov* aov, const gmupt_motion* motion /* may be NULL */,
                                         uint32_t width, uint32_t height,
                                         const gmupt_history* prev, const gmupt_camera_buffer* prev_cam, uint32_t prev_x0, uint32_t prev_y0,
                                         uint32_t prev_width, uint32_t prev_height, const gmupt_temporal_params* p,
                                         float* out_rgba, gmupt_history* out_history, uint32_t threads);
int gmupt_temporal_denoise_image_motion(gmupt_temporal* t, const float* beauty_rgba, const gmupt_aov* aov, const gmupt_motion* motion /* may be NULL */,
                                        const gmupt_camera_buffer* cam, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height,
                                        int new_accumulation, const gmupt_temporal_params* p, float* out_rgba, size_t out_bytes,
                                        float* ms /* may be NULL */);
int gmupt_render_denoised_temporal_motion(gmupt_renderer* r, gmupt_temporal* t, uint32_t aov_samples, const gmupt_temporal_params* p,
                                          float* out_rgba, size_t bytes, gmupt_trace_info* info /* may be NULL */);

/* ---- Infill: surface pixels without a sample take a colour from the sampled pixels of the same surface, before the denoiser runs (a
 * guided push of sparse samples: the a-trous taps and edge stops of the denoiser above, run over growing steps from the sampled pixels
 * into the holes).  Opt-in: every entry point above behaves as before. ----
 * Inputs per pixel: the beauty texel (rgb = running mean of tonemapped samples, a = sample count as uint bits) and its gmupt_aov record.
 * All arithmetic is binary32 in the order stated here, no contraction; dpow / dexp2 / normalize3 as for the denoiser.
 *
 * Classes.  Surface pixel: aov.triangle != -1, aov.light == 0, sqrt(dot3(aov.normal, aov.normal)) > 0 (the denoiser's test without the
 *   sample count).  SOURCE: a surface pixel with count > 0.  HOLE: a surface pixel with count == 0.  Every other pixel (miss, light
 *   sphere, zero or NaN normal) is copied to the output bit for bit, is never a source and is never filled.  A surface pixel has
 *   n = normalize3(aov.normal), x = aov.position, z = aov.depth, a = aov.albedo, m = aov.material.
 * Pass k = 0 .. passes-1, step s = 1 << k.  A pixel is KNOWN in pass k when it is a source or was filled by a pass before k; a hole that
 *   is not known is OPEN.  Per open hole p, taps q = p + s * (i, j), j = -2..2 outer, i = -2..2 inner; a tap counts when it lies inside
 *   the image, is known in pass k, and m_q == m_p (the centre is open, so it never counts):
 *     w   = ((h[i] * h[j]) * w_n) * E,  h = {1/16, 1/4, 3/8, 1/4, 1/16}
 *     w_n = dpow(max(0, dot3(n_p, n_q)), sigma_normal)          (max(0, c) is 0 when c is NaN)
 *     E   = dexp2(-(d_x + d_a) * 1.44269504f)
 *     d_x = |dot3(n_p, x_q - x_p)| / (sigma_plane * z_p)
 *     d_a = ((|a_q.r - a_p.r| + |a_q.g - a_p.g|) + |a_q.b - a_p.b|) / sigma_albedo
 *   There is no luminance term: a hole has no luminance.  W = sum w, C = sum w * c_q (per channel), from 0.0f in tap order, c_q the
 *   source's beauty rgb or the colour q was filled with.  If W > 0 (false for NaN) the hole is filled with C / W (one division per channel)
 *   and is known from pass k+1 on; otherwise it stays open.  Pixels filled in pass k are not visible to pass k, so the result does not
 *   depend on the order in which pixels are processed.  Sources and filled pixels never change again.
 * Output: RGBA32F.  A filled pixel: its colour, alpha = the bits of sample count 1 (so that gmupt_denoise_image takes it as valid).
 *   Every other pixel -- no surface, source, hole still open after the last pass -- is its input texel bit for bit.
 *   Non-finite colours and guides are no error: they propagate through the sums, or leave the hole open, as the statements above say.
 * Reach: a hole filled in pass k has a known pixel at most 2 * 2^k away per axis, which itself was known by a chain of earlier passes:
 *   at most 2 * (2^0 + .. + 2^(passes-1)) = 2 * (2^passes - 1) pixels per axis from a source, 126 at passes = 6.  A hole farther than
 *   that from every source stays open.
 * Hence, bit for bit: (a) a frame without holes, and a frame without sources, come out as they went in; (b) filled colour never enters
 *   a temporal history -- in the chains below the records are written by the integration, before the infill runs, so a later call's
 *   output does not depend on whether an earlier call had the infill on; (c) every chained entry point equals the composition of its
 *   parts: gmupt_denoise_image(gmupt_infill_image(beauty, aov), aov) without a history,
 *   gmupt_denoise_image(gmupt_infill_image(integrated, aov), aov) with one (integrated: gmupt_temporal_integrate*_host's image).
 * Parameters: passes 1..8, every sigma finite and > 0, else GMUPT_ERR_INVALID_ARGUMENT. */
typedef struct {
    uint32_t passes;      /* passes (steps 1, 2, 4, ..); default 6 */
    float sigma_normal;   /* exponent of the normal cosine; default 32 */
    float sigma_plane;    /* distance from p's tangent plane, relative to p's depth; default 0.02 */
    float sigma_albedo;   /* L1 albedo difference; default 0.1 */
} gmupt_infill_params;    /* 16 bytes */
#define GMUPT_INFILL_MAX_PASSES 8
void gmupt_infill_default_params(gmupt_infill_params* p);
typedef struct {
    uint32_t sources, holes;      /* of the input: surface pixels with / without a sample */
    uint32_t filled, open_left;   /* holes that took a colour / that no pass reached (filled + open_left == holes) */
    double ms;                    /* device time of the stage (gmupt_infill_host: 0) */
} gmupt_infill_info;              /* 24 bytes */
/* beauty_rgba, aov, out_rgba: caller-owned DEVICE memory as for gmupt_denoise_image (16-byte aligned, any image size; out must not
 * overlap beauty; out_bytes >= width * height * 16).  Enqueued on the renderer's stream behind pending work: a 16-byte memset of the
 * counters, k_if_prepare, then one k_if_pass per pass, no host synchronisation between them.  info == NULL: the call returns without
 * waiting for the stream (later work on the renderer's stream is ordered behind it).  info != NULL: one synchronisation, then the four
 * counts and the event time.  The counts are integer sums, the same whatever the order of the waves.  The stage's scratch (256 bytes +
 * 76 per pixel) is allocated on first use, grown when a larger image comes (that waits for the stream) and kept until
 * gmupt_renderer_destroy; the frame, path state, queues, counters and statistics are not touched.  p may be NULL (the defaults).
 * Errors, nothing written: GMUPT_ERR_INVALID_ARGUMENT for a NULL or misaligned pointer, an overlapping output, too few out_bytes, an
 * empty image or bad parameters. */
int gmupt_infill_image(gmupt_renderer* r, const float* beauty_rgba, const gmupt_aov* aov, uint32_t width, uint32_t height,
                       const gmupt_infill_params* p, float* out_rgba, size_t out_bytes, gmupt_infill_info* info /* may be NULL */);
/* The same rule on host arrays (the same binary32 sequence, bit for bit the device result, counts included), in row bands on up to
 * `threads` std::threads (0 -> 1, at most 16); the result does not depend on the thread count.  Errors as gmupt_infill_image. */
int gmupt_infill_host(const float* beauty_rgba, const gmupt_aov* aov, uint32_t width, uint32_t height, const gmupt_infill_params* p,
                      float* out_rgba, size_t out_bytes, gmupt_infill_info* info /* may be NULL */, uint32_t threads);
/* The chain integrate -> infill -> denoise on caller images: gmupt_temporal_denoise_image (motion == NULL) or
 * gmupt_temporal_denoise_image_motion with the infill between the integration and the spatial filter, all on the renderer's stream
 * without a host synchronisation in between.  infill == NULL: bit for bit those two calls (temporal params NULL: the defaults).  The
 * history records are the integration's (consequence (b)).  Errors: theirs, and bad infill parameters. */
int gmupt_temporal_preview_image(gmupt_temporal* t, const float* beauty_rgba, const gmupt_aov* aov, const gmupt_motion* motion /* may be NULL */,
                                 const gmupt_camera_buffer* cam, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height,
                                 int new_accumulation, const gmupt_temporal_params* p, const gmupt_infill_params* infill /* may be NULL */,
                                 float* out_rgba, size_t out_bytes, float* ms /* may be NULL */);
/* The renderer's preview in one call: AOVs -> optional integration (t != NULL) -> optional infill (infill != NULL) -> denoise.
 *   t == NULL:  gmupt_render_denoised with p->spatial (p == NULL: the defaults; nothing else of p is read); flags must be 0.
 *   t != NULL:  gmupt_render_denoised_temporal, or with GMUPT_PREVIEW_MOTION gmupt_render_denoised_temporal_motion.
 * With infill == NULL the call is one of those three, bit for bit.  Errors and info as theirs; unknown flag bits and bad infill
 * parameters: GMUPT_ERR_INVALID_ARGUMENT.  info->ms includes the infill. */
#define GMUPT_PREVIEW_MOTION 1u
int gmupt_render_preview(gmupt_renderer* r, gmupt_temporal* t /* may be NULL */, uint32_t flags, uint32_t aov_samples,
                         const gmupt_temporal_params* p, const gmupt_infill_params* infill /* may be NULL */, float* out_rgba, size_t bytes,
                         gmupt_trace_info* info /* may be NULL */);

/* ---- LBVH: a tree for new geometry built on the GPU (an extension; the reference builds once on the host) ----
 * A linear BVH (Lauterbach et al. 2009: Morton keys and a radix sort; Karras 2012: the hierarchy as a binary radix tree) over the
 * device-resident vertex buffer, in the node / triangle layout above: gmupt_renderer_bind_scene, gmupt_renderer_refit, the ray queries, the
 * AOVs and the CPU oracle take it like an SBVH.  Its quality is lower than the SBVH's (no surface-area heuristic, no spatial splits); it is
 * for rebuilds between frames -- a mesh that moved far or changed its triangle list -- while gmupt_sbvh_build stays the default.
 *
 * The rule (binary32, no contraction, correctly rounded division; lo / hi as in the refit section; gmupt_lbvh_build_host and the kernels
 * run the same statements, csrc/pt_lbvh.hpp).  Input: num_verts vertices, num_tris index triples (each index in [0, num_verts)), an
 * optional vertex_material[num_verts], max_leaf_size L in 1..64 (default 4).
 *   1. Box and centre of triangle i: bmin = bmax = v0, then v1 and v2 folded in (bmin = lo(bmin, p), bmax = hi(bmax, p));
 *      c = (bmin + bmax) * 0.5f per component.
 *   2. cmin / cmax = the minimum / maximum of all c by value, per component (the sign of a zero has no effect below); ext = cmax - cmin.
 *   3. Per axis: ext > 0: x = ((c - cmin) / ext) * 2097152.0f, q = min(2097151u, (uint32_t)x); else q = 0.  (x lies in [0, 2^21] when the
 *      centres are finite.  Huge finite vertices can overflow a centre or ext; a NaN or infinite x gives q = 2097151.)
 *   4. key (63 bits): bit 3k+2 = bit k of q.x, bit 3k+1 = bit k of q.y, bit 3k = bit k of q.z, k = 0..20.  The triangles are sorted
 *      ascending by (key, i).  pos = position in that order, src[pos] = the triangle at that position.
 *   5. Hierarchy: the binary radix tree over the positions 0 .. num_tris-1 with
 *        delta(a, b) = clz64(key_a ^ key_b) if the keys differ, 64 + clz32(a ^ b) if they are equal (a, b positions), -1 outside the range.
 *      Every node covers a range [first, last] of positions.  A range of more than one position splits at the highest differing bit of
 *      its two ends: its children are [first, s] and [s + 1, last], s = the last position with delta(first, s) > delta(first, last).
 *      The tree is a function of the sorted keys alone.  Depth: root 0, a child one more than its parent.
 *   6. Leaves: a node whose range holds <= L positions is a leaf (the root too, when num_tris <= L); the nodes below it do not exist.
 *   7. Numbering: the nodes that exist, by ascending (depth, first); root = 0.  Siblings are adjacent (right == left + 1) and children have
 *      larger numbers than their parent, which bind and refit require.
 *   8. Records.  Triangle record pos: v = the index triple of triangle src[pos] in input order, materialID = vertex_material ?
 *      vertex_material[v[0]] : 0 -- what gmupt_sbvh_flatten writes.  ref_triangle[pos] = src[pos].
 *      Leaf: left = first, right = last + 1, isLeaf = 1, box by the refit leaf rule (the three vertices of each record in index order).
 *      Inner node: left = the number of the child [first, s], right = left + 1, isLeaf = 0, min / max = lo / hi of the left child's
 *      and the right child's.  pad0 / pad1 / pad2 = 0.  Hence gmupt_bvh_refit_host on a fresh LBVH changes no byte.
 *   9. Errors, nothing written / no buffer created: NULL or empty input, an index outside [0, num_verts), L outside 1..64, more than 2^30
 *      triangles: GMUPT_ERR_INVALID_ARGUMENT.  A non-finite vertex that a triangle uses: GMUPT_ERR_INVALID_ARGUMENT (a vertex no triangle
 *      uses may hold anything, as in refit).  A tree deeper than 64, the size of the traversal stacks: GMUPT_ERR_UNSUPPORTED (it takes more
 *      than 2^k triangles whose centres coincide in a cell k levels from the bottom of the key space; the depth can never pass 96).
 * gmupt_lbvh_build_host: the rule on host arrays, the reference of the device build.  nodes_out holds 2 * num_tris - 1 nodes (info->num_nodes
 *   are written), tris_out num_tris records, ref_triangle_out (may be NULL) num_tris words.  info (may be NULL): ms = 0.
 * gmupt_lbvh: a builder handle of a device.  It owns a stream, two events and the scratch of a build (keys, sort storage, parent links,
 *   ranges, numbering and the staged outputs: about 190 bytes per triangle), allocated by the first build, grown when a larger mesh comes and
 *   kept: a per-frame rebuild of a mesh that does not grow allocates only its two output buffers.
 * gmupt_lbvh_build: vertices = a GMUPT_BUFFER_VERTICES buffer of the builder's device; device_indices = caller-owned DEVICE memory, 3 * num_tris
 *   int32, 4-byte aligned; device_vertex_material = DEVICE uint32 per vertex, or NULL; device_ref_triangle = DEVICE int32 per triangle, or
 *   NULL.  The whole build is enqueued on the builder's stream (it does not wait for other streams: finish work that writes the vertex buffer
 *   first), then ONE small readback -- error flags, node count, depth, root box -- and a synchronise.  On success *nodes_out
 *   (GMUPT_BUFFER_BVH_NODES, gmupt_buffer_size = num_nodes * 48) and *triangles_out (GMUPT_BUFFER_TRIANGLES, num_tris * 16) are new buffers
 *   the caller destroys; they go into gmupt_renderer_bind_scene like any other.  Bit for bit the arrays of gmupt_lbvh_build_host.
 *   info->ms = device time of the build's launches (hipEvents).  The host pass of bind (the traversal tables) still runs afterwards. */
typedef struct { uint32_t max_leaf_size; } gmupt_lbvh_params;
void gmupt_lbvh_default_params(gmupt_lbvh_params* p);
typedef struct { uint32_t num_nodes, num_leaves, depth, num_tris; float root_min[3], root_max[3]; double ms; } gmupt_lbvh_info;   /* 48 bytes */
int gmupt_lbvh_build_host(const float* verts, uint32_t num_verts, const int32_t* indices, uint32_t num_tris, const uint32_t* vertex_material /* may be NULL */,
                          const gmupt_lbvh_params* params /* may be NULL */, gmupt_bvh_node* nodes_out, gmupt_triangle* tris_out,
                          int32_t* ref_triangle_out /* may be NULL */, gmupt_lbvh_info* info /* may be NULL */);
typedef struct gmupt_lbvh gmupt_lbvh;
int gmupt_lbvh_create(gmupt_device* dev, gmupt_lbvh** out);
void gmupt_lbvh_destroy(gmupt_lbvh* h);
int gmupt_lbvh_build(gmupt_lbvh* h, const gmupt_buffer* vertices, const int32_t* device_indices, uint32_t num_tris,
                     const uint32_t* device_vertex_material /* may be NULL */, const gmupt_lbvh_params* params /* may be NULL */,
                     gmupt_buffer** nodes_out, gmupt_buffer** triangles_out, int32_t* device_ref_triangle /* may be NULL */,
                     gmupt_lbvh_info* info /* may be NULL */);

/* ---- normals: smooth vertex normals recomputed on the GPU for a mesh that deforms (an extension; the reference loads its normals once) ----
 * The shading normals are the `normal` field of the GMUPT_BUFFER_TRI_PROPS records, one record per vertex, read by the kernels from the
 * caller's buffer.  gmupt_normals_update rewrites that field from the vertex buffer the renderer is bound to, on the renderer's stream.
 *
 * The rule (binary32, nothing contracted, division and square root correctly rounded; gmupt_vertex_normals_host and the kernels run the
 * same statements, csrc/pt_normals.hpp).  Input: num_verts vertices, num_tris index triples, each index in [0, num_verts).  Corner
 * c = 3*t + k is corner k of triangle t.
 *   1. Face vector of triangle t with vertices p0, p1, p2: e1 = p1 - p0, e2 = p2 - p0 (per component),
 *      f = (e1.y*e2.z - e1.z*e2.y, e1.z*e2.x - e1.x*e2.z, e1.x*e2.y - e1.y*e2.x).  Its length is twice the area: the sum below is
 *      area-weighted.  A triangle that is listed twice counts twice.
 *   2. Vertex sum: s = (0, 0, 0); then, for the corners that reference the vertex IN ASCENDING CORNER NUMBER, s = s + f(triangle of the
 *      corner), per component.  The order is part of the rule: float atomics or a tree reduction give another result.
 *   3. l = sqrt((s.x*s.x + s.y*s.y) + s.z*s.z).  If l > 0 and l is finite: n = s * (1.0f / l) per component.  Otherwise n = (0, 1, 0):
 *      a vertex no triangle uses, a sum that vanished, underflowed or overflowed, and a NaN or an infinity anywhere in the vertex's fan.
 *   4. Non-finite vertices are no error and need no readback: rule 3 absorbs them, and a vertex whose fan holds none is unaffected.
 *   5. Only the three `normal` floats of the property records 0 .. num_verts-1 are written.  pad0, uv, materialID, pad1 and any records
 *      beyond num_verts keep their bits.
 * gmupt_vertex_normals_host: the rule on host arrays, no device; normals_out holds 3 floats per vertex.  Up to `threads` std::threads
 *   (0 -> 1, at most 16); the result does not depend on the count.  NULL or empty input, an index outside [0, num_verts), more than 2^30
 *   triangles: GMUPT_ERR_INVALID_ARGUMENT, nothing written.
 * gmupt_normals: a handle of a renderer for one index list: it uses the renderer's device and stream and must not outlive the renderer.
 *   gmupt_normals_create: device_indices = caller-owned DEVICE memory, 3 * num_tris int32, 4-byte aligned, finished by the caller; the
 *   handle keeps its own copy.  It needs a bound scene (GMUPT_ERR_NOT_BOUND); num_verts = the element count of the bound vertex buffer.
 *   On the renderer's stream it builds the vertex -> corner adjacency -- the corner numbers sorted by (vertex, corner) with a stable radix
 *   sort, and where each vertex's corners start -- then reads ONE flag word pair back and synchronises once.  An index outside the vertex
 *   buffer: GMUPT_ERR_INVALID_ARGUMENT and no handle.  Device memory: 40 bytes per triangle and 4 per vertex are kept (index copy, corner
 *   list, face vectors; offsets); 36 more per triangle plus the sort's temporary storage exist during create only.
 * gmupt_normals_update: works on the vertex and property buffers the renderer is bound to NOW (a rebind to buffers of the same vertex
 *   count needs no new handle).  GMUPT_ERR_NOT_BOUND without a scene; a bound vertex count other than at create, or fewer property records
 *   than vertices: GMUPT_ERR_INVALID_ARGUMENT, nothing written.  Two launches on the renderer's stream, ordered with gmupt_renderer_refit
 *   and gmupt_iterate: the face vectors, then one thread per vertex (a vertex of very high valence serialises its thread).  info == NULL:
 *   no host synchronisation.  With info: synchronises; ms = device time of the two launches (hipEvents), max_valence = the most corners
 *   on one vertex.  Paths in flight have shaded with the old normals: restart the accumulation as after a refit.
 * gmupt_buffer_update_device: gmupt_buffer_update with the source in device memory of the buffer's device (e.g. a pose computed by
 *   another library on the GPU): the same ordering (the device is idle before and after the copy) and the same size check.  The caller
 *   has finished the work that produced device_src.  A source that is not device memory of that device: GMUPT_ERR_INVALID_ARGUMENT. */
typedef struct { uint32_t num_verts, num_tris, max_valence, pad; double ms; } gmupt_normals_info;   /* 24 bytes */
int gmupt_vertex_normals_host(const float* verts, uint32_t num_verts, const int32_t* indices, uint32_t num_tris, float* normals_out /* 3 per vertex */,
                              uint32_t threads);
typedef struct gmupt_normals gmupt_normals;
int gmupt_normals_create(gmupt_renderer* r, const int32_t* device_indices, uint32_t num_tris, gmupt_normals** out);
int gmupt_normals_update(gmupt_normals* n, gmupt_normals_info* info /* may be NULL */);
void gmupt_normals_destroy(gmupt_normals* n);
int gmupt_buffer_update_device(gmupt_buffer* buf, const void* device_src, size_t bytes);

/* ---- Tree cost: the surface-area cost of a node buffer, measured where the buffer lives (an extension; the reference builds once and
 * never asks).  It tells a caller whose mesh deforms when the refitted tree has degraded far enough for a rebuild (gmupt_lbvh_build) to
 * pay: compare `sah` of the refitted tree with `sah` at bind time, and with that of a candidate tree before it is bound.
 *
 * The rule, for the N >= 1 records of a GMUPT_BUFFER_BVH_NODES array (gmupt_tree_cost_host and the kernels run the same statements,
 * csrc/pt_treecost.hpp).  No link is followed: every record counts on its own, so any N records are valid input, a buffer that is not a
 * tree included.  All arithmetic is IEEE binary64, nothing contracted.
 *   Extent, per axis:  d = (double)max - (double)min;  e = d > 0 ? d : 0  (a NaN gives 0, so does max < min).
 *   Half area:         a = (ex*ey + ey*ez) + ez*ex.
 *   Weight:            inner node (isLeaf == 0): w = 2;  leaf: w = (double)(uint32_t)(right - left), the subtraction done in uint32
 *                      (right < left wraps).
 *   Term:              a * w.
 *   Sums:              sum_inner over the inner nodes, sum_leaf over the leaves; in each a record of the other kind contributes +0.0.
 *   Order of a sum:    the N terms in record order, padded with +0.0 to a multiple of 256.  Every run of 256 consecutive entries is
 *                      reduced by stride halving -- for s = 128, 64, .., 1: x[i] = x[i] + x[i+s] for all i < s -- and leaves x[0].  The
 *                      results, in run order, are the entries of the next level; repeat until one value is left (N <= 256: one level).
 *                      It is what a block of 256 threads does: s = 128 and 64 across its waves, s = 32 .. 1 inside the first wave.
 *   Integers:          num_inner, num_leaves; num_refs = the sum of the leaf weights as uint64; max_leaf_refs = the largest leaf weight.
 *   SAH:               root_half_area = a of record 0;  sah = (sum_inner + sum_leaf) / root_half_area if root_half_area > 0, else 0.0.
 *                      It is the quantity gmupt_sbvh_sah reports at its default costs (node_cost = tri_cost = 1), from the flattened
 *                      boxes and in a stated order.
 *   Infinite extents are no error: a term may be +inf.  Only inf * 0 (an infinite extent next to a flat axis or an empty leaf) gives a
 *   NaN; the sums are then NaN, and the sign and payload of that NaN are not part of the rule.
 * gmupt_tree_cost_host: the rule on a host array, no device.  Runs on up to `threads` std::threads (0 -> 1, at most 16); not a bit of the
 *   result depends on the count.  ms = 0.  n == 0 or a NULL pointer: GMUPT_ERR_INVALID_ARGUMENT, *info untouched.
 * gmupt_renderer_tree_cost: the rule on device memory.  nodes_or_null == NULL: the node buffer the renderer is bound to, as
 *   gmupt_renderer_refit keeps it current (GMUPT_ERR_NOT_BOUND without a scene).  Otherwise any GMUPT_BUFFER_BVH_NODES buffer of the
 *   renderer's device, bound or not -- e.g. the one gmupt_lbvh_build just returned; a scene need not be bound.  Another kind, another
 *   device, an empty buffer or more than 2^32 - 1 records: GMUPT_ERR_INVALID_ARGUMENT, as are a NULL renderer or info.  No error path
 *   allocates anything or writes *info.  The launches go on the renderer's stream, behind a preceding gmupt_renderer_refit or gmupt_iterate
 *   without a host wait: one thread per record, one block per run (k_tc_nodes), then one launch per further level over the partial
 *   results (k_tc_reduce) -- four launches at 20 M nodes; no float atomics.  Then ONE readback of 48 bytes and a synchronise.  The partial
 *   results live in scratch of the renderer (48 bytes per 256 records), allocated by the first call, grown when a larger buffer comes and
 *   kept.  ms = device time of the launches (hipEvents).  Bit for bit the result of gmupt_tree_cost_host on the same records.  The frame,
 *   path state, queues, counters, statistics, tables and the node buffer are not touched. */
typedef struct {
    double sum_inner, sum_leaf;
    uint32_t num_inner, num_leaves;
    uint64_t num_refs;
    uint32_t max_leaf_refs, pad;
    double root_half_area, sah;
    double ms;
} gmupt_tree_cost_info;   /* 64 bytes */
int gmupt_tree_cost_host(const gmupt_bvh_node* nodes, uint32_t n, gmupt_tree_cost_info* info, uint32_t threads);
int gmupt_renderer_tree_cost(gmupt_renderer* r, gmupt_buffer* nodes_or_null, gmupt_tree_cost_info* info);

/* ---- Tree optimisation: treelet restructuring of a node buffer, so that its tree cost falls (an extension; Karras & Aila 2013, "Fast
 * Parallel Construction of High-Quality Bounding Volume Hierarchies", section 3).  It is meant for the tree gmupt_lbvh_build returns,
 * between the build and gmupt_renderer_bind_scene, and is opt-in everywhere.  Only node records are read and written: the leaves keep
 * their triangle ranges and boxes, so the triangle buffer and ref_triangle of the tree stay valid as they are.
 *
 * The rule (gmupt_tree_optimize_host and the kernels run the same statements, csrc/pt_treeopt.hpp; binary64 for areas and costs, nothing
 * contracted; lo / hi and the union of two boxes as in the refit section).
 *   Input.  N >= 1 records that gmupt_renderer_bind_scene accepts as a tree: the root is record 0, an inner node (isLeaf == 0) has both
 *     children in (its own number, N), and every record but the root is the child of exactly one inner node -- otherwise
 *     GMUPT_ERR_INVALID_ARGUMENT.  Depth: root 0, a child one more than its parent; an input deeper than 64: GMUPT_ERR_UNSUPPORTED.
 *     passes in 1..8 (default 3), otherwise GMUPT_ERR_INVALID_ARGUMENT.
 *   Working copy.  The records under their input numbers, the "working ids"; links may then point to any working id.
 *   Cost, in the terms of the tree cost:  a(box) = (ex*ey + ey*ez) + ez*ex of the extents e = d > 0 ? d : 0, d = (double)max - (double)min.
 *     C(leaf) = a * (double)(uint32_t)(right - left).   C(inner) = a * 2.0 + (C(left) + C(right)).
 *   Processing an inner node X (all nodes below it have been processed in this pass):
 *     1. Treelet.  Slot 0 = X's left child, slot 1 = its right child.  While there are fewer than 7 slots and one of them holds an inner
 *        node: among those take the one whose box has the largest a -- slots scanned in ascending order, a later slot wins with a
 *        larger a, or with an equal a and a lower working id.  That node joins the treelet's inner nodes; its left child takes its
 *        slot, its right child the next free slot.  k = the number of slots at the end (2..7).
 *     2. X's box becomes the union of its children's boxes (left, then right), pad0 = pad1 = pad2 = 0;
 *        C(X) = a(X) * 2.0 + (C(left) + C(right)).  With k < 3 that is all.
 *     3. Programme over the non-empty subsets s of the slots, bit j of s = slot j.  a[s] = a of the box of the lowest slot in s with the
 *        other slots of s folded in by ascending slot (lo / hi per component).  c[{j}] = C(node of slot j).  For two slots or more:
 *        c[s] = a[s] * 2.0 + min over p of (c[p] + c[s \ p]), p running over the proper subsets of s that contain the lowest slot of s, in
 *        increasing numeric value; a candidate replaces the best one only when it is strictly smaller.  part[s] = that best p.
 *     4. Only when c[all] < C(X), strictly, the treelet is rewritten (the current topology is one of the candidates and evaluates to the
 *        same bits, so a tie keeps it).  Subset `all` is X, which keeps its id.  The k - 2 other inner ids of the old treelet are given,
 *        ascending, to the other subsets of two slots or more in pre-order of the new topology: a subset s has the left child part[s]
 *        and the right child s \ part[s]; a subset of one slot is that slot's node.  Then, children first, every inner node of the new
 *        treelet gets the box, the padding and the cost of step 2; its C equals c[its subset] bit for bit.
 *   A pass processes every inner node once, each after all nodes of its subtree.  A rewrite keeps the set of ids below X, and touches
 *     no node outside it but X, so the result does not depend on the order among nodes that are not below one another.  The depths as
 *     they were at the start of the pass are a valid schedule -- deepest first, any order within a depth -- because every id below X had a
 *     larger depth than X then and still lies below X when X's turn comes; a post-order recursion is another.
 *   After each pass the depths are recomputed.  A tree deeper than 64 after any pass: GMUPT_ERR_UNSUPPORTED (the pass does not rebalance).
 *   Output.  After the last pass the nodes are numbered by ascending (depth, working id): root = 0, children above their parent (siblings
 *     are not adjacent in general).  A leaf record is copied byte for byte; an inner record has its links renumbered.  Every inner box is
 *     the union of its children's, so gmupt_bvh_refit_host changes no byte of an optimised tree whose leaf boxes follow the refit rule.
 *   cost_before = C(root) of the input by step 2 alone (no rewrite), cost_after = C(root) after the last pass: what gmupt_tree_cost_host
 *     reports as sum_inner + sum_leaf, up to the order of the sum.  cost_after <= cost_before.  treelets_rewritten counts step 4 over all
 *     passes.  Non-finite boxes are no error; the comparisons above decide as they are written.
 * gmupt_tree_optimize_host: the rule on host arrays, no device; nodes_out holds n records and may be the input array.  info (may be
 *   NULL): ms = 0.  On an error nothing is written.
 * gmupt_treeopt: an optimiser handle of a device.  It owns a stream, two events and its scratch (working copy, staged output, parent links,
 *   costs, sort keys and storage: about 160 bytes per node), allocated by the first run, grown when a larger tree comes and kept.
 * gmupt_treeopt_run: nodes = a GMUPT_BUFFER_BVH_NODES buffer of the optimiser's device; it is not modified.  The whole run is enqueued on
 *   the optimiser's stream (it does not wait for other streams: finish the work that writes the buffer first, as gmupt_lbvh_build has when
 *   it returns): per pass a depth launch, a radix sort of (depth, id) and one launch per depth 63 .. 0, in which one wave handles one
 *   treelet with a[] and c[] in LDS; no launch waits for another workgroup of the same launch.  Then ONE small readback -- flags, depths,
 *   the rewrite count, the two costs -- and a synchronise.  On success *nodes_out is a new GMUPT_BUFFER_BVH_NODES buffer the caller
 *   destroys, bit for bit the array of gmupt_tree_optimize_host; on an error no buffer is created and *info is untouched.
 *   info->ms = device time of the run's launches (hipEvents). */
typedef struct { uint32_t passes; } gmupt_treeopt_params;
void gmupt_treeopt_default_params(gmupt_treeopt_params* p);
typedef struct { uint32_t num_nodes, depth_before, depth_after, treelets_rewritten; double cost_before, cost_after, ms; } gmupt_treeopt_info;   /* 40 bytes */
int gmupt_tree_optimize_host(const gmupt_bvh_node* nodes, uint32_t n, const gmupt_treeopt_params* params /* may be NULL */,
                             gmupt_bvh_node* nodes_out, gmupt_treeopt_info* info /* may be NULL */);
typedef struct gmupt_treeopt gmupt_treeopt;
int gmupt_treeopt_create(gmupt_device* dev, gmupt_treeopt** out);
void gmupt_treeopt_destroy(gmupt_treeopt* h);
int gmupt_treeopt_run(gmupt_treeopt* h, const gmupt_buffer* nodes, const gmupt_treeopt_params* params /* may be NULL */,
                      gmupt_buffer** nodes_out, gmupt_treeopt_info* info /* may be NULL */);

/* ---- Pose: linear-blend skinning and dense morph targets on the GPU (an extension; the reference's meshes never move).  It produces what
 * gmupt_normals_update, gmupt_renderer_refit and the motion-aware history start from -- "the vertex buffer holds the new pose" -- from a
 * few kilobytes per frame (joint matrices, target weights) instead of a vertex array.
 *
 * The rule (binary32, nothing contracted; gmupt_pose_host and the kernel run the same statements, csrc/pt_pose.hpp).  Input:
 *   num_verts rest positions R, 3 floats each;
 *   influences K in 1..8; per vertex K joint numbers (uint16_t) and K weights (float), vertex-major: joints[v*K + k], weights[v*K + k];
 *   num_joints J in 0..65535 joint matrices M, each 3 rows x 4 columns, row-major, 12 floats: M[j][c][i] = joint_mats[12*j + 4*c + i].  The
 *     caller supplies the joint's global transform times its inverse bind matrix;
 *   num_targets T in 0..256 dense morph targets D[t], 3 floats per vertex each: deltas[3*(t*num_verts + v) + c], and T target weights a.
 *   J == 0: morph only; K, joints, weights and joint_mats are ignored and may be 0 / NULL.  T == 0: skin only; deltas and target_weights
 *   may be NULL.  J == 0 together with T == 0 is an error.
 * For vertex v, per component:
 *   1. Morph.  m = R[v].  For t = 0 .. T-1 in ascending order, every target with a[t] != 0.0f: m = m + a[t] * D[t][v].  A target whose weight
 *      compares equal to zero (either sign) is skipped, not multiplied: 0 * inf would be a NaN, and the skip is what lets the kernel leave
 *      the memory of inactive targets alone.  A NaN weight is not equal to zero: the target counts.
 *   2. Skin (J > 0).  p = (0, 0, 0), any = false.  For k = 0 .. K-1 in ascending order, w = weights[v][k], j = joints[v][k], every influence
 *      with w != 0.0f:  q_c = ((M[j][c][0]*m.x + M[j][c][1]*m.y) + M[j][c][2]*m.z) + M[j][c][3]  for c = 0..2, then p_c = p_c + w * q_c and
 *      any = true.
 *   3. Result: p if any, else m -- a vertex without influences follows the morph only.  Weights are not normalised; that is the caller's
 *      business, as in glTF.  A skinned component that is -0 comes out as +0 (p starts from +0); an unskinned one keeps its sign.
 *   4. A joint number >= J on an influence whose weight is not zero is an error (at gmupt_pose_create for the device path).  The joint
 *      number of an influence of weight zero may be anything: it is never followed.
 *   5. Non-finite matrices, weights or deltas are no error; they propagate into the vertex.  gmupt_renderer_refit then refuses a non-finite
 *      vertex that a triangle uses, as it does for any vertex buffer; a later pose with finite input recovers.
 *   Only the 3 floats of the vertices 0 .. num_verts-1 are written.
 * gmupt_pose_host: the rule on host arrays, no device; verts_out holds 3 floats per vertex.  Up to `threads` std::threads (0 -> 1, at most
 *   16); the result does not depend on the count.  A NULL rest or verts_out, num_verts == 0, K outside 1..8 with J > 0, J or T beyond their
 *   limits, J == T == 0, a missing array, rule 4: GMUPT_ERR_INVALID_ARGUMENT, nothing written.
 * gmupt_pose: a handle of a renderer for one rig: it uses the renderer's device and stream and must not outlive the renderer.
 *   gmupt_pose_create: rest, joints, weights and deltas are caller-owned DEVICE memory in the layout above, finished by the caller, floats
 *   4-byte and joint numbers 2-byte aligned; the handle keeps its own copies.  It needs a bound scene (GMUPT_ERR_NOT_BOUND); num_verts =
 *   the element count of the bound vertex buffer.  One launch on the renderer's stream copies the rig into the handle's layout and checks
 *   rule 4, then ONE flag word is read back and the stream synchronised once; on an error no handle is created.  Device memory kept per
 *   vertex (the count rounded up to 64): 12 bytes of rest position, 6 per influence, 12 per target -- every component its own array, so
 *   that a wave reads whole rows in lane order; plus 48 bytes per joint, 12 per target and 64 bytes of words.  A pinned host staging area of
 *   48 * J + 4 * T bytes belongs to the handle too.
 * gmupt_pose_update: joint_mats (12 * J floats) and target_weights (T floats) are HOST pointers (NULL where the count is 0).  They are
 *   copied into the handle's pinned staging area and from there to the device on the renderer's stream; the call returns without waiting
 *   for the stream (it waits only for the staging area's previous copy, a few kilobytes, when that has not run yet).
 * gmupt_pose_update_device: the same with DEVICE pointers that the caller has finished and keeps unchanged until the renderer's stream has
 *   passed the call (gmupt_synchronize, or any call that synchronises): they are copied on that stream.
 * Both updates write the vertex buffer the renderer is bound to NOW (a rebind to buffers of the same vertex count needs no new handle).
 *   GMUPT_ERR_NOT_BOUND without a scene; a bound vertex count other than at create: GMUPT_ERR_INVALID_ARGUMENT, nothing written or copied.
 *   Two launches on the renderer's stream, ahead of a following gmupt_normals_update / gmupt_renderer_refit / gmupt_iterate without a host
 *   wait: one block that lists the targets whose weight is not zero, then one thread per vertex, which reads the deltas of those targets
 *   only; joint matrices sit in LDS up to 640 joints and are read from global memory above (the same statements).  No float atomics.
 *   info == NULL: no host synchronisation.  With info: synchronises; ms = device time of the copies and launches (hipEvents),
 *   active_targets = the number of target weights that are not zero.  Nothing else of the renderer is touched: as after any vertex update,
 *   call gmupt_renderer_refit before the next gmupt_iterate and restart the accumulation. */
typedef struct { uint32_t num_verts, active_targets; double ms; } gmupt_pose_info;   /* 16 bytes */
int gmupt_pose_host(const float* rest, uint32_t num_verts, const uint16_t* joints, const float* weights, uint32_t influences, const float* joint_mats,
                    uint32_t num_joints, const float* deltas, const float* target_weights, uint32_t num_targets, float* verts_out /* 3 per vertex */,
                    uint32_t threads);
typedef struct gmupt_pose gmupt_pose;
int gmupt_pose_create(gmupt_renderer* r, const float* device_rest, const uint16_t* device_joints, const float* device_weights, uint32_t influences,
                      uint32_t num_joints, const float* device_deltas, uint32_t num_targets, gmupt_pose** out);
int gmupt_pose_update(gmupt_pose* p, const float* joint_mats, const float* target_weights, gmupt_pose_info* info /* may be NULL */);
int gmupt_pose_update_device(gmupt_pose* p, const float* device_joint_mats, const float* device_target_weights, gmupt_pose_info* info /* may be NULL */);
void gmupt_pose_destroy(gmupt_pose* p);

/* ---- Convergence: a per-pixel error estimate of the accumulation and a stop rule built on it (an extension; the reference's Window::loop
 * renders until the window closes).  The accumulation keeps a running mean and a sample count per pixel and no second moment, and the
 * monitor does not change that: from two read-outs of a pixel the samples that arrived between them can be recovered -- n1*mean1 -
 * n0*mean0 is their sum -- so a sequence of read-outs gives BATCH MEANS.  Their weighted spread estimates the per-sample variance, and
 * with it the standard error of the pixel's mean.  Opt-in everywhere: no kernel of the renderer is changed or reads the monitor.
 *
 * The rule (gmupt_converge_host and the kernels run the same statements, csrc/pt_converge.hpp).  All arithmetic is IEEE, nothing
 * contracted, binary64 except where marked.
 *   State of a pixel: gmupt_converge_pixel, 40 bytes; all zero is the initial state.  n = the count at the last update that saw new
 *     samples, k = batches seen, w = samples in them, s = n * luminance then, mean / m2 = weighted mean of the batch means and the
 *     weighted sum of their squared deviations.
 *   Update of one pixel from its RGBA32F value (r, g, b, a):
 *     1. n1 = bits(a).  y = (0.2126f*r + 0.7152f*g) + 0.0722f*b in binary32: the denoiser's luminance.
 *     2. n1 < n: the accumulation restarted.  The state becomes all zero; continue.
 *     3. bsz = n1 - n.  bsz == 0: the state is unchanged.
 *     4. Otherwise, in this order:  s1 = (double)n1 * (double)y;  t = s1 - s;  B = t / (double)bsz;  w1 = w + bsz;  d = B - mean;
 *        mean1 = mean + ((double)bsz / (double)w1) * d;  m2 = m2 + ((double)bsz * d) * (B - mean1);
 *        then mean = mean1, s = s1, n = n1, w = w1, k = k + 1.
 *     5. Error.  k < 2: err = -1.0f, "unknown".  Otherwise v = (m2 / (double)(k - 1)) / (double)w;  if (v < 0) v = 0 (a NaN stays a
 *        NaN);  err = sqrtf((float)v), the correctly rounded binary32 root.  The sign and payload of a NaN -- in s, mean, m2 or err -- are
 *        not part of the rule.
 *   Summary (gmupt_converge_info) under gmupt_converge_params { threshold, min_batches >= 2, allow_pixels }:
 *     pixels      the pixels of the image
 *     unsampled   pixels with n1 == 0
 *     known       pixels with k >= 2 after the update
 *     nonfinite   known pixels whose err is NaN or inf
 *     below       pixels with k >= min_batches, err finite and err <= threshold
 *     max_error   the largest finite err of a known pixel; 0 when there is none
 *     sum_error   the binary64 sum of the finite err values of the known pixels in pixel order, every other pixel contributing +0.0.
 *                 Order of the sum: the one "Tree cost" states -- the entries padded with +0.0 to a multiple of 256, every run of 256
 *                 reduced by stride halving (s = 128 .. 1: x[i] = x[i] + x[i+s] for i < s), the results in run order being the entries
 *                 of the next level, until one value is left.
 *     mean_error  sum_error / (known - nonfinite); 0 when that count is 0
 *     converged   1 when pixels - below <= allow_pixels, else 0
 *     ms          device time of the launches (hipEvents); 0 from gmupt_converge_host
 *   Defaults (gmupt_converge_default_params): threshold = 0, min_batches = 2, allow_pixels = 0 -- with these a call only reports;
 *     there is no default threshold.
 *   Meaning.  err estimates the standard error of the mean of the pixel's tone-mapped, gamma-encoded luminance -- the samples are
 *     tone-mapped before they are averaged (logic.hlsl:49-73), so a threshold is in display units ("below one 8-bit step" = 1/255) --
 *     and nothing more: not the error of the radiance, not the bias of a clamped sample, not what a denoiser leaves.  A pixel whose
 *     batches were all equal has err == 0; unsampled pixels never become known and so never count as below.
 *   Noise floor.  The target holds the mean in binary32, so n1*y carries a relative error of about 2^-24 of the SUM; a batch mean
 *     recovered from two such sums is off by about (n / bsz) * 2^-24 relative.  Short batches late in a long accumulation measure that
 *     rounding, not the renderer: keep bsz a fixed fraction of n (check less often as the count grows) when thresholds near 1e-5 matter.
 *   Missed restart.  A restart followed by re-accumulation PAST the old count between two updates cannot be told from the counts
 *     alone (n1 >= n).  gmupt_converge_update does not rely on the counts for it, see below; gmupt_converge_update_image and
 *     gmupt_converge_host have step 2 only, and their caller calls gmupt_converge_reset (or zeroes the state) after such a restart.
 * gmupt_converge_host: the rule on host arrays, no device: state = width*height records the call updates, rgba = as many RGBA32F
 *   texels, error_or_null = as many floats.  ms = 0.
 * gmupt_converge: a handle of a renderer: it uses the renderer's device and stream and must not outlive the renderer.  The state is
 *   a structure of arrays in device memory (36 bytes per pixel) together with the partial summaries (32 bytes per 256 pixels),
 *   allocated zeroed by the first update and again when the image size changes.
 * gmupt_converge_update: the rule on the renderer's accumulation target (the tile of a tile renderer), on the renderer's stream behind
 *   pending gmupt_iterate work and without a host wait before the launches: one thread per pixel, one block per run (k_cv_update), then
 *   one launch per further level over the partial summaries (k_cv_reduce); no atomics.  Then ONE readback of 32 bytes and a
 *   synchronise.  Every pixel restarts (the state is zeroed on the stream first) when the renderer's accumulation generation -- advanced
 *   by an iteration that clears the frame and by gmupt_resize -- differs from the one the previous gmupt_converge_update saw, when the
 *   frame size changed, and on the first gmupt_converge_update after a gmupt_converge_update_image.  device_error_or_null: width*height
 *   floats of device memory, 4-byte aligned, that receive err per pixel.
 * gmupt_converge_update_image: the same on caller-owned device memory (16-byte aligned, finished by the caller), e.g. a gathered frame
 *   or a torch tensor; 1 <= width*height < 2^32.  Restarts are step 2's and a changed image size only: called after a
 *   gmupt_converge_update of the same size it CONTINUES the state of the renderer's target.  Do not feed one handle from both sources
 *   without a gmupt_converge_reset in between, or use a handle per source.
 * gmupt_converge_reset: zeroes the state on the stream.  gmupt_converge_read_state: the state as width*height 40-byte records (pad = 0)
 *   for tests; 0 records before the first update; synchronises.
 * gmupt_render_until: the loop of gmupt_render_budget (camera update, upload, iterate) with gmupt_converge_update after every
 *   check_every iterations; ends when a check reports converged, after max_iterations (the last iteration is followed by a check
 *   only when it completes a group of check_every), or on an error; GMUPT_ERR_CAST_FAULT is checked at every check and at the end.
 *   *iters = iterations run.  *info = the last check's summary; it is written only when a check ran.  A path_budget is not needed.
 * Errors: GMUPT_ERR_INVALID_ARGUMENT for a NULL handle, info, state or image, min_batches < 2, a NaN threshold, a misaligned device
 *   pointer, an empty or too large image, bytes too small, check_every == 0.  No error path allocates anything or writes *info.  The
 *   frame, path state, queues, counters, statistics and traversal tables are never written. */
typedef struct { uint32_t n, k, w, pad; double s, mean, m2; } gmupt_converge_pixel;   /* 40 bytes */
typedef struct { float threshold; uint32_t min_batches, allow_pixels; } gmupt_converge_params;   /* 12 bytes */
typedef struct {
    uint32_t pixels, unsampled, known, nonfinite, below, converged;
    float max_error; uint32_t pad;
    double sum_error, mean_error, ms;
} gmupt_converge_info;   /* 56 bytes */
void gmupt_converge_default_params(gmupt_converge_params* p);
int gmupt_converge_host(gmupt_converge_pixel* state, const float* rgba, uint32_t width, uint32_t height, const gmupt_converge_params* params /* may be NULL */,
                        float* error_or_null, gmupt_converge_info* info);
typedef struct gmupt_converge gmupt_converge;
int gmupt_converge_create(gmupt_renderer* r, gmupt_converge** out);
void gmupt_converge_destroy(gmupt_converge* c);
int gmupt_converge_reset(gmupt_converge* c);
int gmupt_converge_update(gmupt_converge* c, const gmupt_converge_params* params /* may be NULL */, float* device_error_or_null, gmupt_converge_info* info);
int gmupt_converge_update_image(gmupt_converge* c, const float* device_rgba, uint32_t width, uint32_t height, const gmupt_converge_params* params /* may be NULL */,
                                float* device_error_or_null, gmupt_converge_info* info);
int gmupt_converge_read_state(gmupt_converge* c, gmupt_converge_pixel* dst, size_t bytes);
int gmupt_render_until(gmupt_renderer* r, gmupt_camera* camera, gmupt_converge* c, const gmupt_converge_params* params /* may be NULL */,
                       uint32_t check_every, uint32_t max_iterations, uint32_t* iters /* may be NULL */, gmupt_converge_info* info);

/* ---- Adaptive sampling (an extension): new camera paths go where the convergence monitor's error still is.  Its rule, structures
 * and functions are declared in include/gmupt_adaptive.h, which includes this file.  Opt-in everywhere: without a sampling plan
 * attached to a renderer an iteration launches exactly what it launched before, and no kernel of the renderer is changed.
 * The AOV, denoiser, temporal and infill stages need no change under a plan: they read the per-pixel running mean and count of the
 * accumulation target, which stay valid under uneven counts. */

/* ---- Lens (an extension): depth of field.  A thin lens attached to a renderer moves the origin of every fresh camera path onto a disk
 * around the camera position and aims it through the focal plane, in one extra launch after the shading stage.  Its rule, structure and
 * functions are declared in include/gmupt_lens.h, which includes this file.  Opt-in everywhere: without a lens, or at aperture 0, an
 * iteration launches exactly what it launched before.  gmupt_pick, gmupt_camera_pick_ray, the AOV rays, the motion plane and the
 * temporal projection stay on the pinhole centre ray. */

/* ---- test / debug access (reference path-state layout, structs.h:19-48) ---- */
int gmupt_debug_read_path_state(gmupt_renderer* r, void* dst, size_t bytes);        /* 248 * pool_paths */
int gmupt_debug_write_path_state(gmupt_renderer* r, const void* src, size_t bytes);
int gmupt_debug_read_queues(gmupt_renderer* r, uint32_t* dst, size_t bytes);        /* 5 * pool_paths u32, structs.h:53-58 */
int gmupt_debug_write_queues(gmupt_renderer* r, const uint32_t* src, size_t bytes);
int gmupt_debug_write_counters(gmupt_renderer* r, const uint32_t in[8]);
int gmupt_debug_write_framebuffer(gmupt_renderer* r, const float* rgba, size_t bytes);
typedef enum { GMUPT_STAGE_SHADE = 0 /* logic+newPath+materialUE4+materialGlass */, GMUPT_STAGE_EXTEND = 1, GMUPT_STAGE_SHADOW = 2,
               GMUPT_STAGE_RAYCASTS = 3 /* both ray casts as gmupt_iterate launches them (one fused launch by default) */ } gmupt_stage;
int gmupt_debug_run_stage(gmupt_renderer* r, gmupt_stage stage);
/* evaluates the device copy of the deterministic math (fn: 0 sin, 1 cos, 2 log2, 3 exp2, 4 pow(x,y), 5 frac, 6 rng probe) */
int gmupt_debug_detmath(gmupt_device* dev, int fn, const float* x, const float* y, float* out, uint32_t n);

/* The traversal tables a bind would build from these host arrays (csrc/pt_travtables.hpp), without a device: numbering switches as
 * arguments instead of GMUPT_TOP_ORDER / GMUPT_NODE_PAIRING, LDS capacities of this build.  gmupt_debug_travtables_data returns the bytes
 * of one table or map (owned by the handle; NULL and 0 bytes for an empty one or for GMUPT_TT_REC64 outside a -DGMUPT_VARIANTS build).
 * GMUPT_TT_SCALARS: 15 words -- topCount, topCountDeep, maxDepth, rootDesc, rootMin[3], rootMax[3], triBase, wideTopCount,
 * wideStackBound, numPairs, wideCount.  A malformed tree: the message of gmupt_renderer_bind_scene, GMUPT_ERR_INVALID_ARGUMENT. */
typedef struct gmupt_travtables gmupt_travtables;
typedef enum { GMUPT_TT_NODE64 = 0, GMUPT_TT_TRI48 = 1, GMUPT_TT_TRIPAIR = 2, GMUPT_TT_PAIRREF = 3, GMUPT_TT_WNODE = 4, GMUPT_TT_REC64 = 5,
               GMUPT_TT_SCALARS = 6, GMUPT_TT_LEVEL_NODES = 7, GMUPT_TT_LEVEL_OFF = 8, GMUPT_TT_NODE_MAP = 9, GMUPT_TT_WIDE_MAP = 10,
               GMUPT_TT_OPENED = 11 } gmupt_travtable_kind;
int gmupt_debug_travtables_build(const gmupt_bvh_node* nodes, uint32_t num_nodes, const gmupt_triangle* tris, uint32_t num_tris,
                                 const float* verts, uint32_t num_verts, int want_wide, int top_order_bfs, int node_pairing, gmupt_travtables** out);
const void* gmupt_debug_travtables_data(const gmupt_travtables* h, int which /* gmupt_travtable_kind */, size_t* bytes);
void gmupt_debug_travtables_destroy(gmupt_travtables* h);
/* The same kinds read back from a renderer with a bound scene: the device tables as bind uploaded and refit rewrote them (GMUPT_TT_TRI48:
 * the references and their sentinel; GMUPT_TT_REC64 in a -DGMUPT_VARIANTS build only), GMUPT_TT_SCALARS from the renderer's own copy of the
 * 15 words above, the five maps from the host vectors the renderer keeps for refit.  Waits for the renderer's stream, sets *needed to the
 * size of that table and copies it to dst when bytes >= *needed; dst == NULL with bytes == 0 asks for the size only.  A table the renderer
 * does not hold (no wide copy: WNODE, TRIPAIR and PAIRREF, whose pairs then stay on the host; REC64 in the shipped build) has
 * *needed = 0 and succeeds.  Errors: NULL renderer or `needed`, a buffer smaller than *needed (nothing written), an unknown kind:
 * GMUPT_ERR_INVALID_ARGUMENT; no scene bound: GMUPT_ERR_NOT_BOUND.  It touches no frame, path state, queue, counter, statistic or table. */
int gmupt_debug_read_travtable(gmupt_renderer* r, int which /* gmupt_travtable_kind */, void* dst, size_t bytes, size_t* needed);
/* 1 when tables of these sizes are within the wide ray cast's signed 32-bit byte offsets -- wide_nodes * 128, (num_tris + 1) * 48 (the
 * references and their sentinel record) and num_pairs * 80 all below 2^31 -- else 0.  The one rule behind the renderer's choice of the wide
 * kernel and behind GMUPT_ERR_UNSUPPORTED of the ray queries; no device involved. */
int gmupt_debug_wide_tables_addressable(uint32_t wide_nodes, uint32_t num_tris, uint32_t num_pairs);

/* ---- host side: SBVH build + flatten (replaces BVHWrapper::buildSBVH, Source/BVHWrapper.cpp:13-96, and the vendored Nvidia-SBVH builder) ---- */
typedef struct {
    float split_alpha;       /* BVH::BuildParams::splitAlpha = 1e-5 (Include/Nvidia-SBVH/BVH.h:77) */
    int32_t max_depth;       /* SplitBVHBuilder::MaxDepth = 64 */
    int32_t max_spatial_depth; /* MaxSpatialDepth = 48 */
    int32_t min_leaf_size;   /* Platform default 1 */
    int32_t max_leaf_size;   /* Platform default 0x7FFFFFF */
    float node_cost, tri_cost; /* Platform default 1, 1 */
} gmupt_sbvh_params;
void gmupt_sbvh_default_params(gmupt_sbvh_params* p);
typedef struct gmupt_sbvh gmupt_sbvh;
/* vertices: numVerts tightly packed float3; indices: numTris * 3 vertex indices */
int gmupt_sbvh_build(const float* vertices, uint32_t num_vertices, const int32_t* indices, uint32_t num_triangles,
                     const gmupt_sbvh_params* params, gmupt_sbvh** out);
uint32_t gmupt_sbvh_num_nodes(const gmupt_sbvh* h);
uint32_t gmupt_sbvh_num_references(const gmupt_sbvh* h);
float gmupt_sbvh_sah(const gmupt_sbvh* h);
uint32_t gmupt_sbvh_depth(const gmupt_sbvh* h);
/* flattened reference layout; vertex_material may be NULL (materialID 0). ref_triangle (optional) receives the source triangle of each reference */
int gmupt_sbvh_flatten(const gmupt_sbvh* h, const uint32_t* vertex_material, gmupt_bvh_node* nodes, gmupt_triangle* triangles, int32_t* ref_triangle);
void gmupt_sbvh_destroy(gmupt_sbvh* h);

/* ---- host side: camera (replaces Camera::updateResolution / update / setRotation, Source/Camera.cpp) ---- */
int gmupt_camera_create(uint32_t width, uint32_t height, gmupt_camera** out);
void gmupt_camera_destroy(gmupt_camera* c);
void gmupt_camera_update_resolution(gmupt_camera* c, uint32_t width, uint32_t height);
void gmupt_camera_set_pose(gmupt_camera* c, float x, float y, float z, float pitch, float yaw); /* Scene.cpp:95-97 */
void gmupt_camera_update(gmupt_camera* c, float dt); /* Camera::update without input devices */
void gmupt_camera_reset_accumulation(gmupt_camera* c); /* iterationCounter = -1 (Renderer.cpp:152) */
/* input for the next gmupt_camera_update calls: mouse delta in degrees (yaw += dx, pitch -= dy, consumed by one update; Camera.cpp:28-33) and the
 * W/S/A/D key states (bit 0..3, held until changed; 5 units/s, :47-57).  Any input restarts the accumulation by the reference's
 * hysteresis rule (:72-83): iterationCounter -> 0 when it is > 4, and once more when the motion has stopped. */
void gmupt_camera_set_input(gmupt_camera* c, float mouse_dx, float mouse_dy, uint32_t keys_wsad);
gmupt_camera_buffer* gmupt_camera_get_buffer(gmupt_camera* c);

const char* gmupt_version(void);

#ifdef __cplusplus
}
#endif
#endif
