// C-ABI of libgmupt.so (see include/gmupt.h for the contract and the reference call sites each entry replaces).
// Host code only; the kernels live in pt_kernels.hip.
#include "pt_device.hpp"
#include "detmath.hpp"
#include "pt_shading.hpp"
#include "pt_denoise.hpp"
#include "pt_temporal.hpp"
#include "pt_refit.hpp"
#include "pt_motion.hpp"
#include "pt_travtables.hpp"
#include "pt_lbvh.hpp"
#include "../host/sbvh_builder.hpp"
#include "../host/Camera.hpp"
#include "../host/TextureLoader.hpp"
#include "../host/png_reader.hpp"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <unordered_map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

static_assert(sizeof(gmupt_bvh_node) == 48, "BVHNode is 48 bytes (Include/BVHWrapper.hpp:13-21)");
static_assert(sizeof(gmupt_triangle) == 16, "Triangle is 16 bytes (Include/BVHWrapper.hpp:23-27)");
static_assert(sizeof(gmupt_tri_props) == 32, "TriangleProperties is 32 bytes (Include/BVHWrapper.hpp:29-34)");
static_assert(sizeof(gmupt_light) == 32, "Light is 32 bytes (Include/Scene.hpp:13-19)");
static_assert(sizeof(gmupt_material) == 48, "MaterialProperty is 48 bytes (Include/Scene.hpp:43-68)");
static_assert(sizeof(gmupt_camera_buffer) == 112, "CameraBuffer is 112 bytes (Include/Camera.hpp:8-22)");
static_assert(offsetof(gmupt_camera_buffer, pixelSize) == 64 && offsetof(gmupt_camera_buffer, randomSeed) == 72 &&
              offsetof(gmupt_camera_buffer, envColor) == 80 && offsetof(gmupt_camera_buffer, iterationCounter) == 96 &&
              offsetof(gmupt_camera_buffer, lightCount) == 100 && offsetof(gmupt_camera_buffer, sampleLights) == 104, "Cam cbuffer offsets (structs.h:163-180)");
static_assert(offsetof(gmupt_bvh_node, max) == 16 && offsetof(gmupt_bvh_node, left) == 32 && offsetof(gmupt_bvh_node, isLeaf) == 40, "BVHNode offsets");
static_assert(offsetof(gmupt_material, metallic) == 16 && offsetof(gmupt_material, textureIndices) == 32 && offsetof(gmupt_material, materialType) == 44, "MaterialProperty offsets");

namespace gmupt {
void launch_clear(const RenderParams& p, hipStream_t s);
void launch_logic(const RenderParams& p, hipStream_t s);
void launch_material(const RenderParams& p, int clearFrame, hipStream_t s);
uint32_t launch_extend(const RenderParams& p, uint32_t blocks, bool stats, int mode, hipStream_t s);   // the launch_* of the ray casts return GMUPT_STAT_* bits of what they launched
uint32_t launch_shadow(const RenderParams& p, uint32_t blocks, bool stats, int mode, hipStream_t s);
uint32_t launch_cast(const RenderParams& p, bool stats, int mode, hipStream_t s);                      // 0: not launched, run the two separate casts
bool traversal_is_fused(int mode);
bool traversal_mode_available(int mode);
void launch_detmath(int fn, const float* x, const float* y, float* out, uint32_t n, hipStream_t s);
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
void denoise_host(const float* beauty, const void* aov, int W, int H, const DnParams& prm, float* out, int threads);
void launch_temporal(const float4* beauty, const float4* aov, int W, int H, const TpPrev& prev, const TpParams& prm, float4* out, float4* hist,
                     hipStream_t s);
void launch_temporal_motion(const float4* beauty, const float4* aov, const float4* motion, int W, int H, const TpPrev& prev, const TpParams& prm,
                            float4* out, float4* hist, hipStream_t s);
void launch_mv_resolve(const SceneView& scene, const float* prevVerts, uint32_t npix, uint32_t R, const gmupt_hit* hits, const gmupt_aov* aov,
                       gmupt_motion* out, hipStream_t s);
void motion_host(const gmupt_hit* hits, const gmupt_aov* aov, size_t n, const gmupt_triangle* tris, const float* now, const float* prev, gmupt_motion* out);
void temporal_host(const float* beauty, const void* aov, const void* motion, int W, int H, const void* prev, const gmupt_camera_buffer* prevCam, int px0, int py0,
                   int pW, int pH, const TpParams& prm, float* out, void* outHist, int threads);
void launch_refit_check(const RfArgs& a, hipStream_t s);
uint32_t launch_refit_boxes(const RfArgs& a, const std::vector<uint32_t>& levelOff, hipStream_t s);
void launch_refit_tables(const RfArgs& a, hipStream_t s);
void refit_host(gmupt_bvh_node* nodes, size_t N, const gmupt_triangle* tris, const float* verts, int threads);
hipError_t lbvh_sort_temp_bytes(uint32_t n, size_t* bytes);
LbScratch lbvh_scratch_layout(uint32_t n, size_t sortTemp);
hipError_t launch_lbvh(void* scratch, const LbScratch& off, size_t sortTemp, const float* verts, uint32_t numVerts, const int32_t* indices, uint32_t n,
                       const uint32_t* vertexMaterial, uint32_t maxLeaf, hipStream_t s, LbStaging& st);
}
using namespace gmupt;

// ------------------------------------------------------------------------------------------------ errors
static thread_local std::string g_lastError;

static int fail(int code, const char* fmt, ...)
{
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    g_lastError = buf;
    return code;
}
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(GMUPT_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

extern "C" const char* gmupt_last_error(void) { return g_lastError.c_str(); }
extern "C" const char* gmupt_version(void) { return "gmupt 0.1 (gfx950)"; }

// ------------------------------------------------------------------------------------------------ device
struct gmupt_device { int id; hipDeviceProp_t prop; };

extern "C" int gmupt_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(GMUPT_ERR_HIP, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
    return n;
}

extern "C" int gmupt_device_create(int hip_device, gmupt_device** out)
{
    if (!out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_device_create: out is null");
    *out = nullptr;
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (hip_device < 0 || hip_device >= n) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_device_create: device %d of %d", hip_device, n);
    gmupt_device* d = new (std::nothrow) gmupt_device();
    if (!d) return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_device_create: out of host memory");
    d->id = hip_device;
    hipError_t e = hipSetDevice(hip_device);
    if (e == hipSuccess) e = hipGetDeviceProperties(&d->prop, hip_device);
    if (e != hipSuccess) { delete d; return fail(GMUPT_ERR_HIP, "device %d: %s", hip_device, hipGetErrorString(e)); }
    *out = d;
    return GMUPT_OK;
}

extern "C" void gmupt_device_destroy(gmupt_device* dev) { delete dev; }

// ------------------------------------------------------------------------------------------------ buffers
struct gmupt_buffer { gmupt_device* dev; gmupt_buffer_kind kind; void* dptr; size_t bytes; size_t elems; uint32_t texSize = 0, texLayers = 0; };

static size_t kind_stride(gmupt_buffer_kind k)
{
    switch (k) {
    case GMUPT_BUFFER_BVH_NODES: return 48; case GMUPT_BUFFER_TRIANGLES: return 16; case GMUPT_BUFFER_VERTICES: return 12;
    case GMUPT_BUFFER_LIGHTS: return 32; case GMUPT_BUFFER_TRI_PROPS: return 32; case GMUPT_BUFFER_MATERIALS: return 48;
    case GMUPT_BUFFER_TEXTURE_ARRAY: return 4;
    }
    return 0;
}

extern "C" int gmupt_buffer_create(gmupt_device* dev, gmupt_buffer_kind kind, const void* data, size_t bytes, gmupt_buffer** out)
{
    if (!dev || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_buffer_create: null argument");
    *out = nullptr;
    const size_t stride = kind_stride(kind);
    if (!stride) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_buffer_create: unknown kind %d", (int)kind);
    if (bytes % stride) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_buffer_create: %zu bytes is not a multiple of the %zu-byte element", bytes, stride);
    if (bytes && !data) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_buffer_create: data is null");
    size_t alloc = bytes;
    // lights / materials live in fixed 128-entry tables (Scene.hpp:116, logic.hlsl:8); entries past the data are zero
    if (kind == GMUPT_BUFFER_LIGHTS || kind == GMUPT_BUFFER_MATERIALS) {
        if (bytes > stride * GMUPT_MAX_LIGHTS) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_buffer_create: more than %d entries", GMUPT_MAX_LIGHTS);
        alloc = stride * GMUPT_MAX_LIGHTS;
    }
    if (alloc == 0) alloc = stride;
    gmupt_buffer* b = new (std::nothrow) gmupt_buffer();
    if (!b) return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_buffer_create: out of host memory");
    b->dev = dev; b->kind = kind; b->bytes = alloc; b->elems = bytes / stride; b->dptr = nullptr;
    hipError_t e = hipSetDevice(dev->id);
    if (e == hipSuccess) e = hipMalloc(&b->dptr, alloc + 16); // +16: 12-byte vertices are read with in-bounds dword loads only, slack is for safety
    if (e == hipSuccess) e = hipMemset(b->dptr, 0, alloc + 16);
    if (e == hipSuccess && bytes) e = hipMemcpy(b->dptr, data, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { if (b->dptr) (void)hipFree(b->dptr); delete b; return fail(GMUPT_ERR_HIP, "gmupt_buffer_create(%zu bytes): %s", alloc, hipGetErrorString(e)); }
    *out = b;
    return GMUPT_OK;
}

extern "C" int gmupt_image_decode_png(const void* png, size_t bytes, uint32_t* width, uint32_t* height, uint8_t** rgba)
{
    if (!png || !width || !height || !rgba) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_image_decode_png: null argument");
    *rgba = nullptr; *width = *height = 0;
    try {
        gmupt::png::Image img = gmupt::png::decode(static_cast<const uint8_t*>(png), bytes);
        uint8_t* mem = static_cast<uint8_t*>(std::malloc(img.rgba.size()));
        if (!mem) return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_image_decode_png: out of host memory");
        std::memcpy(mem, img.rgba.data(), img.rgba.size());
        *rgba = mem; *width = img.width; *height = img.height;
    } catch (const std::exception& e) { return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_image_decode_png: %s", e.what()); }
    return GMUPT_OK;
}

extern "C" void gmupt_image_free(uint8_t* rgba) { std::free(rgba); }

extern "C" int gmupt_image_resize_square(const uint8_t* rgba, uint32_t old_size, uint32_t new_size, uint8_t* dst)
{
    if (!rgba || !dst || old_size == 0 || new_size == 0) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_image_resize_square: null or empty argument");
    try {
        const std::vector<uint8_t> out = gmupt::resizeSquare(rgba, old_size, new_size);
        std::memcpy(dst, out.data(), out.size());
    } catch (const std::exception& e) { return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_image_resize_square: %s", e.what()); }
    return GMUPT_OK;
}

extern "C" uint32_t gmupt_texture_common_size(const size_t* layer_bytes, uint32_t layers)
{
    if (!layer_bytes || layers == 0) return 0;
    return gmupt::commonDimension(std::vector<size_t>(layer_bytes, layer_bytes + layers));
}

extern "C" int gmupt_texture_array_create(gmupt_device* dev, const uint8_t* rgba8, uint32_t size, uint32_t layers, gmupt_buffer** out)
{
    if (!dev || !out || !rgba8) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_texture_array_create: null argument");
    if (size == 0 || layers == 0 || size > 16384) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_texture_array_create: %u layers of %ux%u", layers, size, size);
    int rc = gmupt_buffer_create(dev, GMUPT_BUFFER_TEXTURE_ARRAY, rgba8, (size_t)size * size * layers * 4, out);
    if (rc == GMUPT_OK) { (*out)->texSize = size; (*out)->texLayers = layers; }
    return rc;
}

extern "C" int gmupt_buffer_update(gmupt_buffer* buf, const void* data, size_t bytes)
{
    if (!buf || (!data && bytes)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_buffer_update: null argument");
    if (bytes > buf->bytes) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_buffer_update: %zu bytes into a %zu-byte buffer", bytes, buf->bytes);
    HIP_TRY(hipSetDevice(buf->dev->id));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(buf->dptr, data, bytes, hipMemcpyHostToDevice));
    return GMUPT_OK;
}

extern "C" int gmupt_buffer_read(const gmupt_buffer* buf, void* dst, size_t bytes)
{
    if (!buf || (!dst && bytes)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_buffer_read: null argument");
    if (bytes > buf->bytes) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_buffer_read: %zu bytes from a %zu-byte buffer", bytes, buf->bytes);
    HIP_TRY(hipSetDevice(buf->dev->id));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(dst, buf->dptr, bytes, hipMemcpyDeviceToHost));
    return GMUPT_OK;
}

extern "C" void gmupt_buffer_destroy(gmupt_buffer* buf)
{
    if (!buf) return;
    (void)hipSetDevice(buf->dev->id);
    (void)hipFree(buf->dptr);
    delete buf;
}

extern "C" size_t gmupt_buffer_size(const gmupt_buffer* buf) { return buf ? buf->bytes : 0; }

// ------------------------------------------------------------------------------------------------ renderer
struct StageEvents { hipEvent_t e[5]; bool extOnly = false; };   // logic | material | ray cast (extension) | shadow

struct gmupt_renderer {
    gmupt_device* dev = nullptr;
    gmupt_renderer_desc desc{};
    hipStream_t stream = nullptr;
    RenderParams p{};
    bool sceneBound = false, cameraSet = false;
    uint64_t iterations = 0;
    uint32_t travBlocks = 0;
    // timing
    int timing = 0; // 0 off, 1 all stages, 2 only the extension ray cast (two events per iteration)
    std::vector<StageEvents> evPool; size_t evUsed = 0;
    double msStage[4] = { 0, 0, 0, 0 }; uint64_t timedIters = 0;
    std::vector<void*> allocs;
    // packed traversal copy of the bound scene
    void* travNodes = nullptr; void* travTris = nullptr; void* travRecs = nullptr; void* travWide = nullptr; void* travPairs = nullptr; void* travPairRef = nullptr;
    size_t travBytes[6] = { 0, 0, 0, 0, 0, 0 }; // bytes uploaded to each, in the order of trav_tables() (gmupt_debug_read_travtable)
    int travMode = 70; // GMUPT_TRAVERSAL: "wide" (default) both ray casts in one launch over the 4-wide collapse | "cast0" the same over the binary tree | "def0" separate launches; the other rungs of the ladder exist in -DGMUPT_VARIANTS builds only
    uint32_t castFlags = 0; // GMUPT_STAT_* bits of the ray-cast kernels launched since the last reset
    // ray queries (gmupt_trace_rays): work counters + statistics of their own, allocated on first use; one ray + one hit for gmupt_pick
    uint32_t* queryCounters = nullptr; DevStats* queryStats = nullptr; void* pickBuf = nullptr;
    hipEvent_t queryEv[2] = { nullptr, nullptr };
    // AOV buffers (gmupt_render_aovs): rays and hits of one chunk (GMUPT_AOV_CHUNK_RAYS each, 128 MiB), allocated on first use
    gmupt_ray* aovRays = nullptr; gmupt_hit* aovHits = nullptr;
    // denoiser (gmupt_denoise_image): the filter's scratch (kDnScratchBytes per pixel) and, for gmupt_render_denoised, the AOV records and
    // the framebuffer copy (80 bytes per pixel); allocated on first use, grown when a larger image comes, freed by gmupt_renderer_destroy
    void* dnScratch = nullptr; size_t dnScratchBytes = 0;
    void* dnInput = nullptr; size_t dnInputBytes = 0;
    hipEvent_t dnEv[2] = { nullptr, nullptr };
    // temporal reuse (gmupt_render_denoised_temporal): advanced by an iteration that clears the frame and by gmupt_resize (host only)
    uint64_t accumGeneration = 0;
    // motion (gmupt_render_denoised_temporal_motion): which binding the renderer has and how many refits it has seen (host only)
    uint64_t bindingId = 0, geomGeneration = 0;
    // refit (gmupt_renderer_refit): the buffers of the binding with their element counts, and what build_trav_tables (pt_travtables.hpp) knows about the
    // topology of its tables -- host vectors, uploaded into one allocation (rfDev) by the first refit after a bind
    const gmupt_buffer* boundNodes = nullptr; const gmupt_buffer* boundTris = nullptr; const gmupt_buffer* boundVerts = nullptr;
    size_t boundElems[3] = { 0, 0, 0 };
    std::vector<uint32_t> rfLevelNodes, rfLevelOff, rfNodeMap, rfWideMap, rfOpened;
    void* rfDev = nullptr;
    hipEvent_t rfEv[2] = { nullptr, nullptr };
};

// the renderer's six device tables, in the order build_traversal_copy fills them
static std::array<void**, 6> trav_tables(gmupt_renderer* r) { return { &r->travNodes, &r->travTris, &r->travRecs, &r->travWide, &r->travPairs, &r->travPairRef }; }

static int dev_alloc(gmupt_renderer* r, void** ptr, size_t bytes, int fill)
{
    *ptr = nullptr;
    HIP_TRY(hipMalloc(ptr, bytes ? bytes : 16));
    r->allocs.push_back(*ptr);
    HIP_TRY(hipMemsetAsync(*ptr, fill, bytes ? bytes : 16, r->stream));
    return GMUPT_OK;
}

static int alloc_framebuffer(gmupt_renderer* r, uint32_t w, uint32_t h)
{
    void* fb = nullptr; void* head = nullptr;
    const size_t npix = (size_t)w * h;
    HIP_TRY(hipMalloc(&fb, npix * 16 + 16));
    HIP_TRY(hipMalloc(&head, npix * 4 + 16));
    HIP_TRY(hipMemsetAsync(fb, 0, npix * 16 + 16, r->stream));        // createRenderTexture: no initial data => zero
    HIP_TRY(hipMemsetAsync(head, 0xFF, npix * 4 + 16, r->stream));
    r->p.fb = (float4*)fb; r->p.listHead = (uint32_t*)head; r->p.fbW = w; r->p.fbH = h;
    return GMUPT_OK;
}

extern "C" void gmupt_renderer_destroy(gmupt_renderer* r)
{
    if (!r) return;
    (void)hipSetDevice(r->dev->id);
    if (r->stream) (void)hipStreamSynchronize(r->stream);
    for (auto& se : r->evPool) for (auto& e : se.e) (void)hipEventDestroy(e);
    for (hipEvent_t e : r->queryEv) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : r->dnEv) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : r->rfEv) if (e) (void)hipEventDestroy(e);
    if (r->rfDev) (void)hipFree(r->rfDev);
    for (void* a : r->allocs) (void)hipFree(a);
    if (r->dnScratch) (void)hipFree(r->dnScratch);
    if (r->dnInput) (void)hipFree(r->dnInput);
    if (r->p.fb) (void)hipFree(r->p.fb);
    if (r->p.listHead) (void)hipFree(r->p.listHead);
    for (void** t : trav_tables(r)) if (*t) (void)hipFree(*t);
    if (r->stream) (void)hipStreamDestroy(r->stream);
    delete r;
}

// GMUPT_TRAVERSAL selects a rung of the traversal ladder; all rungs give identical results, the default is the fastest
static int parse_traversal_mode(const char* tv)
{
    constexpr int kDefault = 70;                                            // wide: both ray casts in one launch over the 4-wide collapse of the tree (cast0, the binary fused kernel, takes what it does not)
    if (!tv || !*tv) return kDefault;
    if (std::strcmp(tv, "whilewhile") == 0) return 0;
    if (std::strcmp(tv, "ref") == 0) return 1;
    if (std::strcmp(tv, "static") == 0) return 2;
    if (std::strncmp(tv, "ifif", 4) == 0) return 3 + std::atoi(tv + 4);
    if (std::strcmp(tv, "coop") == 0) return 20;
    if (std::strcmp(tv, "top") == 0) return 30;
    if (std::strncmp(tv, "def", 3) == 0) return 40 + std::atoi(tv + 3);     // separate deferred-leaf launches
    if (std::strncmp(tv, "pipe", 4) == 0) return 50 + std::atoi(tv + 4);    // three-slot lane pipeline
    if (std::strncmp(tv, "cast", 4) == 0) return 60 + std::atoi(tv + 4);    // cast0 mixed lanes + fused fetches, cast1 extension then shadow per wave, cast2 mixed lanes
    if (std::strcmp(tv, "wide") == 0) return 70;                            // both ray casts in one launch over the 4-wide collapse of the tree (pt_traverse_wide.hip)
    return kDefault;
}

extern "C" int gmupt_renderer_create(gmupt_device* dev, const gmupt_renderer_desc* desc, gmupt_renderer** out)
{
    if (!dev || !desc || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_create: null argument");
    *out = nullptr;
    if (desc->width == 0 || desc->height == 0) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_create: empty accumulation target %ux%u", desc->width, desc->height);
    gmupt_renderer* r = new (std::nothrow) gmupt_renderer();
    if (!r) return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_renderer_create: out of host memory");
    r->dev = dev; r->desc = *desc;
    r->travMode = parse_traversal_mode(std::getenv("GMUPT_TRAVERSAL"));
    if (!traversal_mode_available(r->travMode)) {
        delete r;
        return fail(GMUPT_ERR_UNSUPPORTED, "gmupt_renderer_create: GMUPT_TRAVERSAL=%s is not part of this build (wide, cast0 and def0 are; the other rungs need -DGMUPT_VARIANTS)", std::getenv("GMUPT_TRAVERSAL"));
    }
    if (r->desc.pool_paths == 0) r->desc.pool_paths = GMUPT_PATHCOUNT;
    if (r->desc.live_paths == 0 || r->desc.live_paths > r->desc.pool_paths) r->desc.live_paths = r->desc.pool_paths;
    const uint32_t P = r->desc.pool_paths, L = r->desc.live_paths;
    if ((uint64_t)P * F_COUNT * 4ull > (200ull << 30)) { delete r; return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_create: pool of %u paths is too large", P); }

    hipError_t e = hipSetDevice(dev->id);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete r; return fail(GMUPT_ERR_HIP, "gmupt_renderer_create: %s", hipGetErrorString(e)); }

    RenderParams& p = r->p;
    p.P = P; p.L = L;
    p.nBlocks = (L + kBlock - 1) / kBlock;
    p.tileEnabled = desc->tile_enabled; p.tileX0 = desc->tile_x0; p.tileY0 = desc->tile_y0;
    p.budget = desc->path_budget; p.maxDepth = desc->max_depth;
    const uint32_t tb = traversal_block_threads();
    r->travBlocks = (L + tb - 1) / tb;
    p.ovfStride = r->travBlocks * tb;
    if (p.ovfStride < deferred_block_threads()) p.ovfStride = deferred_block_threads();
    { const char* rw = std::getenv("GMUPT_RAYS_PER_WAVE"); p.raysPerWave = rw ? (uint32_t)std::atoi(rw) : 128u; if (p.raysPerWave < 64) p.raysPerWave = 64; if (r->travMode >= 60 && p.raysPerWave > 128) p.raysPerWave = 128; /* the fused kernel keeps a chunk in two registers per lane */ }
    { const char* wpc = std::getenv("GMUPT_WAVES_PER_CU"); const uint32_t w = wpc ? (uint32_t)std::atoi(wpc) : 16u; const uint32_t db = deferred_block_threads(); p.travGridBlocks = (uint32_t)dev->prop.multiProcessorCount * ((w * 64 + db - 1) / db); if (p.travGridBlocks * db > p.ovfStride) p.travGridBlocks = p.ovfStride / db; if (p.travGridBlocks == 0) p.travGridBlocks = 1; }
    { const char* ep = std::getenv("GMUPT_EXTEND_PRUNE"); p.extendPrune = ep ? (uint32_t)std::atoi(ep) : 0u; }
    { const char* sp = std::getenv("GMUPT_SHADOW_PRUNE"); p.shadowPrune = sp ? (uint32_t)std::atoi(sp) : 0u; }
    { const char* ws = std::getenv("GMUPT_WIDE_STEPS"); p.tuneWideSteps = ws ? (uint32_t)std::atoi(ws) : 0u; }
    { const char* xb = std::getenv("GMUPT_XCD_BINS"); p.xcdBins = xb ? (uint32_t)std::atoi(xb) : 0u; }
    { const char* lc = std::getenv("GMUPT_CAST_LOOP_CAP"); p.castLoopCap = lc ? (uint32_t)std::atoi(lc) : (1u << 20); if (p.castLoopCap == 0) p.castLoopCap = 1u << 20; }
    { const char* e1 = std::getenv("GMUPT_REFILL"); p.tuneRefill = e1 ? (uint32_t)std::atoi(e1) : 20u; const char* e2 = std::getenv("GMUPT_TRI_THRESH"); p.tuneTriThresh = e2 ? (uint32_t)std::atoi(e2) : ((r->travMode == 60 || r->travMode == 63 || r->travMode == 70) ? 24u : 32u); } // fused fetches make a burst cheaper

    int rc = GMUPT_OK;
    // Renderer::createBuffers creates the UAV buffers without initial data: D3D11 zero-initialises them
    // the fields of the path state 17 x 256 bytes further apart than the pool size: with P a power of two, the ~50 streams a stage reads and
    // writes would otherwise all be at the same point of the HBM channel rotation (k_logic / k_material: -2 to -3 % on config 3)
    { const char* pad = std::getenv("GMUPT_STATE_PAD"); p.PS = P + (pad ? (uint32_t)std::atoi(pad) & ~63u : 1088u); }
    if (rc == GMUPT_OK) rc = dev_alloc(r, (void**)&p.state, (size_t)F_COUNT * p.PS * 4, 0);
    if (rc == GMUPT_OK) rc = dev_alloc(r, (void**)&p.cls, (size_t)P, CLS_ENDED);
    if (rc == GMUPT_OK) rc = dev_alloc(r, (void**)&p.listNext, (size_t)P * 4, 0xFF);
    if (rc == GMUPT_OK) rc = dev_alloc(r, (void**)&p.sample, (size_t)P * 12, 0);
    if (rc == GMUPT_OK) rc = dev_alloc(r, (void**)&p.blockCounts, (size_t)p.nBlocks * 4 * kNumCounts, 0);
    p.nGroups = (p.nBlocks + kScanGroup - 1) / kScanGroup; p.groupParity = 0;
    if (rc == GMUPT_OK) rc = dev_alloc(r, (void**)&p.groupTotals, (size_t)2 * kNumCounts * p.nGroups * 4, 0);
    if (rc == GMUPT_OK) rc = dev_alloc(r, (void**)&p.queues, (size_t)P * 20, 0);
    if (rc == GMUPT_OK) rc = dev_alloc(r, (void**)&p.qc, 32, 0);
    if (rc == GMUPT_OK) rc = dev_alloc(r, (void**)&p.stats, sizeof(DevStats), 0);
    if (rc == GMUPT_OK) rc = dev_alloc(r, (void**)&p.travCounters, 128, 0);
    if (rc == GMUPT_OK) rc = dev_alloc(r, (void**)&p.ovfStack, (size_t)p.ovfStride * traversal_overflow_entries() * 4, 0);
    if (rc == GMUPT_OK) rc = alloc_framebuffer(r, desc->width, desc->height);
    if (rc == GMUPT_OK) {
        DevStats init{}; init.activePaths = L;
        e = hipMemcpyAsync(p.stats, &init, sizeof(init), hipMemcpyHostToDevice, r->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
        if (e != hipSuccess) rc = fail(GMUPT_ERR_HIP, "gmupt_renderer_create: %s", hipGetErrorString(e));
    }
    if (rc != GMUPT_OK) { std::string keep = g_lastError; gmupt_renderer_destroy(r); g_lastError = keep; return rc; }
    *out = r;
    return GMUPT_OK;
}

// GMUPT_TOP_ORDER=bfs and GMUPT_NODE_PAIRING=0 are A/B switches of the numbering (pt_travtables.cpp); results do not depend on them
static TravOptions trav_options(bool wantWide)
{
    const char* order = std::getenv("GMUPT_TOP_ORDER");
    const char* pairing = std::getenv("GMUPT_NODE_PAIRING");
    TravOptions o;
    o.wantWide = wantWide; o.topOrderBfs = order && std::strcmp(order, "bfs") == 0; o.nodePairing = !(pairing && std::atoi(pairing) == 0);
    o.topCapacity = traversal_top_capacity; o.wideTopCapacity = traversal_wide_top_capacity();
    return o;
}

// Downloads the bound tree, has pt_travtables.cpp build the traversal tables, uploads them.  Once per bind (and per refit that rebuilds).
static int build_traversal_copy(gmupt_renderer* r, const gmupt_buffer* nodesB, const gmupt_buffer* trisB, const gmupt_buffer* vertsB)
{
    HIP_TRY(hipSetDevice(r->dev->id));
    HIP_TRY(hipStreamSynchronize(r->stream));
    const size_t N = nodesB->elems, R = trisB->elems, V = vertsB->elems;
    std::vector<gmupt_bvh_node> nodes(N);
    std::vector<gmupt_triangle> tris(R ? R : 1);
    std::vector<float> verts(V ? V * 3 : 3);
    HIP_TRY(hipMemcpy(nodes.data(), nodesB->dptr, N * sizeof(gmupt_bvh_node), hipMemcpyDeviceToHost));
    if (R) HIP_TRY(hipMemcpy(tris.data(), trisB->dptr, R * sizeof(gmupt_triangle), hipMemcpyDeviceToHost));
    if (V) HIP_TRY(hipMemcpy(verts.data(), vertsB->dptr, V * 12, hipMemcpyDeviceToHost));

    // nothing of the renderer or on the device is touched before the tables exist
    TravTables tt;
    const std::string err = build_trav_tables(nodes.data(), N, tris.data(), R, verts.data(), V, trav_options(r->travMode == 70), tt);
    if (!err.empty()) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s", err.c_str());

    const bool haveWide = !tt.wide.empty();   // without a wide copy the pairs stay on the host
    const void* recs = nullptr; size_t recBytes = 0;
#ifdef GMUPT_VARIANTS
    recs = tt.recs.data(); recBytes = tt.recs.size() * sizeof(Rec64);
#endif
    const struct { const void* data; size_t bytes; } up[6] = {      // in the order of trav_tables()
        { tt.nodes.data(), tt.nodes.size() * sizeof(Node64) }, { tt.tris.data(), tt.tris.size() * sizeof(Tri48) }, { recs, recBytes },
        { tt.wide.data(), tt.wide.size() * sizeof(WNode) }, { tt.pairs.data(), haveWide ? tt.pairs.size() * sizeof(TriPair) : 0 },
        { tt.pairRef.data(), haveWide ? tt.pairRef.size() * 4 : 0 } };
    const std::array<void**, 6> dst = trav_tables(r);
    for (int k = 0; k < 6; k++) {
        if (*dst[k]) { HIP_TRY(hipFree(*dst[k])); *dst[k] = nullptr; }
        r->travBytes[k] = 0;
        if (!up[k].bytes) continue;
        HIP_TRY(hipMalloc(dst[k], up[k].bytes));
        HIP_TRY(hipMemcpy(*dst[k], up[k].data, up[k].bytes, hipMemcpyHostToDevice));
        r->travBytes[k] = up[k].bytes;
    }
    TravScene& t = r->p.trav;
    t.recs = (const Rec64*)r->travRecs; t.nodes = (const Node64*)r->travNodes; t.tris = (const Tri48*)r->travTris;
    t.wnodes = (const WNode*)r->travWide; t.pairs = (const TriPair*)r->travPairs; t.pairRef = (const uint32_t*)r->travPairRef;
    t.triBase = tt.s.triBase; t.rootDesc = tt.s.rootDesc; t.topCount = tt.s.topCount; t.topCountDeep = tt.s.topCountDeep; t.maxDepth = tt.s.maxDepth;
    for (int k = 0; k < 3; k++) { t.rootMin[k] = tt.s.rootMin[k]; t.rootMax[k] = tt.s.rootMax[k]; }
    t.wideCount = tt.s.wideCount; t.wideTopCount = tt.s.wideTopCount; t.wideStackBound = tt.s.wideStackBound; t.wideRootDesc = 0; t.numPairs = tt.s.numPairs;

    // what a refit needs to rewrite these tables in place (host vectors; the first gmupt_renderer_refit uploads them)
    if (r->rfDev) { HIP_TRY(hipFree(r->rfDev)); r->rfDev = nullptr; }
    r->rfLevelNodes.swap(tt.levelNodes); r->rfLevelOff.swap(tt.levelOff); r->rfNodeMap.swap(tt.nodeMap); r->rfWideMap.swap(tt.wideMap); r->rfOpened.swap(tt.opened);
    r->boundNodes = nodesB; r->boundTris = trisB; r->boundVerts = vertsB;
    r->boundElems[0] = N; r->boundElems[1] = R; r->boundElems[2] = V;
    return GMUPT_OK;
}

static_assert(sizeof(gmupt_refit_info) == 24 && offsetof(gmupt_refit_info, ms) == 16, "gmupt_refit_info layout");

extern "C" int gmupt_renderer_refit(gmupt_renderer* r, gmupt_refit_info* info)
{
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_refit: null renderer");
    if (info) *info = gmupt_refit_info{};
    if (!r->sceneBound) return fail(GMUPT_ERR_NOT_BOUND, "gmupt_renderer_refit: no scene bound");
    if (r->boundNodes->elems != r->boundElems[0] || r->boundTris->elems != r->boundElems[1] || r->boundVerts->elems != r->boundElems[2])
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_refit: the bound buffers hold (%zu, %zu, %zu) nodes / triangle records / vertices, at bind time (%zu, %zu, %zu)",
                    r->boundNodes->elems, r->boundTris->elems, r->boundVerts->elems, r->boundElems[0], r->boundElems[1], r->boundElems[2]);
    HIP_TRY(hipSetDevice(r->dev->id));
    HIP_TRY(hipStreamSynchronize(r->stream));
    // one allocation: 16 words of flags and results, then the maps (each starts at a multiple of 16 bytes)
    const std::vector<uint32_t>* maps[4] = { &r->rfLevelNodes, &r->rfNodeMap, &r->rfWideMap, &r->rfOpened };
    size_t off[4], words = 16;
    for (int k = 0; k < 4; k++) { off[k] = words; words += (maps[k]->size() + 3) & ~(size_t)3; }
    if (!r->rfDev) {
        HIP_TRY(hipMalloc(&r->rfDev, words * 4));
        for (int k = 0; k < 4; k++)
            if (!maps[k]->empty()) HIP_TRY(hipMemcpy((uint32_t*)r->rfDev + off[k], maps[k]->data(), maps[k]->size() * 4, hipMemcpyHostToDevice));
    }
    for (hipEvent_t& e : r->rfEv) if (!e) HIP_TRY(hipEventCreate(&e));
    uint32_t* dev = (uint32_t*)r->rfDev;
    const TravScene& t = r->p.trav;
    RfArgs a{};
    a.nodes = (DNode*)r->boundNodes->dptr; a.tris = (const gmupt_triangle*)r->boundTris->dptr; a.verts = (const float*)r->boundVerts->dptr;
    a.numNodes = (uint32_t)r->boundElems[0]; a.numTris = (uint32_t)r->boundElems[1]; a.numVerts = (uint32_t)r->boundElems[2];
    a.levelNodes = dev + off[0];
    a.ttris = (Tri48*)r->travTris; a.pairs = (TriPair*)r->travPairs; a.pairRef = t.pairRef; a.numPairs = t.numPairs;
    a.tnodes = (Node64*)r->travNodes; a.nodeMap = dev + off[1]; a.numPacked = (uint32_t)r->rfNodeMap.size();
    a.wnodes = (WNode*)r->travWide; a.wideMap = dev + off[2]; a.wideCount = r->travWide ? t.wideCount : 0u;
    a.opened = dev + off[3]; a.numOpened = r->travWide ? (uint32_t)r->rfOpened.size() : 0u;
    a.flags = dev;

    uint32_t back[16] = { 0 };
    HIP_TRY(hipMemsetAsync(dev, 0, 64, r->stream));
    launch_refit_check(a, r->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(back, dev, 4, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (back[0] & kRfFlagBadIndex) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_refit: a triangle record references a vertex outside the vertex buffer (the triangle records changed since bind)");
    if (back[0] & kRfFlagNonFinite) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_refit: a vertex used by a triangle record is not finite; nothing was written");

    uint32_t reason = 0;
#ifdef GMUPT_VARIANTS
    reason = GMUPT_REFIT_VARIANTS_BUILD;
#endif
    HIP_TRY(hipEventRecord(r->rfEv[0], r->stream));
    const uint32_t levels = launch_refit_boxes(a, r->rfLevelOff, r->stream);
    if (!reason) launch_refit_tables(a, r->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(dev + 4, a.nodes, 32, hipMemcpyDeviceToDevice, r->stream));      // the root box next to the flags
    HIP_TRY(hipEventRecord(r->rfEv[1], r->stream));
    HIP_TRY(hipMemcpyAsync(back, dev, 64, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, r->rfEv[0], r->rfEv[1]));
    if (back[1]) reason |= GMUPT_REFIT_FLAT_CHILD;
    const uint32_t openedNodes = a.numOpened;
    if (reason) {
        int rc = build_traversal_copy(r, r->boundNodes, r->boundTris, r->boundVerts);
        if (rc != GMUPT_OK) return rc;
    } else {
        for (int k = 0; k < 3; k++) { std::memcpy(&r->p.trav.rootMin[k], &back[4 + k], 4); std::memcpy(&r->p.trav.rootMax[k], &back[8 + k], 4); }
    }
    r->geomGeneration++;
    if (info) { info->rebuilt = reason ? 1u : 0u; info->reason = reason; info->levels = levels; info->opened_nodes = openedNodes; info->ms = (double)ms; }
    return GMUPT_OK;
}

extern "C" int gmupt_bvh_refit_host(gmupt_bvh_node* nodes, uint32_t num_nodes, const gmupt_triangle* tris, uint32_t num_tris,
                                    const float* verts, uint32_t num_verts, uint32_t threads)
{
    if (!nodes || num_nodes == 0 || (!tris && num_tris) || (!verts && num_verts)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_bvh_refit_host: null or empty array");
    const std::string err = validate_tree("gmupt_bvh_refit_host", nodes, num_nodes, tris, num_tris, num_verts, 0);
    if (!err.empty()) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s", err.c_str());
    refit_host(nodes, num_nodes, tris, verts, (int)std::min(std::max(threads, 1u), 16u));
    return GMUPT_OK;
}

struct gmupt_travtables { TravTables t; };

extern "C" int gmupt_debug_travtables_build(const gmupt_bvh_node* nodes, uint32_t num_nodes, const gmupt_triangle* tris, uint32_t num_tris,
                                            const float* verts, uint32_t num_verts, int want_wide, int top_order_bfs, int node_pairing, gmupt_travtables** out)
{
    if (!out || !nodes || num_nodes == 0 || (!tris && num_tris) || (!verts && num_verts)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_travtables_build: null or empty array");
    *out = nullptr;
    TravOptions o;
    o.wantWide = want_wide != 0; o.topOrderBfs = top_order_bfs != 0; o.nodePairing = node_pairing != 0;
    o.topCapacity = traversal_top_capacity; o.wideTopCapacity = traversal_wide_top_capacity();
    gmupt_travtables* h = new (std::nothrow) gmupt_travtables();
    if (!h) return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_debug_travtables_build: out of host memory");
    const std::string err = build_trav_tables(nodes, num_nodes, tris, num_tris, verts, num_verts, o, h->t);
    if (!err.empty()) { delete h; return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s", err.c_str()); }
    *out = h;
    return GMUPT_OK;
}

extern "C" const void* gmupt_debug_travtables_data(const gmupt_travtables* h, int which, size_t* bytes)
{
    if (!h || !bytes) return nullptr;
    const TravTables& t = h->t;
    auto of = [&](const auto& v) -> const void* { *bytes = v.size() * sizeof(v[0]); return v.data(); };
    switch (which) {
    case GMUPT_TT_NODE64: return of(t.nodes); case GMUPT_TT_TRI48: return of(t.tris); case GMUPT_TT_TRIPAIR: return of(t.pairs);
    case GMUPT_TT_PAIRREF: return of(t.pairRef); case GMUPT_TT_WNODE: return of(t.wide);
#ifdef GMUPT_VARIANTS
    case GMUPT_TT_REC64: return of(t.recs);
#endif
    case GMUPT_TT_SCALARS: *bytes = sizeof(TravScalars); return &t.s;
    case GMUPT_TT_LEVEL_NODES: return of(t.levelNodes); case GMUPT_TT_LEVEL_OFF: return of(t.levelOff); case GMUPT_TT_NODE_MAP: return of(t.nodeMap);
    case GMUPT_TT_WIDE_MAP: return of(t.wideMap); case GMUPT_TT_OPENED: return of(t.opened);
    }
    *bytes = 0;
    return nullptr;
}

extern "C" void gmupt_debug_travtables_destroy(gmupt_travtables* h) { delete h; }

// What the renderer holds of the tables above: the device tables as bind uploaded and refit rewrote them, the scalars of its TravScene,
// the refit maps it keeps on the host.  Reads only.
extern "C" int gmupt_debug_read_travtable(gmupt_renderer* r, int which, void* dst, size_t bytes, size_t* needed)
{
    if (!r || !needed) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_read_travtable: null argument");
    *needed = 0;
    if (!r->sceneBound) return fail(GMUPT_ERR_NOT_BOUND, "gmupt_debug_read_travtable: no scene bound");
    HIP_TRY(hipSetDevice(r->dev->id));
    HIP_TRY(hipStreamSynchronize(r->stream));
    const TravScene& t = r->p.trav;
    TravScalars s{};
    s.topCount = t.topCount; s.topCountDeep = t.topCountDeep; s.maxDepth = t.maxDepth; s.rootDesc = t.rootDesc;
    for (int k = 0; k < 3; k++) { s.rootMin[k] = t.rootMin[k]; s.rootMax[k] = t.rootMax[k]; }
    s.triBase = t.triBase; s.wideTopCount = t.wideTopCount; s.wideStackBound = t.wideStackBound; s.numPairs = t.numPairs; s.wideCount = t.wideCount;
    const void* src = nullptr; size_t need = 0; bool onDevice = false;
    auto table = [&](int k) { src = *trav_tables(r)[(size_t)k]; need = src ? r->travBytes[k] : 0; onDevice = true; };      // k: the order of trav_tables()
    auto map = [&](const std::vector<uint32_t>& v) { src = v.data(); need = v.size() * 4; };
    switch (which) {
    case GMUPT_TT_NODE64: table(0); break; case GMUPT_TT_TRI48: table(1); break; case GMUPT_TT_REC64: table(2); break;
    case GMUPT_TT_WNODE: table(3); break; case GMUPT_TT_TRIPAIR: table(4); break; case GMUPT_TT_PAIRREF: table(5); break;
    case GMUPT_TT_SCALARS: src = &s; need = sizeof(s); break;
    case GMUPT_TT_LEVEL_NODES: map(r->rfLevelNodes); break; case GMUPT_TT_LEVEL_OFF: map(r->rfLevelOff); break;
    case GMUPT_TT_NODE_MAP: map(r->rfNodeMap); break; case GMUPT_TT_WIDE_MAP: map(r->rfWideMap); break; case GMUPT_TT_OPENED: map(r->rfOpened); break;
    default: return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_read_travtable: %d is no gmupt_travtable_kind", which);
    }
    *needed = need;
    if (!dst && bytes == 0) return GMUPT_OK;                         // the size query
    if (!dst || bytes < need) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_read_travtable: %zu bytes given, %zu needed", bytes, need);
    if (!need) return GMUPT_OK;
    if (onDevice) HIP_TRY(hipMemcpy(dst, src, need, hipMemcpyDeviceToHost));
    else std::memcpy(dst, src, need);
    return GMUPT_OK;
}

extern "C" int gmupt_debug_wide_tables_addressable(uint32_t wide_nodes, uint32_t num_tris, uint32_t num_pairs)
{
    return wide_tables_addressable(wide_nodes, num_tris, num_pairs) ? 1 : 0;
}

extern "C" int gmupt_renderer_bind_scene(gmupt_renderer* r, const gmupt_buffer* nodes, const gmupt_buffer* triangles, const gmupt_buffer* vertices,
                                         const gmupt_buffer* lights, const gmupt_buffer* tri_props, const gmupt_buffer* materials)
{
    if (!r || !nodes || !triangles || !vertices || !lights || !tri_props || !materials) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_bind_scene: null argument");
    if (nodes->kind != GMUPT_BUFFER_BVH_NODES || triangles->kind != GMUPT_BUFFER_TRIANGLES || vertices->kind != GMUPT_BUFFER_VERTICES ||
        lights->kind != GMUPT_BUFFER_LIGHTS || tri_props->kind != GMUPT_BUFFER_TRI_PROPS || materials->kind != GMUPT_BUFFER_MATERIALS)
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_bind_scene: buffer bound to the wrong slot");
    if (nodes->elems == 0) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_bind_scene: empty BVH");
    if (tri_props->elems < vertices->elems) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_bind_scene: %zu vertex properties for %zu vertices", tri_props->elems, vertices->elems);
    SceneView& s = r->p.scene;
    s.nodes = (const DNode*)nodes->dptr; s.tris = (const gmupt_triangle*)triangles->dptr; s.verts = (const float*)vertices->dptr;
    s.lights = (const gmupt_light*)lights->dptr; s.props = (const gmupt_tri_props*)tri_props->dptr; s.materials = (const gmupt_material*)materials->dptr;
    s.numNodes = (uint32_t)nodes->elems; s.numTris = (uint32_t)triangles->elems; s.numVerts = (uint32_t)vertices->elems; s.numMaterials = (uint32_t)materials->elems;
    int rc = build_traversal_copy(r, nodes, triangles, vertices);
    if (rc != GMUPT_OK) return rc;
    r->sceneBound = true;
    r->bindingId++;
    return GMUPT_OK;
}

extern "C" int gmupt_renderer_bind_textures(gmupt_renderer* r, const gmupt_buffer* diffuse, const gmupt_buffer* metallic_roughness, const gmupt_buffer* normals)
{
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_bind_textures: null renderer");
    const gmupt_buffer* t[3] = { diffuse, metallic_roughness, normals };
    for (int k = 0; k < 3; k++) {
        if (t[k] && t[k]->kind != GMUPT_BUFFER_TEXTURE_ARRAY) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_bind_textures: slot %d is not a texture array", k);
        r->p.scene.tex[k] = t[k] ? (const uint8_t*)t[k]->dptr : nullptr;
        r->p.scene.texSize[k] = t[k] ? t[k]->texSize : 0u;
        r->p.scene.texLayers[k] = t[k] ? t[k]->texLayers : 0u;
    }
    return GMUPT_OK;
}

extern "C" int gmupt_set_camera(gmupt_renderer* r, const gmupt_camera_buffer* cam)
{
    if (!r || !cam) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_set_camera: null argument");
    r->p.cam = *cam; // travels to the kernels as a launch argument: the per-frame 112-byte upload of Renderer.cpp:161
    r->cameraSet = true;
    return GMUPT_OK;
}

static int resolve_timing(gmupt_renderer* r)
{
    if (r->evUsed == 0) return GMUPT_OK;
    HIP_TRY(hipStreamSynchronize(r->stream));
    for (size_t k = 0; k < r->evUsed; k++) {
        for (int sidx = 0; sidx < 4; sidx++) {
            if (r->evPool[k].extOnly && sidx != 2) continue;
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, r->evPool[k].e[sidx], r->evPool[k].e[sidx + 1]));
            r->msStage[sidx] += ms;
        }
        r->timedIters++;
    }
    r->evUsed = 0;
    return GMUPT_OK;
}

static int run_iteration(gmupt_renderer* r, bool doShade, bool doExtend, bool doShadow)
{
    if (!r->sceneBound) return fail(GMUPT_ERR_NOT_BOUND, "gmupt_iterate: no scene bound");
    if (!r->cameraSet) return fail(GMUPT_ERR_NOT_BOUND, "gmupt_iterate: no camera set");
    HIP_TRY(hipSetDevice(r->dev->id));
    const RenderParams& p = r->p;
    const int clearFrame = (p.cam.iterationCounter == 0) ? 1 : 0; // logic.hlsl:206
    const bool stats = r->desc.collect_stats != 0;
    StageEvents* ev = nullptr;
    const bool extOnly = r->timing == 2;
    if (r->timing && doShade && doExtend && doShadow) {
        if (r->evUsed == r->evPool.size()) {
            if (r->evPool.size() >= 4096) { int rc = resolve_timing(r); if (rc != GMUPT_OK) return rc; }
            else { StageEvents se; for (auto& e : se.e) HIP_TRY(hipEventCreate(&e)); r->evPool.push_back(se); }
        }
        ev = &r->evPool[r->evUsed++];
        ev->extOnly = extOnly;
        if (!extOnly) HIP_TRY(hipEventRecord(ev->e[0], r->stream));
    }
    if (doShade) {
        r->p.groupParity ^= 1u;    // p is a reference to r->p: the launches of this iteration see the flipped half of the group totals
        if (clearFrame) { launch_clear(p, r->stream); r->accumGeneration++; } else launch_logic(p, r->stream);
        if (ev && !extOnly) HIP_TRY(hipEventRecord(ev->e[1], r->stream));
        launch_material(p, clearFrame, r->stream);  // computes its own queue offsets (no scan launch)
        if (ev) HIP_TRY(hipEventRecord(ev->e[2], r->stream));
    }
    if (!doShade) HIP_TRY(hipMemsetAsync(p.travCounters, 0, 128, r->stream)); // k_material (block 0) zeroes the ray-cast work counters in a full iteration
    if (doExtend && doShadow && traversal_is_fused(r->travMode)) {
        // one launch for both ray casts; its time is reported as the extension stage, the shadow stage as zero
        const uint32_t launched = launch_cast(p, stats, r->travMode, r->stream);
        if (launched) {
            r->castFlags |= launched;
            if (ev) HIP_TRY(hipEventRecord(ev->e[3], r->stream));
            if (ev && !extOnly) HIP_TRY(hipEventRecord(ev->e[4], r->stream));
            HIP_TRY(hipGetLastError());
            return GMUPT_OK;
        }
    }
    if (doExtend) { r->castFlags |= launch_extend(p, r->travBlocks, stats, r->travMode, r->stream); if (ev) HIP_TRY(hipEventRecord(ev->e[3], r->stream)); }
    if (doShadow) { r->castFlags |= launch_shadow(p, r->travBlocks, stats, r->travMode, r->stream); if (ev && !extOnly) HIP_TRY(hipEventRecord(ev->e[4], r->stream)); }
    HIP_TRY(hipGetLastError());
    return GMUPT_OK;
}

// After a stream synchronise: did a ray-cast launch flag its own results as invalid (DevStats::stackOverflow, sticky until gmupt_reset_stats)?
static int check_cast_flags(gmupt_renderer* r, const char* who)
{
    uint32_t flags = 0;
    HIP_TRY(hipMemcpyAsync(&flags, &r->p.stats->stackOverflow, 4, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (flags & 2u) return fail(GMUPT_ERR_CAST_FAULT, "%s: a wave of the ray cast left its loop at the iteration limit (GMUPT_STAT_CAST_ABORTED): the frame is invalid", who);
    if (flags & 1u) return fail(GMUPT_ERR_CAST_FAULT, "%s: a traversal stack overflowed (GMUPT_STAT_STACK_OVERFLOW): the frame is invalid", who);
    return GMUPT_OK;
}

extern "C" int gmupt_iterate(gmupt_renderer* r)
{
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_iterate: null renderer");
    int rc = run_iteration(r, true, true, true);
    if (rc == GMUPT_OK) r->iterations++;
    return rc;
}

extern "C" int gmupt_debug_run_stage(gmupt_renderer* r, gmupt_stage stage)
{
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_run_stage: null renderer");
    switch (stage) {
    case GMUPT_STAGE_SHADE: return run_iteration(r, true, false, false);
    case GMUPT_STAGE_EXTEND: return run_iteration(r, false, true, false);
    case GMUPT_STAGE_SHADOW: return run_iteration(r, false, false, true);
    case GMUPT_STAGE_RAYCASTS: return run_iteration(r, false, true, true);
    }
    return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_run_stage: unknown stage %d", (int)stage);
}

extern "C" int gmupt_synchronize(gmupt_renderer* r)
{
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_synchronize: null renderer");
    HIP_TRY(hipSetDevice(r->dev->id));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return check_cast_flags(r, "gmupt_synchronize");
}

extern "C" int gmupt_resize(gmupt_renderer* r, uint32_t width, uint32_t height)
{
    if (!r || width == 0 || height == 0) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_resize: bad argument");
    HIP_TRY(hipSetDevice(r->dev->id));
    HIP_TRY(hipStreamSynchronize(r->stream));
    // the new target first: a failed allocation leaves the renderer on its old, still valid target
    float4* oldFb = r->p.fb; uint32_t* oldHead = r->p.listHead; const uint32_t oldW = r->p.fbW, oldH = r->p.fbH;
    r->p.fb = nullptr; r->p.listHead = nullptr;
    const int rc = alloc_framebuffer(r, width, height);
    if (rc != GMUPT_OK) {
        if (r->p.fb) (void)hipFree(r->p.fb);
        if (r->p.listHead) (void)hipFree(r->p.listHead);
        r->p.fb = oldFb; r->p.listHead = oldHead; r->p.fbW = oldW; r->p.fbH = oldH;
        return rc;
    }
    HIP_TRY(hipStreamSynchronize(r->stream));
    (void)hipFree(oldFb); (void)hipFree(oldHead);
    r->desc.width = width; r->desc.height = height;
    r->accumGeneration++;
    return GMUPT_OK;
}

extern "C" int gmupt_read_framebuffer(gmupt_renderer* r, float* rgba, size_t bytes)
{
    if (!r || !rgba) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_read_framebuffer: null argument");
    const size_t need = (size_t)r->p.fbW * r->p.fbH * 16;
    if (bytes < need) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_read_framebuffer: %zu bytes given, %zu needed", bytes, need);
    HIP_TRY(hipSetDevice(r->dev->id));
    HIP_TRY(hipMemcpyAsync(rgba, r->p.fb, need, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return check_cast_flags(r, "gmupt_read_framebuffer");
}

extern "C" int gmupt_copy_framebuffer_to_device(gmupt_renderer* r, void* device_dst, size_t bytes)
{
    if (!r || !device_dst) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_copy_framebuffer_to_device: null argument");
    const size_t need = (size_t)r->p.fbW * r->p.fbH * 16;
    if (bytes < need) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_copy_framebuffer_to_device: %zu bytes given, %zu needed", bytes, need);
    HIP_TRY(hipSetDevice(r->dev->id));
    HIP_TRY(hipMemcpyAsync(device_dst, r->p.fb, need, hipMemcpyDeviceToDevice, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return check_cast_flags(r, "gmupt_copy_framebuffer_to_device");
}

extern "C" int gmupt_get_counters(gmupt_renderer* r, uint32_t out[8])
{
    if (!r || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_get_counters: null argument");
    HIP_TRY(hipSetDevice(r->dev->id));
    HIP_TRY(hipMemcpyAsync(out, r->p.qc, 32, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return GMUPT_OK;
}

extern "C" int gmupt_enable_timing(gmupt_renderer* r, int enabled)
{
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_enable_timing: null renderer");
    if (!enabled) { int rc = resolve_timing(r); if (rc != GMUPT_OK) return rc; }
    r->timing = enabled < 0 ? 0 : enabled;
    return GMUPT_OK;
}

extern "C" int gmupt_get_stats(gmupt_renderer* r, gmupt_stats* out)
{
    if (!r || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_get_stats: null argument");
    HIP_TRY(hipSetDevice(r->dev->id));
    int rc = resolve_timing(r);
    if (rc != GMUPT_OK) return rc;
    DevStats ds;
    HIP_TRY(hipMemcpyAsync(&ds, r->p.stats, sizeof(ds), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    std::memset(out, 0, sizeof(*out));
    out->iterations = r->iterations;
    out->paths_generated = ds.pathsGenerated; out->paths_completed = ds.pathsCompleted; out->segments = ds.segments;
    out->active_paths = ds.activePaths; out->flags = ((ds.stackOverflow & 1u) ? GMUPT_STAT_STACK_OVERFLOW : 0u) | ((ds.stackOverflow & 2u) ? GMUPT_STAT_CAST_ABORTED : 0u) | r->castFlags;
    out->ext_rays = ds.extRays; out->ext_inner = ds.extInner; out->ext_leaves = ds.extLeaves; out->ext_tris = ds.extTris;
    out->sh_rays = ds.shRays; out->sh_inner = ds.shInner; out->sh_leaves = ds.shLeaves; out->sh_tris = ds.shTris;
    out->ms_logic = r->msStage[0]; out->ms_material = r->msStage[1];
    out->ms_scan = 0.0;       // no scan launch: the queue ranks are computed inside k_logic (group totals) and k_material (block prefixes)
    out->ms_accumulate = 0.0; // accumulation is fused into the material kernel
    out->ms_extend = r->msStage[2]; out->ms_shadow = r->msStage[3];
    out->timed_iterations = r->timedIters;
    for (int k = 0; k < 32; k++) { out->ext_depth_hist[k] = ds.extDepthHist[k]; out->cast_wave_end_hist[k] = ds.castWaveEndHist[k]; out->ray_inner_hist[k] = ds.rayInnerHist[k]; }
    for (int k = 0; k < 4; k++) out->lane_census[k] = ds.laneCensus[k];
    out->cast_waves = ds.castWaves; out->cast_wave_ticks = ds.castWaveClocks; out->cast_wave_ticks_max = ds.castWaveClocksMax;
    out->cast_drain_ticks = ds.castDrainClocks; out->cast_drain_iters = ds.castDrainIters; out->cast_drain_busy_lanes = ds.castDrainBusyLanes;
    out->ext_top_inner = ds.extTopInner; out->sh_top_inner = ds.shTopInner; out->cast_helper_subtrees = ds.castHelperSubtrees;
    out->cast_nested_helpers = ds.castNestedHelpers; out->cast_redo_rays = ds.castRedoRays; out->wide_nodes = r->p.trav.wideCount; out->wide_top_nodes = r->p.trav.wideTopCount; out->wide_stack_bound = r->p.trav.wideStackBound; out->wide_pairs = r->p.trav.numPairs; out->wide_pair_fetches = ds.widePairFetches; out->wide_box_tests = ds.wideBoxTests; out->wide_iterations = ds.wideIters; out->wide_general_iterations = ds.wideGeneralIters;
    out->ext_wave_inner = ds.extWaveInner; out->ext_wave_tris = ds.extWaveTris; out->sh_wave_inner = ds.shWaveInner; out->sh_wave_tris = ds.shWaveTris;
    if (ds.stackOverflow & 3u) return fail(GMUPT_ERR_CAST_FAULT, "gmupt_get_stats: a ray-cast launch flagged its results as invalid (flags %#x; the statistics are filled in)", out->flags);
    return GMUPT_OK;
}

extern "C" int gmupt_reset_stats(gmupt_renderer* r)
{
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_reset_stats: null renderer");
    HIP_TRY(hipSetDevice(r->dev->id));
    int rc = resolve_timing(r);
    if (rc != GMUPT_OK) return rc;
    DevStats ds;
    HIP_TRY(hipMemcpyAsync(&ds, r->p.stats, sizeof(ds), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    const uint32_t active = ds.activePaths;
    std::memset(&ds, 0, sizeof(ds)); ds.activePaths = active;
    HIP_TRY(hipMemcpyAsync(r->p.stats, &ds, sizeof(ds), hipMemcpyHostToDevice, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    for (double& m : r->msStage) m = 0.0;
    r->timedIters = 0; r->iterations = 0; r->castFlags = 0;
    return GMUPT_OK;
}

// ------------------------------------------------------------------------------------------------ ray queries
static_assert(sizeof(gmupt_ray) == 32 && offsetof(gmupt_ray, tmax) == 12 && offsetof(gmupt_ray, direction) == 16, "gmupt_ray layout");
static_assert(sizeof(gmupt_hit) == 32 && offsetof(gmupt_hit, triangle) == 12 && offsetof(gmupt_hit, light) == 16 && offsetof(gmupt_hit, material) == 20, "gmupt_hit layout");
static_assert(sizeof(gmupt_trace_info) == 24 && offsetof(gmupt_trace_info, redo_rays) == 8 && offsetof(gmupt_trace_info, ms) == 16, "gmupt_trace_info layout");

// the wide collapse and the limits of k_cast_w's 32-bit buffer offsets, the rule launch_cast_wide applies (gmupt_trace_rays, gmupt_render_aovs)
static int query_supported(gmupt_renderer* r, const char* fn)
{
    const RenderParams& p = r->p;
    if (!p.trav.wnodes || p.extendPrune || p.shadowPrune)
        return fail(GMUPT_ERR_UNSUPPORTED, "%s: the bound scene has no wide collapse (it needs GMUPT_TRAVERSAL=wide, no GMUPT_EXTEND_PRUNE / GMUPT_SHADOW_PRUNE, "
                    "and child boxes inside their parents)", fn);
    if (!wide_tables_addressable(p.trav.wideCount, p.scene.numTris, p.trav.numPairs))
        return fail(GMUPT_ERR_UNSUPPORTED, "%s: the wide tables of the bound scene exceed 2 GiB (%u nodes, %u references, %u pairs)", fn, p.trav.wideCount, p.scene.numTris, p.trav.numPairs);
    return GMUPT_OK;
}

// the query's own work counters, statistics and events, on first use
static int query_buffers(gmupt_renderer* r)
{
    HIP_TRY(hipSetDevice(r->dev->id));
    if (!r->queryStats) {
        int rc = dev_alloc(r, (void**)&r->queryCounters, 128, 0);
        if (rc == GMUPT_OK) rc = dev_alloc(r, (void**)&r->queryStats, sizeof(DevStats), 0);
        if (rc != GMUPT_OK) { r->queryStats = nullptr; return rc; }
        for (hipEvent_t& e : r->queryEv) HIP_TRY(hipEventCreate(&e));
    }
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
    const RenderParams& p = r->p;
    int rc = query_supported(r, "gmupt_trace_rays");
    if (rc == GMUPT_OK) rc = query_buffers(r);
    if (rc != GMUPT_OK) return rc;
    const uint32_t launchFlags = GMUPT_STAT_FUSED_CAST | GMUPT_STAT_CAST_WIDE;
    if (n_closest == 0 && n_any == 0) { HIP_TRY(hipStreamSynchronize(r->stream)); if (info) info->flags = launchFlags; return GMUPT_OK; }
    // behind whatever the renderer has queued; the renderer's counters and statistics are left alone
    HIP_TRY(hipMemsetAsync(r->queryCounters, 0, 128, r->stream));
    HIP_TRY(hipMemsetAsync(r->queryStats, 0, sizeof(DevStats), r->stream));
    RenderParams q = p;
    q.travCounters = r->queryCounters; q.stats = r->queryStats;
    HIP_TRY(hipEventRecord(r->queryEv[0], r->stream));
    launch_trace_wide(q, closest, n_closest, hits, any, n_any, occluded, light_count, r->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(r->queryEv[1], r->stream));
    DevStats ds;
    HIP_TRY(hipMemcpyAsync(&ds, r->queryStats, sizeof(ds), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, r->queryEv[0], r->queryEv[1]));
    const uint32_t flags = launchFlags | ((ds.stackOverflow & 1u) ? GMUPT_STAT_STACK_OVERFLOW : 0u) | ((ds.stackOverflow & 2u) ? GMUPT_STAT_CAST_ABORTED : 0u);
    if (info) { info->flags = flags; info->redo_rays = ds.castRedoRays; info->ms = ms; }
    if (ds.stackOverflow & 2u) return fail(GMUPT_ERR_CAST_FAULT, "gmupt_trace_rays: a wave of the ray cast left its loop at the iteration limit (GMUPT_STAT_CAST_ABORTED): the results are invalid");
    if (ds.stackOverflow & 1u) return fail(GMUPT_ERR_CAST_FAULT, "gmupt_trace_rays: a traversal stack overflowed (GMUPT_STAT_STACK_OVERFLOW): the results are invalid");
    return GMUPT_OK;
}

extern "C" int gmupt_camera_pick_ray(const gmupt_camera_buffer* cam, float px, float py, gmupt_ray* out)
{
    if (!cam || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_camera_pick_ray: null argument");
    // newPath.hlsl:36-39 with the jitter at 0: (x + 0) * pixelSize is x * pixelSize for every float x
    const f3 dir = camera_ray_direction(*cam, px, py);
    std::memset(out, 0, sizeof(*out));
    for (int k = 0; k < 3; k++) out->origin[k] = cam->position[k];
    out->direction[0] = dir.x; out->direction[1] = dir.y; out->direction[2] = dir.z;
    out->tmax = std::numeric_limits<float>::max();   // FLT_MAX: the reference's starting distance (structs.h:9)
    return GMUPT_OK;
}

extern "C" int gmupt_pick(gmupt_renderer* r, float px, float py, uint32_t light_count, gmupt_ray* ray_out, gmupt_hit* hit_out)
{
    if (!r || !hit_out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_pick: null argument");
    if (!r->cameraSet) return fail(GMUPT_ERR_NOT_BOUND, "gmupt_pick: no camera set");
    if (!r->sceneBound) return fail(GMUPT_ERR_NOT_BOUND, "gmupt_pick: no scene bound");
    gmupt_ray ray;
    int rc = gmupt_camera_pick_ray(&r->p.cam, px, py, &ray);
    if (rc != GMUPT_OK) return rc;
    HIP_TRY(hipSetDevice(r->dev->id));
    if (!r->pickBuf) { rc = dev_alloc(r, &r->pickBuf, 64, 0); if (rc != GMUPT_OK) { r->pickBuf = nullptr; return rc; } }
    gmupt_ray* dRay = (gmupt_ray*)r->pickBuf;
    gmupt_hit* dHit = (gmupt_hit*)((char*)r->pickBuf + 32);
    HIP_TRY(hipMemcpyAsync(dRay, &ray, sizeof(ray), hipMemcpyHostToDevice, r->stream));
    rc = gmupt_trace_rays(r, dRay, 1, dHit, nullptr, 0, nullptr, light_count, nullptr);
    if (rc != GMUPT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(hit_out, dHit, sizeof(*hit_out), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (ray_out) *ray_out = ray;
    return GMUPT_OK;
}

// ------------------------------------------------------------------------------------------------ AOV buffers
static_assert(sizeof(gmupt_aov) == 64 && offsetof(gmupt_aov, depth) == 12 && offsetof(gmupt_aov, normal) == 16 && offsetof(gmupt_aov, roughness) == 28 &&
              offsetof(gmupt_aov, position) == 32 && offsetof(gmupt_aov, metallic) == 44 && offsetof(gmupt_aov, triangle) == 48 &&
              offsetof(gmupt_aov, material) == 52 && offsetof(gmupt_aov, light) == 56 && offsetof(gmupt_aov, coverage) == 60, "gmupt_aov layout");

extern "C" int gmupt_aov_ray(const gmupt_camera_buffer* cam, uint32_t x, uint32_t y, uint32_t samples, uint32_t k, gmupt_ray* out)
{
    if (!cam || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_aov_ray: null argument");
    if (samples < 1 || samples > GMUPT_AOV_MAX_SAMPLES) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_aov_ray: samples = %u (1..%d)", samples, GMUPT_AOV_MAX_SAMPLES);
    const uint32_t R = samples == 1 ? 1u : samples * samples + 1u;
    if (k >= R) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_aov_ray: ray %u of %u", k, R);
    float px, py;
    aov_ray_coords(x, y, samples, k, px, py);
    return gmupt_camera_pick_ray(cam, px, py, out);
}

// gmupt_render_aovs, and with motion != nullptr gmupt_render_aovs_motion: k_mv_resolve follows k_aov_resolve on every chunk's hits
static int render_aovs(gmupt_renderer* r, uint32_t samples, gmupt_aov* out, size_t bytes, gmupt_trace_info* info, const float* prevVerts, gmupt_motion* motion);

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

static int render_aovs(gmupt_renderer* r, uint32_t samples, gmupt_aov* out, size_t bytes, gmupt_trace_info* info, const float* prevVerts, gmupt_motion* motion)
{
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_render_aovs: null renderer");
    if (!r->sceneBound) return fail(GMUPT_ERR_NOT_BOUND, "gmupt_render_aovs: no scene bound");
    if (!r->cameraSet) return fail(GMUPT_ERR_NOT_BOUND, "gmupt_render_aovs: no camera set");
    if (!out || ((uintptr_t)out & 15u)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_render_aovs: null or misaligned output (16 bytes)");
    if (samples < 1 || samples > GMUPT_AOV_MAX_SAMPLES) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_render_aovs: samples = %u (1..%d)", samples, GMUPT_AOV_MAX_SAMPLES);
    const uint32_t W = r->p.fbW, H = r->p.fbH;
    if (bytes < (size_t)W * H * sizeof(gmupt_aov)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_render_aovs: %zu bytes for %ux%u records of 64 bytes", bytes, W, H);
    const uint32_t R = samples == 1 ? 1u : samples * samples + 1u;
    if ((uint64_t)W * R > GMUPT_AOV_CHUNK_RAYS) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_render_aovs: one row of %u pixels is %u rays at samples = %u (at most 2^21)", W, W * R, samples);
    int rc = query_supported(r, "gmupt_render_aovs");
    if (rc == GMUPT_OK) rc = query_buffers(r);
    if (rc != GMUPT_OK) return rc;
    if (!r->aovRays) {
        rc = dev_alloc(r, (void**)&r->aovRays, (size_t)GMUPT_AOV_CHUNK_RAYS * sizeof(gmupt_ray), 0);
        if (rc == GMUPT_OK) rc = dev_alloc(r, (void**)&r->aovHits, (size_t)GMUPT_AOV_CHUNK_RAYS * sizeof(gmupt_hit), 0);
        if (rc != GMUPT_OK) { r->aovRays = nullptr; r->aovHits = nullptr; return rc; }
    }
    const RenderParams& p = r->p;
    const uint32_t x0 = p.tileEnabled ? p.tileX0 : 0u, y0 = p.tileEnabled ? p.tileY0 : 0u;
    const uint32_t rowsPerChunk = GMUPT_AOV_CHUNK_RAYS / (W * R);
    // behind whatever the renderer has queued; the renderer's counters and statistics are left alone (the query's are used)
    HIP_TRY(hipMemsetAsync(r->queryStats, 0, sizeof(DevStats), r->stream));
    RenderParams q = p;
    q.travCounters = r->queryCounters; q.stats = r->queryStats;
    HIP_TRY(hipEventRecord(r->queryEv[0], r->stream));
    for (uint32_t row = 0; row < H; row += rowsPerChunk) {
        const uint32_t rows = std::min(rowsPerChunk, H - row), n = rows * W * R;
        launch_aov_raygen(p.cam, x0, y0 + row, W, rows, samples, R, r->aovRays, r->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(r->queryCounters, 0, 128, r->stream));
        launch_trace_wide(q, r->aovRays, n, r->aovHits, nullptr, 0, nullptr, p.cam.lightCount, r->stream);
        HIP_TRY(hipGetLastError());
        launch_aov_resolve(p, rows * W, samples, R, r->aovRays, r->aovHits, out + (size_t)row * W, r->stream);
        HIP_TRY(hipGetLastError());
        if (motion) {
            launch_mv_resolve(p.scene, prevVerts, rows * W, R, r->aovHits, out + (size_t)row * W, motion + (size_t)row * W, r->stream);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipEventRecord(r->queryEv[1], r->stream));
    DevStats ds;
    HIP_TRY(hipMemcpyAsync(&ds, r->queryStats, sizeof(ds), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, r->queryEv[0], r->queryEv[1]));
    const uint32_t flags = GMUPT_STAT_FUSED_CAST | GMUPT_STAT_CAST_WIDE | ((ds.stackOverflow & 1u) ? GMUPT_STAT_STACK_OVERFLOW : 0u) | ((ds.stackOverflow & 2u) ? GMUPT_STAT_CAST_ABORTED : 0u);
    if (info) { info->flags = flags; info->redo_rays = ds.castRedoRays; info->ms = ms; }
    if (ds.stackOverflow & 2u) return fail(GMUPT_ERR_CAST_FAULT, "gmupt_render_aovs: a wave of the ray cast left its loop at the iteration limit (GMUPT_STAT_CAST_ABORTED): the records are invalid");
    if (ds.stackOverflow & 1u) return fail(GMUPT_ERR_CAST_FAULT, "gmupt_render_aovs: a traversal stack overflowed (GMUPT_STAT_STACK_OVERFLOW): the records are invalid");
    return GMUPT_OK;
}

// ------------------------------------------------------------------------------------------------ denoiser
static_assert(sizeof(gmupt_denoise_params) == 20 && offsetof(gmupt_denoise_params, sigma_color) == 4 && offsetof(gmupt_denoise_params, sigma_normal) == 8 &&
              offsetof(gmupt_denoise_params, sigma_plane) == 12 && offsetof(gmupt_denoise_params, sigma_albedo) == 16, "gmupt_denoise_params layout");

extern "C" void gmupt_denoise_default_params(gmupt_denoise_params* p)
{
    if (!p) return;
    p->passes = 5; p->sigma_color = 4.0f; p->sigma_normal = 128.0f; p->sigma_plane = 0.02f; p->sigma_albedo = 0.1f;
}

static int denoise_params(const char* fn, const gmupt_denoise_params* p, DnParams& out)
{
    gmupt_denoise_params d;
    if (!p) { gmupt_denoise_default_params(&d); p = &d; }
    if (p->passes < 1 || p->passes > GMUPT_DENOISE_MAX_PASSES) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: passes = %u (1..%d)", fn, p->passes, GMUPT_DENOISE_MAX_PASSES);
    const float s[4] = { p->sigma_color, p->sigma_normal, p->sigma_plane, p->sigma_albedo };
    const char* names[4] = { "sigma_color", "sigma_normal", "sigma_plane", "sigma_albedo" };
    for (int k = 0; k < 4; k++)
        if (!(std::isfinite(s[k]) && s[k] > 0.0f)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: %s = %g (finite and > 0)", fn, names[k], (double)s[k]);
    out.passes = (int)p->passes; out.sigmaColor = s[0]; out.sigmaNormal = s[1]; out.sigmaPlane = s[2]; out.sigmaAlbedo = s[3];
    return GMUPT_OK;
}

// the arguments every denoiser entry checks; device pointers must be 16-byte aligned
static int denoise_args(const char* fn, const void* beauty, const void* aov, uint32_t W, uint32_t H, const gmupt_denoise_params* p, const void* out, size_t bytes,
                        bool device, DnParams& prm)
{
    if (!beauty || !aov || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null beauty, aov or output", fn);
    if (device && (((uintptr_t)beauty | (uintptr_t)aov | (uintptr_t)out) & 15u)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: misaligned pointer (16 bytes)", fn);
    if (W == 0 || H == 0 || W > 65535 || H > 65535 || (uint64_t)W * H > (1ull << 28)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: image of %ux%u (1..65535 each, at most 2^28 pixels)", fn, W, H);
    {   // the last pass reads beauty texels of other pixels while it writes the output: the two ranges must not overlap at all
        const uintptr_t b0 = (uintptr_t)beauty, o0 = (uintptr_t)out, n = (uintptr_t)W * H * 16;
        if (o0 < b0 + n && b0 < o0 + n) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: the output overlaps the beauty image", fn);
    }
    if (bytes < (size_t)W * H * 16) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: %zu output bytes for %ux%u RGBA32F texels", fn, bytes, W, H);
    return denoise_params(fn, p, prm);
}

// device memory of at least `need` bytes in *ptr, kept between calls (the old contents are not kept when it grows)
static int grow_scratch(gmupt_renderer* r, void** ptr, size_t* have, size_t need)
{
    if (*have >= need) return GMUPT_OK;
    if (*ptr) { HIP_TRY(hipStreamSynchronize(r->stream)); HIP_TRY(hipFree(*ptr)); *ptr = nullptr; *have = 0; }
    HIP_TRY(hipMalloc(ptr, need));
    *have = need;
    return GMUPT_OK;
}

extern "C" int gmupt_denoise_image(gmupt_renderer* r, const float* beauty_rgba, const gmupt_aov* aov, uint32_t width, uint32_t height,
                                   const gmupt_denoise_params* p, float* out_rgba, size_t out_bytes, float* ms)
{
    if (ms) *ms = 0.0f;
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_denoise_image: null renderer");
    DnParams prm;
    int rc = denoise_args("gmupt_denoise_image", beauty_rgba, aov, width, height, p, out_rgba, out_bytes, true, prm);
    if (rc != GMUPT_OK) return rc;
    HIP_TRY(hipSetDevice(r->dev->id));
    rc = grow_scratch(r, &r->dnScratch, &r->dnScratchBytes, (size_t)width * height * kDnScratchBytes);
    if (rc != GMUPT_OK) return rc;
    if (!r->dnEv[0]) for (hipEvent_t& e : r->dnEv) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(r->dnEv[0], r->stream));
    launch_denoise(reinterpret_cast<const float4*>(beauty_rgba), reinterpret_cast<const float4*>(aov), (int)width, (int)height, prm, r->dnScratch,
                   reinterpret_cast<float4*>(out_rgba), r->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(r->dnEv[1], r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    float t = 0.0f;
    HIP_TRY(hipEventElapsedTime(&t, r->dnEv[0], r->dnEv[1]));
    if (ms) *ms = t;
    return GMUPT_OK;
}

extern "C" int gmupt_render_denoised(gmupt_renderer* r, uint32_t aov_samples, const gmupt_denoise_params* p, float* out_rgba, size_t bytes, gmupt_trace_info* info)
{
    if (info) std::memset(info, 0, sizeof(*info));
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_render_denoised: null renderer");
    const uint32_t W = r->p.fbW, H = r->p.fbH;
    if (!out_rgba || ((uintptr_t)out_rgba & 15u)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_render_denoised: null or misaligned output (16 bytes)");
    if (bytes < (size_t)W * H * 16) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_render_denoised: %zu output bytes for %ux%u RGBA32F texels", bytes, W, H);
    DnParams prm;
    int rc = denoise_params("gmupt_render_denoised", p, prm);
    if (rc != GMUPT_OK) return rc;
    // what gmupt_render_aovs would refuse, before the scratch is grown for it
    if (!r->sceneBound) return fail(GMUPT_ERR_NOT_BOUND, "gmupt_render_denoised: no scene bound");
    if (!r->cameraSet) return fail(GMUPT_ERR_NOT_BOUND, "gmupt_render_denoised: no camera set");
    if (aov_samples < 1 || aov_samples > GMUPT_AOV_MAX_SAMPLES) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_render_denoised: aov_samples = %u (1..%d)", aov_samples, GMUPT_AOV_MAX_SAMPLES);
    const uint32_t R = aov_samples == 1 ? 1u : aov_samples * aov_samples + 1u;
    if ((uint64_t)W * R > GMUPT_AOV_CHUNK_RAYS) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_render_denoised: one row of %u pixels is %u rays at aov_samples = %u (at most 2^21)", W, W * R, aov_samples);
    rc = query_supported(r, "gmupt_render_denoised");
    if (rc != GMUPT_OK) return rc;
    HIP_TRY(hipSetDevice(r->dev->id));
    rc = grow_scratch(r, &r->dnInput, &r->dnInputBytes, (size_t)W * H * (sizeof(gmupt_aov) + 16));
    if (rc != GMUPT_OK) return rc;
    gmupt_aov* aov = static_cast<gmupt_aov*>(r->dnInput);
    float* beauty = reinterpret_cast<float*>(static_cast<char*>(r->dnInput) + (size_t)W * H * sizeof(gmupt_aov));
    gmupt_trace_info ai;
    rc = gmupt_render_aovs(r, aov_samples, aov, (size_t)W * H * sizeof(gmupt_aov), &ai);
    if (info) *info = ai;
    if (rc != GMUPT_OK) return rc;
    rc = gmupt_copy_framebuffer_to_device(r, beauty, (size_t)W * H * 16);
    if (rc != GMUPT_OK) return rc;
    float ms = 0.0f;
    rc = gmupt_denoise_image(r, beauty, aov, W, H, p, out_rgba, bytes, &ms);
    if (info) info->ms = ai.ms + ms;
    return rc;
}

extern "C" int gmupt_denoise_host(const float* beauty_rgba, const gmupt_aov* aov, uint32_t width, uint32_t height, const gmupt_denoise_params* p,
                                  float* out_rgba, size_t out_bytes, uint32_t threads)
{
    DnParams prm;
    int rc = denoise_args("gmupt_denoise_host", beauty_rgba, aov, width, height, p, out_rgba, out_bytes, false, prm);
    if (rc != GMUPT_OK) return rc;
    try {
        denoise_host(beauty_rgba, aov, (int)width, (int)height, prm, out_rgba, (int)std::min(std::max(threads, 1u), 16u));
    } catch (const std::bad_alloc&) {
        return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_denoise_host: out of host memory for %ux%u pixels", width, height);
    } catch (const std::exception& e) {
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_denoise_host: %s", e.what());
    }
    return GMUPT_OK;
}

// ------------------------------------------------------------------------------------------------ temporal reuse
static_assert(sizeof(gmupt_history) == 48 && offsetof(gmupt_history, count) == 12 && offsetof(gmupt_history, normal) == 16 &&
              offsetof(gmupt_history, material) == 28 && offsetof(gmupt_history, position) == 32 && offsetof(gmupt_history, valid) == 44, "gmupt_history layout");
static_assert(sizeof(gmupt_temporal_params) == 32 && offsetof(gmupt_temporal_params, history_cap) == 20 && offsetof(gmupt_temporal_params, min_normal_cos) == 24 &&
              offsetof(gmupt_temporal_params, plane_dist) == 28, "gmupt_temporal_params layout");

// one record set with the camera and rectangle it was made for
struct TpSlot {
    void* rec = nullptr; size_t bytes = 0;
    bool present = false;
    gmupt_camera_buffer cam{};
    uint32_t x0 = 0, y0 = 0, W = 0, H = 0;
    // the vertex pose the records were written in (gmupt_render_denoised_temporal_motion only): a device copy of the bound vertex buffer
    void* verts = nullptr; size_t vertsBytes = 0;
    bool hasPose = false; uint64_t binding = 0, geomGeneration = 0; uint32_t numVerts = 0;
};
static_assert(sizeof(gmupt_motion) == 16 && offsetof(gmupt_motion, flags) == 12, "gmupt_motion layout");

struct gmupt_temporal {
    gmupt_renderer* r = nullptr;
    TpSlot frozen, last;                        // history of earlier accumulations; the records of the latest call
    void* integrated = nullptr; size_t integratedBytes = 0;   // the integrated image the spatial filter reads (16 bytes per pixel)
    bool seen = false; uint64_t generation = 0; // the renderer's accumulation generation at the last gmupt_render_denoised_temporal
    hipEvent_t ev[2] = { nullptr, nullptr };
};

extern "C" void gmupt_temporal_default_params(gmupt_temporal_params* p)
{
    if (!p) return;
    gmupt_denoise_default_params(&p->spatial);
    p->history_cap = 32.0f; p->min_normal_cos = 0.9f; p->plane_dist = 0.02f;
}

static int temporal_params(const char* fn, const gmupt_temporal_params* p, DnParams& dn, TpParams& tp)
{
    gmupt_temporal_params d;
    if (!p) { gmupt_temporal_default_params(&d); p = &d; }
    int rc = denoise_params(fn, &p->spatial, dn);
    if (rc != GMUPT_OK) return rc;
    if (!(std::isfinite(p->history_cap) && p->history_cap >= 0.0f && p->history_cap <= GMUPT_TEMPORAL_MAX_CAP))
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: history_cap = %g (0..%g)", fn, (double)p->history_cap, (double)GMUPT_TEMPORAL_MAX_CAP);
    if (!(std::isfinite(p->min_normal_cos) && p->min_normal_cos <= 1.0f)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: min_normal_cos = %g (finite, <= 1)", fn, (double)p->min_normal_cos);
    if (!(std::isfinite(p->plane_dist) && p->plane_dist >= 0.0f)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: plane_dist = %g (finite and >= 0)", fn, (double)p->plane_dist);
    tp.cap = p->history_cap; tp.minCos = p->min_normal_cos; tp.planeDist = p->plane_dist;
    return GMUPT_OK;
}

extern "C" int gmupt_temporal_create(gmupt_renderer* r, gmupt_temporal** out)
{
    if (out) *out = nullptr;
    if (!r || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_temporal_create: null argument");
    gmupt_temporal* t = new (std::nothrow) gmupt_temporal();
    if (!t) return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_temporal_create: out of host memory");
    t->r = r;
    *out = t;
    return GMUPT_OK;
}

extern "C" void gmupt_temporal_destroy(gmupt_temporal* t)
{
    if (!t) return;
    (void)hipSetDevice(t->r->dev->id);
    (void)hipStreamSynchronize(t->r->stream);
    for (hipEvent_t e : t->ev) if (e) (void)hipEventDestroy(e);
    for (void* a : { t->frozen.rec, t->last.rec, t->integrated, t->frozen.verts, t->last.verts }) if (a) (void)hipFree(a);
    delete t;
}

extern "C" int gmupt_temporal_reset(gmupt_temporal* t)
{
    if (!t) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_temporal_reset: null handle");
    t->frozen.present = false; t->last.present = false;
    if (t->frozen.verts || t->last.verts) {   // the pose snapshots go with the records
        HIP_TRY(hipSetDevice(t->r->dev->id));
        HIP_TRY(hipStreamSynchronize(t->r->stream));
        for (TpSlot* sl : { &t->frozen, &t->last }) {
            if (sl->verts) HIP_TRY(hipFree(sl->verts));
            sl->verts = nullptr; sl->vertsBytes = 0; sl->hasPose = false;
        }
    }
    return GMUPT_OK;
}

// gmupt_temporal_denoise_image (motion == nullptr: k_tp_integrate) and gmupt_temporal_denoise_image_motion (k_tp_integrate_mv)
static int temporal_denoise(const char* fn, gmupt_temporal* t, const float* beauty_rgba, const gmupt_aov* aov, const gmupt_motion* motion,
                            const gmupt_camera_buffer* cam, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, int new_accumulation,
                            const gmupt_temporal_params* p, float* out_rgba, size_t out_bytes, float* ms)
{
    if (ms) *ms = 0.0f;
    gmupt_temporal_params d;
    if (!p) { gmupt_temporal_default_params(&d); p = &d; }
    DnParams dn; TpParams tp;
    int rc = denoise_args(fn, beauty_rgba, aov, width, height, &p->spatial, out_rgba, out_bytes, true, dn);   // needs no device: checked first
    if (rc == GMUPT_OK) rc = temporal_params(fn, p, dn, tp);
    if (rc != GMUPT_OK) return rc;
    if (!cam) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null camera", fn);
    if (!t) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null handle", fn);
    gmupt_renderer* r = t->r;
    const size_t n = (size_t)width * height;
    HIP_TRY(hipSetDevice(r->dev->id));
    if (new_accumulation) std::swap(t->frozen, t->last);   // the records of the accumulation that ended become the history
    rc = grow_scratch(r, &t->last.rec, &t->last.bytes, n * sizeof(gmupt_history));
    if (rc == GMUPT_OK) rc = grow_scratch(r, &t->integrated, &t->integratedBytes, n * 16);
    if (rc == GMUPT_OK) rc = grow_scratch(r, &r->dnScratch, &r->dnScratchBytes, n * kDnScratchBytes);
    if (rc != GMUPT_OK) { t->last.present = false; return rc; }
    if (!t->ev[0]) for (hipEvent_t& e : t->ev) HIP_TRY(hipEventCreate(&e));
    TpPrev prev{};
    if (t->frozen.present) {
        prev.rec = static_cast<const float4*>(t->frozen.rec);
        prev.x0 = (int)t->frozen.x0; prev.y0 = (int)t->frozen.y0; prev.W = (int)t->frozen.W; prev.H = (int)t->frozen.H;
        prev.cam = tp_camera(t->frozen.cam);
    }
    float4* integrated = static_cast<float4*>(t->integrated);
    t->last.present = false;                                // until its records are written
    t->last.hasPose = false;                                // until gmupt_render_denoised_temporal_motion says which pose they are in
    HIP_TRY(hipEventRecord(t->ev[0], r->stream));
    if (motion)
        launch_temporal_motion(reinterpret_cast<const float4*>(beauty_rgba), reinterpret_cast<const float4*>(aov), reinterpret_cast<const float4*>(motion),
                               (int)width, (int)height, prev, tp, integrated, static_cast<float4*>(t->last.rec), r->stream);
    else
        launch_temporal(reinterpret_cast<const float4*>(beauty_rgba), reinterpret_cast<const float4*>(aov), (int)width, (int)height, prev, tp, integrated,
                        static_cast<float4*>(t->last.rec), r->stream);
    HIP_TRY(hipGetLastError());
    launch_denoise(integrated, reinterpret_cast<const float4*>(aov), (int)width, (int)height, dn, r->dnScratch, reinterpret_cast<float4*>(out_rgba), r->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(t->ev[1], r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    t->last.present = true; t->last.cam = *cam; t->last.x0 = x0; t->last.y0 = y0; t->last.W = width; t->last.H = height;
    float e = 0.0f;
    HIP_TRY(hipEventElapsedTime(&e, t->ev[0], t->ev[1]));
    if (ms) *ms = e;
    return GMUPT_OK;
}

extern "C" int gmupt_temporal_denoise_image(gmupt_temporal* t, const float* beauty_rgba, const gmupt_aov* aov, const gmupt_camera_buffer* cam,
                                            uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, int new_accumulation,
                                            const gmupt_temporal_params* p, float* out_rgba, size_t out_bytes, float* ms)
{
    return temporal_denoise("gmupt_temporal_denoise_image", t, beauty_rgba, aov, nullptr, cam, x0, y0, width, height, new_accumulation, p, out_rgba, out_bytes, ms);
}

extern "C" int gmupt_temporal_denoise_image_motion(gmupt_temporal* t, const float* beauty_rgba, const gmupt_aov* aov, const gmupt_motion* motion,
                                                   const gmupt_camera_buffer* cam, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height,
                                                   int new_accumulation, const gmupt_temporal_params* p, float* out_rgba, size_t out_bytes, float* ms)
{
    const char* fn = "gmupt_temporal_denoise_image_motion";
    if ((uintptr_t)motion & 15u) { if (ms) *ms = 0.0f; return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: misaligned motion plane (16 bytes)", fn); }
    return temporal_denoise(fn, t, beauty_rgba, aov, motion, cam, x0, y0, width, height, new_accumulation, p, out_rgba, out_bytes, ms);
}

// gmupt_render_denoised_temporal, and with `poses` gmupt_render_denoised_temporal_motion: the record sets keep their vertex pose
static int render_denoised_temporal(const char* fn, bool poses, gmupt_renderer* r, gmupt_temporal* t, uint32_t aov_samples, const gmupt_temporal_params* p,
                                    float* out_rgba, size_t bytes, gmupt_trace_info* info);

extern "C" int gmupt_render_denoised_temporal(gmupt_renderer* r, gmupt_temporal* t, uint32_t aov_samples, const gmupt_temporal_params* p,
                                              float* out_rgba, size_t bytes, gmupt_trace_info* info)
{
    return render_denoised_temporal("gmupt_render_denoised_temporal", false, r, t, aov_samples, p, out_rgba, bytes, info);
}

extern "C" int gmupt_render_denoised_temporal_motion(gmupt_renderer* r, gmupt_temporal* t, uint32_t aov_samples, const gmupt_temporal_params* p,
                                                     float* out_rgba, size_t bytes, gmupt_trace_info* info)
{
    return render_denoised_temporal("gmupt_render_denoised_temporal_motion", true, r, t, aov_samples, p, out_rgba, bytes, info);
}

static int render_denoised_temporal(const char* fn, bool poses, gmupt_renderer* r, gmupt_temporal* t, uint32_t aov_samples, const gmupt_temporal_params* p,
                                    float* out_rgba, size_t bytes, gmupt_trace_info* info)
{
    if (info) std::memset(info, 0, sizeof(*info));
    if (!r || !t) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null renderer or handle", fn);
    if (t->r != r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: the handle belongs to another renderer", fn);
    const uint32_t W = r->p.fbW, H = r->p.fbH;
    if (!out_rgba || ((uintptr_t)out_rgba & 15u)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null or misaligned output (16 bytes)", fn);
    if (bytes < (size_t)W * H * 16) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: %zu output bytes for %ux%u RGBA32F texels", fn, bytes, W, H);
    DnParams dn; TpParams tp;
    int rc = temporal_params(fn, p, dn, tp);
    if (rc != GMUPT_OK) return rc;
    // what gmupt_render_aovs would refuse, before the scratch is grown for it
    if (!r->sceneBound) return fail(GMUPT_ERR_NOT_BOUND, "%s: no scene bound", fn);
    if (!r->cameraSet) return fail(GMUPT_ERR_NOT_BOUND, "%s: no camera set", fn);
    if (aov_samples < 1 || aov_samples > GMUPT_AOV_MAX_SAMPLES) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: aov_samples = %u (1..%d)", fn, aov_samples, GMUPT_AOV_MAX_SAMPLES);
    const uint32_t R = aov_samples == 1 ? 1u : aov_samples * aov_samples + 1u;
    if ((uint64_t)W * R > GMUPT_AOV_CHUNK_RAYS) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: one row of %u pixels is %u rays at aov_samples = %u (at most 2^21)", fn, W, W * R, aov_samples);
    rc = query_supported(r, fn);
    if (rc != GMUPT_OK) return rc;
    HIP_TRY(hipSetDevice(r->dev->id));
    const bool fold = !t->seen || t->generation != r->accumGeneration;
    // the record sets as they will be once the fold has swapped them: `fz` is integrated against, `nw` receives this call's records
    TpSlot& fz = fold ? t->last : t->frozen;
    TpSlot& nw = fold ? t->frozen : t->last;
    const uint32_t nv = r->p.scene.numVerts;
    const auto inPose = [&](const TpSlot& sl) { return sl.hasPose && sl.binding == r->bindingId && sl.numVerts == nv; };
    const bool moved = poses && fz.present && inPose(fz) && fz.geomGeneration != r->geomGeneration;
    const size_t npix = (size_t)W * H;
    rc = grow_scratch(r, &r->dnInput, &r->dnInputBytes, npix * (sizeof(gmupt_aov) + 16 + (moved ? sizeof(gmupt_motion) : 0)));
    if (rc != GMUPT_OK) return rc;
    gmupt_aov* aov = static_cast<gmupt_aov*>(r->dnInput);
    float* beauty = reinterpret_cast<float*>(static_cast<char*>(r->dnInput) + npix * sizeof(gmupt_aov));
    gmupt_motion* motion = moved ? reinterpret_cast<gmupt_motion*>(static_cast<char*>(r->dnInput) + npix * (sizeof(gmupt_aov) + 16)) : nullptr;
    gmupt_trace_info ai;
    if (moved) rc = gmupt_render_aovs_motion(r, aov_samples, static_cast<const float*>(fz.verts), nv, aov, npix * sizeof(gmupt_aov), motion, npix * sizeof(gmupt_motion), &ai);
    else rc = gmupt_render_aovs(r, aov_samples, aov, npix * sizeof(gmupt_aov), &ai);
    if (info) *info = ai;
    if (rc != GMUPT_OK) return rc;
    rc = gmupt_copy_framebuffer_to_device(r, beauty, npix * 16);
    if (rc != GMUPT_OK) return rc;
    if (poses && !(inPose(nw) && nw.geomGeneration == r->geomGeneration)) {
        // the pose of the records this call writes: once per refit, into the set that receives them (never the one integrated against).
        // It is written before temporal_denoise() has checked its arguments and folded, so that one synchronisation serves both; the
        // set is marked as having no pose first and gets it back only after that call succeeded, so a refused call leaves a set that
        // is integrated against without a motion plane, never one with a wrong pose.
        nw.hasPose = false;
        rc = grow_scratch(r, &nw.verts, &nw.vertsBytes, (size_t)nv * 12);
        if (rc != GMUPT_OK) return rc;
        HIP_TRY(hipMemcpyAsync(nw.verts, r->p.scene.verts, (size_t)nv * 12, hipMemcpyDeviceToDevice, r->stream));
    }
    const uint32_t x0 = r->p.tileEnabled ? r->p.tileX0 : 0u, y0 = r->p.tileEnabled ? r->p.tileY0 : 0u;
    float ms = 0.0f;
    rc = temporal_denoise(fn, t, beauty, aov, motion, &r->p.cam, x0, y0, W, H, fold ? 1 : 0, p, out_rgba, bytes, &ms);   // synchronises the stream
    if (info) info->ms = ai.ms + ms;
    if (rc != GMUPT_OK) return rc;
    t->seen = true; t->generation = r->accumGeneration;
    if (poses) { t->last.hasPose = true; t->last.binding = r->bindingId; t->last.geomGeneration = r->geomGeneration; t->last.numVerts = nv; }
    return GMUPT_OK;
}

static int temporal_integrate_host(const char* fn, const float* beauty_rgba, const gmupt_aov* aov, const gmupt_motion* motion, uint32_t width, uint32_t height,
                                   const gmupt_history* prev, const gmupt_camera_buffer* prev_cam, uint32_t prev_x0, uint32_t prev_y0,
                                   uint32_t prev_width, uint32_t prev_height, const gmupt_temporal_params* p,
                                   float* out_rgba, gmupt_history* out_history, uint32_t threads)
{
    if (!beauty_rgba || !aov || !out_rgba || !out_history) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null beauty, aov or output", fn);
    if (width == 0 || height == 0 || width > 65535 || height > 65535 || (uint64_t)width * height > (1ull << 28))
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: image of %ux%u (1..65535 each, at most 2^28 pixels)", fn, width, height);
    if (prev) {
        if (!prev_cam) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: a previous record set without its camera", fn);
        if (prev_width == 0 || prev_height == 0 || prev_width > 65535 || prev_height > 65535 || (uint64_t)prev_width * prev_height > (1ull << 28) ||
            prev_x0 > 65535 || prev_y0 > 65535)
            return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: previous rectangle of %ux%u at (%u, %u) (1..65535 each, at most 2^28 pixels)", fn, prev_width, prev_height, prev_x0, prev_y0);
    }
    {   // the outputs may not overlap each other or any input
        const size_t n = (size_t)width * height;
        const uintptr_t o[2] = { (uintptr_t)out_rgba, (uintptr_t)out_history }, on[2] = { n * 16, n * sizeof(gmupt_history) };
        const uintptr_t i[5] = { (uintptr_t)beauty_rgba, (uintptr_t)aov, (uintptr_t)prev, (uintptr_t)motion, (uintptr_t)out_history },
                        in[5] = { n * 16, n * sizeof(gmupt_aov), prev ? (size_t)prev_width * prev_height * sizeof(gmupt_history) : 0,
                                  motion ? n * sizeof(gmupt_motion) : 0, n * sizeof(gmupt_history) };
        for (int a = 0; a < 2; a++)
            for (int b = 0; b < (a == 0 ? 5 : 4); b++)
                if (in[b] && o[a] < i[b] + in[b] && i[b] < o[a] + on[a]) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: an output overlaps another array", fn);
    }
    gmupt_temporal_params d;
    if (!p) { gmupt_temporal_default_params(&d); p = &d; }
    DnParams dn; TpParams tp;
    int rc = temporal_params(fn, p, dn, tp);
    if (rc != GMUPT_OK) return rc;
    try {
        temporal_host(beauty_rgba, aov, motion, (int)width, (int)height, prev, prev_cam, (int)prev_x0, (int)prev_y0, (int)prev_width, (int)prev_height, tp,
                      out_rgba, out_history, (int)std::min(std::max(threads, 1u), 16u));
    } catch (const std::bad_alloc&) {
        return fail(GMUPT_ERR_OUT_OF_MEMORY, "%s: out of host memory for %ux%u pixels", fn, width, height);
    } catch (const std::exception& e) {
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: %s", fn, e.what());
    }
    return GMUPT_OK;
}

extern "C" int gmupt_temporal_integrate_host(const float* beauty_rgba, const gmupt_aov* aov, uint32_t width, uint32_t height,
                                             const gmupt_history* prev, const gmupt_camera_buffer* prev_cam, uint32_t prev_x0, uint32_t prev_y0,
                                             uint32_t prev_width, uint32_t prev_height, const gmupt_temporal_params* p,
                                             float* out_rgba, gmupt_history* out_history, uint32_t threads)
{
    return temporal_integrate_host("gmupt_temporal_integrate_host", beauty_rgba, aov, nullptr, width, height, prev, prev_cam, prev_x0, prev_y0, prev_width,
                                   prev_height, p, out_rgba, out_history, threads);
}

extern "C" int gmupt_temporal_integrate_motion_host(const float* beauty_rgba, const gmupt_aov* aov, const gmupt_motion* motion, uint32_t width, uint32_t height,
                                                    const gmupt_history* prev, const gmupt_camera_buffer* prev_cam, uint32_t prev_x0, uint32_t prev_y0,
                                                    uint32_t prev_width, uint32_t prev_height, const gmupt_temporal_params* p,
                                                    float* out_rgba, gmupt_history* out_history, uint32_t threads)
{
    return temporal_integrate_host("gmupt_temporal_integrate_motion_host", beauty_rgba, aov, motion, width, height, prev, prev_cam, prev_x0, prev_y0, prev_width,
                                   prev_height, p, out_rgba, out_history, threads);
}

extern "C" int gmupt_motion_host(const gmupt_hit* hits, const gmupt_aov* aov, size_t n, const gmupt_triangle* tris, uint32_t num_tris,
                                 const float* verts_now, const float* verts_prev, uint32_t num_verts, gmupt_motion* out)
{
    const char* fn = "gmupt_motion_host";
    if (n == 0) return GMUPT_OK;
    if (!hits || !aov || !out || !tris || !verts_now || !verts_prev) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null array", fn);
    for (size_t i = 0; i < n; i++) {
        gmupt_hit h;
        std::memcpy(&h, (const char*)hits + i * sizeof(h), sizeof(h));
        if (h.triangle < 0 || h.light > 0u) continue;
        if ((uint32_t)h.triangle >= num_tris) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: hit %zu names triangle record %d of %u", fn, i, h.triangle, num_tris);
        gmupt_triangle T;
        std::memcpy(&T, (const char*)tris + (size_t)h.triangle * sizeof(T), sizeof(T));
        for (int k = 0; k < 3; k++)
            if (T.v[k] < 0 || (uint32_t)T.v[k] >= num_verts) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: triangle record %d references vertex %d of %u", fn, h.triangle, T.v[k], num_verts);
    }
    motion_host(hits, aov, n, tris, verts_now, verts_prev, out);
    return GMUPT_OK;
}

struct gmupt_camera { Camera cam; gmupt_camera(uint32_t w, uint32_t h) : cam(w, h) {} };

extern "C" int gmupt_render_budget(gmupt_renderer* r, gmupt_camera* cam, uint32_t max_iterations, uint32_t* iters)
{
    if (!r || !cam) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_render_budget: null argument");
    if (!r->desc.path_budget) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_render_budget: renderer was created without a path_budget");
    HIP_TRY(hipSetDevice(r->dev->id));
    static_assert(offsetof(DevStats, stackOverflow) == offsetof(DevStats, activePaths) + 4, "the drain check reads both words with one copy");
    uint32_t* hostActive = nullptr;   // [0] activePaths, [1] stackOverflow
    HIP_TRY(hipHostMalloc((void**)&hostActive, 8, hipHostMallocDefault));
    hostActive[0] = 1; hostActive[1] = 0;
    uint32_t k = 0;
    int rc = GMUPT_OK;
    // Drain: stop when no slot is active any more -- or kDrainHorizon iterations after the budget ran out.  A healthy path lives at most
    // ~205 iterations (Russian roulette after 200 bounces, logic.hlsl:248-255), but the reference has paths that do not end that way:
    // a throughput that overflowed to inf survives the roulette and becomes inf / inf = NaN (:251-254), a NaN throughput survives
    // `all(throughput <= 0)` (:237), and such a path only ends when its ray happens to hit a light or leave the scene -- in the closed
    // bench room their number halves every ~450 iterations (0.007 % of all paths; their sample is saturate(NaN) = 0).  In the
    // reference's progressive loop they just occupy pool slots; a bounded job must cut them off.
    constexpr uint32_t kDrainHorizon = 512;
    uint32_t drainStart = 0xFFFFFFFFu;
    for (; k < max_iterations; k++) {
        cam->cam.update(0.0f);                       // Renderer::update -> Scene::update -> Camera::update (Renderer.cpp:158)
        rc = gmupt_set_camera(r, cam->cam.getBuffer());
        if (rc == GMUPT_OK) rc = gmupt_iterate(r);   // Renderer::draw
        if (rc != GMUPT_OK) break;
        if ((k & 7u) == 7u) {                        // drain check without stalling every iteration
            hipError_t e = hipMemcpyAsync(hostActive, &r->p.stats->activePaths, 8, hipMemcpyDeviceToHost, r->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
            if (e != hipSuccess) { rc = fail(GMUPT_ERR_HIP, "gmupt_render_budget: %s", hipGetErrorString(e)); break; }
            if (hostActive[1] & 3u) { rc = fail(GMUPT_ERR_CAST_FAULT, "gmupt_render_budget: a ray-cast launch flagged its results as invalid after %u iterations (flags %#x)", k + 1, hostActive[1]); k++; break; }
            if (*hostActive == 0) { k++; break; }
            if (*hostActive < r->p.L && drainStart == 0xFFFFFFFFu) drainStart = k;     // the first slots have retired: the budget is spent
            if (drainStart != 0xFFFFFFFFu && k - drainStart >= kDrainHorizon) { k++; break; }
        }
    }
    (void)hipHostFree(hostActive);
    if (rc == GMUPT_OK) { hipError_t e = hipStreamSynchronize(r->stream); if (e != hipSuccess) rc = fail(GMUPT_ERR_HIP, "gmupt_render_budget: %s", hipGetErrorString(e)); }
    if (rc == GMUPT_OK) rc = check_cast_flags(r, "gmupt_render_budget");
    if (iters) *iters = k;
    return rc;
}

// ------------------------------------------------------------------------------------------------ debug access (reference layout)
namespace {
struct FieldMap { uint32_t refOffset, slotBytes, comps, first; };
// Assets/Shaders/structs.h:19-48 (offset in bytes per path, x PATHCOUNT) -> first SoA component
const FieldMap kFieldMap[] = {
    { 0, 16, 3, F_RAY_OX }, { 16, 16, 3, F_RAY_DX }, { 32, 16, 3, F_MAT_R }, { 48, 8, 2, F_MAT_METALLIC }, { 56, 16, 3, F_NRM_X },
    { 72, 16, 3, F_SP_X }, { 88, 16, 3, F_BARY_X }, { 104, 4, 1, F_HIT_DIST }, { 108, 16, 4, F_TRI_0 }, { 124, 16, 3, F_SH_OX },
    { 140, 16, 3, F_SH_DX }, { 156, 4, 1, F_LIGHT_IDX }, { 160, 4, 1, F_LIGHT_DIST }, { 164, 4, 1, F_IN_SHADOW }, { 168, 16, 3, F_RAD_R },
    { 184, 16, 3, F_THR_R }, { 200, 16, 3, F_LTHR_R }, { 216, 16, 3, F_DL_R }, { 232, 4, 1, F_PATH_LEN }, { 236, 8, 2, F_SCR_X }, { 244, 4, 1, F_IS_EMITTER },
};
}

extern "C" int gmupt_debug_read_path_state(gmupt_renderer* r, void* dst, size_t bytes)
{
    if (!r || !dst) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_read_path_state: null argument");
    const size_t P = r->p.P;
    if (bytes < P * GMUPT_STATE_BYTES) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_read_path_state: %zu bytes given, %zu needed", bytes, P * (size_t)GMUPT_STATE_BYTES);
    HIP_TRY(hipSetDevice(r->dev->id));
    const size_t PS = r->p.PS;
    std::vector<uint32_t> soa((size_t)F_COUNT * PS);
    HIP_TRY(hipMemcpyAsync(soa.data(), r->p.state, soa.size() * 4, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    std::memset(dst, 0, P * GMUPT_STATE_BYTES);
    uint8_t* out = (uint8_t*)dst;
    for (const FieldMap& f : kFieldMap)
        for (size_t i = 0; i < P; i++) {
            uint32_t* o = (uint32_t*)(out + (size_t)f.refOffset * P + (size_t)f.slotBytes * i);
            for (uint32_t c = 0; c < f.comps; c++) o[c] = soa[(size_t)(f.first + c) * PS + i];
        }
    return GMUPT_OK;
}

extern "C" int gmupt_debug_write_path_state(gmupt_renderer* r, const void* src, size_t bytes)
{
    if (!r || !src) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_write_path_state: null argument");
    const size_t P = r->p.P;
    if (bytes < P * GMUPT_STATE_BYTES) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_write_path_state: %zu bytes given, %zu needed", bytes, P * (size_t)GMUPT_STATE_BYTES);
    HIP_TRY(hipSetDevice(r->dev->id));
    const size_t PS = r->p.PS;
    std::vector<uint32_t> soa((size_t)F_COUNT * PS);
    const uint8_t* in = (const uint8_t*)src;
    for (const FieldMap& f : kFieldMap)
        for (size_t i = 0; i < P; i++) {
            const uint32_t* o = (const uint32_t*)(in + (size_t)f.refOffset * P + (size_t)f.slotBytes * i);
            for (uint32_t c = 0; c < f.comps; c++) soa[(size_t)(f.first + c) * PS + i] = o[c];
        }
    HIP_TRY(hipMemcpyAsync(r->p.state, soa.data(), soa.size() * 4, hipMemcpyHostToDevice, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return GMUPT_OK;
}

extern "C" int gmupt_debug_read_queues(gmupt_renderer* r, uint32_t* dst, size_t bytes)
{
    if (!r || !dst) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_read_queues: null argument");
    const size_t need = (size_t)r->p.P * 20;
    if (bytes < need) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_read_queues: %zu bytes given, %zu needed", bytes, need);
    HIP_TRY(hipSetDevice(r->dev->id));
    HIP_TRY(hipMemcpyAsync(dst, r->p.queues, need, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return GMUPT_OK;
}

extern "C" int gmupt_debug_write_queues(gmupt_renderer* r, const uint32_t* src, size_t bytes)
{
    if (!r || !src) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_write_queues: null argument");
    const size_t need = (size_t)r->p.P * 20;
    if (bytes < need) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_write_queues: %zu bytes given, %zu needed", bytes, need);
    HIP_TRY(hipSetDevice(r->dev->id));
    HIP_TRY(hipMemcpyAsync(r->p.queues, src, need, hipMemcpyHostToDevice, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return GMUPT_OK;
}

extern "C" int gmupt_debug_write_counters(gmupt_renderer* r, const uint32_t in[8])
{
    if (!r || !in) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_write_counters: null argument");
    HIP_TRY(hipSetDevice(r->dev->id));
    HIP_TRY(hipMemcpyAsync(r->p.qc, in, 32, hipMemcpyHostToDevice, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return GMUPT_OK;
}

extern "C" int gmupt_debug_write_framebuffer(gmupt_renderer* r, const float* rgba, size_t bytes)
{
    if (!r || !rgba) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_write_framebuffer: null argument");
    const size_t need = (size_t)r->p.fbW * r->p.fbH * 16;
    if (bytes < need) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_write_framebuffer: %zu bytes given, %zu needed", bytes, need);
    HIP_TRY(hipSetDevice(r->dev->id));
    HIP_TRY(hipMemcpyAsync(r->p.fb, rgba, need, hipMemcpyHostToDevice, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return GMUPT_OK;
}

extern "C" int gmupt_debug_detmath(gmupt_device* dev, int fn, const float* x, const float* y, float* out, uint32_t n)
{
    if (!dev || !x || !y || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_detmath: null argument");
    if (n == 0) return GMUPT_OK;
    HIP_TRY(hipSetDevice(dev->id));
    float *dx = nullptr, *dy = nullptr, *dout = nullptr;
    HIP_TRY(hipMalloc((void**)&dx, (size_t)n * 4)); HIP_TRY(hipMalloc((void**)&dy, (size_t)n * 4)); HIP_TRY(hipMalloc((void**)&dout, (size_t)n * 4));
    HIP_TRY(hipMemcpy(dx, x, (size_t)n * 4, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(dy, y, (size_t)n * 4, hipMemcpyHostToDevice));
    launch_detmath(fn, dx, dy, dout, n, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost));
    (void)hipFree(dx); (void)hipFree(dy); (void)hipFree(dout);
    return GMUPT_OK;
}

// ------------------------------------------------------------------------------------------------ LBVH: the GPU builder (pt_lbvh.hip) and its host reference (pt_lbvh.cpp)
static_assert(sizeof(gmupt_lbvh_info) == 48 && offsetof(gmupt_lbvh_info, ms) == 40, "gmupt_lbvh_info layout");

extern "C" void gmupt_lbvh_default_params(gmupt_lbvh_params* p) { if (p) p->max_leaf_size = 4; }

static void lbvh_fill_info(gmupt_lbvh_info* info, const LbResult& res, uint32_t numTris, double ms)
{
    if (!info) return;
    info->num_nodes = res.numNodes; info->num_leaves = res.numLeaves; info->depth = res.depth; info->num_tris = numTris;
    for (int k = 0; k < 3; k++) { info->root_min[k] = res.rootMin[k]; info->root_max[k] = res.rootMax[k]; }
    info->ms = ms;
}

static int lbvh_leaf_size(const char* fn, const gmupt_lbvh_params* params, uint32_t* L)
{
    *L = params ? params->max_leaf_size : 4u;
    if (*L < 1 || *L > kLbMaxLeaf) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: max_leaf_size %u outside 1..%u", fn, *L, kLbMaxLeaf);
    return GMUPT_OK;
}

extern "C" int gmupt_lbvh_build_host(const float* verts, uint32_t num_verts, const int32_t* indices, uint32_t num_tris, const uint32_t* vertex_material,
                                     const gmupt_lbvh_params* params, gmupt_bvh_node* nodes_out, gmupt_triangle* tris_out, int32_t* ref_triangle_out,
                                     gmupt_lbvh_info* info)
{
    if (!verts || !indices || !nodes_out || !tris_out || num_verts == 0 || num_tris == 0) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_lbvh_build_host: null or empty array");
    if (num_tris > kLbMaxTris) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_lbvh_build_host: more than 2^30 triangles");
    uint32_t L;
    int rc = lbvh_leaf_size("gmupt_lbvh_build_host", params, &L);
    if (rc != GMUPT_OK) return rc;
    LbResult res{};
    int status = GMUPT_OK;
    const std::string err = lbvh_build_host(verts, num_verts, indices, num_tris, vertex_material, L, nodes_out, tris_out, ref_triangle_out, res, &status);
    if (status != GMUPT_OK) return fail(status, "gmupt_lbvh_build_host: %s", err.c_str());
    lbvh_fill_info(info, res, num_tris, 0.0);
    return GMUPT_OK;
}

// the builder handle: a stream, two events and the scratch of the largest mesh built so far
struct gmupt_lbvh { gmupt_device* dev; hipStream_t stream = nullptr; hipEvent_t ev[2] = { nullptr, nullptr }; void* scratch = nullptr; uint32_t capTris = 0; size_t sortTemp = 0; };

extern "C" int gmupt_lbvh_create(gmupt_device* dev, gmupt_lbvh** out)
{
    if (!dev || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_lbvh_create: null argument");
    *out = nullptr;
    gmupt_lbvh* h = new (std::nothrow) gmupt_lbvh();
    if (!h) return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_lbvh_create: out of host memory");
    h->dev = dev;
    hipError_t e = hipSetDevice(dev->id);
    if (e == hipSuccess) e = hipStreamCreate(&h->stream);
    for (hipEvent_t& ev : h->ev) if (e == hipSuccess) e = hipEventCreate(&ev);
    if (e != hipSuccess) { gmupt_lbvh_destroy(h); return fail(GMUPT_ERR_HIP, "gmupt_lbvh_create: %s", hipGetErrorString(e)); }
    *out = h;
    return GMUPT_OK;
}

extern "C" void gmupt_lbvh_destroy(gmupt_lbvh* h)
{
    if (!h) return;
    (void)hipSetDevice(h->dev->id);
    if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
    for (hipEvent_t ev : h->ev) if (ev) (void)hipEventDestroy(ev);
    if (h->scratch) (void)hipFree(h->scratch);
    delete h;
}

// a gmupt_buffer of `elems` elements filled from device memory on stream s (the caller synchronises)
static int lbvh_output_buffer(gmupt_device* dev, gmupt_buffer_kind kind, size_t elems, const void* src, hipStream_t s, gmupt_buffer** out)
{
    gmupt_buffer* b = new (std::nothrow) gmupt_buffer();
    if (!b) return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_lbvh_build: out of host memory");
    b->dev = dev; b->kind = kind; b->elems = elems; b->bytes = elems * kind_stride(kind); b->dptr = nullptr;
    hipError_t e = hipMalloc(&b->dptr, b->bytes + 16);       // the slack of gmupt_buffer_create
    if (e == hipSuccess) e = hipMemsetAsync((char*)b->dptr + b->bytes, 0, 16, s);
    if (e == hipSuccess) e = hipMemcpyAsync(b->dptr, src, b->bytes, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) { if (b->dptr) (void)hipFree(b->dptr); delete b; return fail(GMUPT_ERR_HIP, "gmupt_lbvh_build(%zu bytes): %s", elems * kind_stride(kind), hipGetErrorString(e)); }
    *out = b;
    return GMUPT_OK;
}

extern "C" int gmupt_lbvh_build(gmupt_lbvh* h, const gmupt_buffer* vertices, const int32_t* device_indices, uint32_t num_tris, const uint32_t* device_vertex_material,
                                const gmupt_lbvh_params* params, gmupt_buffer** nodes_out, gmupt_buffer** triangles_out, int32_t* device_ref_triangle,
                                gmupt_lbvh_info* info)
{
    if (nodes_out) *nodes_out = nullptr;
    if (triangles_out) *triangles_out = nullptr;
    if (!h || !vertices || !device_indices || !nodes_out || !triangles_out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_lbvh_build: null argument");
    if (vertices->kind != GMUPT_BUFFER_VERTICES || vertices->dev != h->dev) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_lbvh_build: not a vertex buffer of the builder's device");
    if (vertices->elems == 0 || num_tris == 0) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_lbvh_build: empty mesh");
    if (num_tris > kLbMaxTris || vertices->elems > 0x7FFFFFFFu) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_lbvh_build: more than 2^30 triangles or 2^31 - 1 vertices");
    if (((uintptr_t)device_indices | (uintptr_t)device_vertex_material | (uintptr_t)device_ref_triangle) & 3) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_lbvh_build: misaligned pointer");
    uint32_t L;
    int rc = lbvh_leaf_size("gmupt_lbvh_build", params, &L);
    if (rc != GMUPT_OK) return rc;
    HIP_TRY(hipSetDevice(h->dev->id));
    // the sort's temporary storage is asked for per build (a host-only call): a smaller mesh is not assumed to need less than the capacity did.
    // (capTris, sortTemp) is "large enough for every build so far", not "what the capacity needs": a later build may grow either once more
    size_t sortTemp = 0;
    HIP_TRY(lbvh_sort_temp_bytes(num_tris, &sortTemp));
    if (num_tris > h->capTris || sortTemp > h->sortTemp) {
        if (h->scratch) { HIP_TRY(hipStreamSynchronize(h->stream)); HIP_TRY(hipFree(h->scratch)); h->scratch = nullptr; h->capTris = 0; h->sortTemp = 0; }
        const uint32_t cap = std::max(num_tris, h->capTris);
        HIP_TRY(hipMalloc(&h->scratch, lbvh_scratch_layout(cap, sortTemp).total));
        h->capTris = cap; h->sortTemp = sortTemp;
    }
    const LbScratch off = lbvh_scratch_layout(h->capTris, h->sortTemp);     // the parts are placed for the capacity: a smaller mesh uses the front of each

    LbStaging st{};
    HIP_TRY(hipEventRecord(h->ev[0], h->stream));
    HIP_TRY(launch_lbvh(h->scratch, off, h->sortTemp, (const float*)vertices->dptr, (uint32_t)vertices->elems, device_indices, num_tris, device_vertex_material, L, h->stream, st));
    HIP_TRY(hipEventRecord(h->ev[1], h->stream));
    uint32_t back[16] = { 0 };
    HIP_TRY(hipMemcpyAsync(back, st.words, sizeof(back), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (back[0] & kLbFlagBadIndex) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_lbvh_build: a triangle references a vertex outside the vertex buffer (%zu vertices)", vertices->elems);
    if (back[0] & kLbFlagNonFinite) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_lbvh_build: a vertex used by a triangle is not finite");
    LbResult res{};
    res.numNodes = back[1]; res.numLeaves = (back[1] + 1) / 2; res.depth = back[2];
    for (int k = 0; k < 3; k++) { std::memcpy(&res.rootMin[k], &back[4 + k], 4); std::memcpy(&res.rootMax[k], &back[8 + k], 4); }
    if (res.depth > kLbMaxDepth) return fail(GMUPT_ERR_UNSUPPORTED, "gmupt_lbvh_build: the tree is %u levels deep, the traversal stacks hold %u", res.depth, kLbMaxDepth);
    if (res.numNodes == 0 || res.numNodes > 2 * (size_t)num_tris - 1) return fail(GMUPT_ERR_HIP, "gmupt_lbvh_build: the device reported %u nodes for %u triangles", res.numNodes, num_tris);
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));

    gmupt_buffer* nb = nullptr; gmupt_buffer* tb = nullptr;
    rc = lbvh_output_buffer(h->dev, GMUPT_BUFFER_BVH_NODES, res.numNodes, st.nodes, h->stream, &nb);
    if (rc == GMUPT_OK) rc = lbvh_output_buffer(h->dev, GMUPT_BUFFER_TRIANGLES, num_tris, st.tris, h->stream, &tb);
    hipError_t e = hipSuccess;
    if (rc == GMUPT_OK && device_ref_triangle) e = hipMemcpyAsync(device_ref_triangle, st.ref, (size_t)num_tris * 4, hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (rc == GMUPT_OK && e != hipSuccess) rc = fail(GMUPT_ERR_HIP, "gmupt_lbvh_build: %s", hipGetErrorString(e));
    if (rc != GMUPT_OK) { gmupt_buffer_destroy(nb); gmupt_buffer_destroy(tb); return rc; }
    *nodes_out = nb; *triangles_out = tb;
    lbvh_fill_info(info, res, num_tris, (double)ms);
    return GMUPT_OK;
}

// ------------------------------------------------------------------------------------------------ host: SBVH
struct gmupt_sbvh { gmupt::SbvhBuilder* b; };

extern "C" void gmupt_sbvh_default_params(gmupt_sbvh_params* p)
{
    if (!p) return;
    p->split_alpha = 1.0e-5f; p->max_depth = 64; p->max_spatial_depth = 48; p->min_leaf_size = 1; p->max_leaf_size = 0x7FFFFFF;
    p->node_cost = 1.0f; p->tri_cost = 1.0f;
}

extern "C" int gmupt_sbvh_build(const float* vertices, uint32_t num_vertices, const int32_t* indices, uint32_t num_triangles,
                                const gmupt_sbvh_params* params, gmupt_sbvh** out)
{
    if (!out || (!vertices && num_vertices) || (!indices && num_triangles)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_sbvh_build: null argument");
    *out = nullptr;
    gmupt_sbvh_params prm; gmupt_sbvh_default_params(&prm);
    if (params) prm = *params;
    if (prm.max_depth < 1 || prm.max_depth > 64) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_sbvh_build: max_depth %d outside [1, 64]", prm.max_depth);
    try {
        gmupt_sbvh* h = new gmupt_sbvh();
        h->b = new gmupt::SbvhBuilder(vertices, num_vertices, indices, num_triangles, prm);
        h->b->build();
        *out = h;
    } catch (const std::exception& e) {
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_sbvh_build: %s", e.what());
    }
    return GMUPT_OK;
}
extern "C" uint32_t gmupt_sbvh_num_nodes(const gmupt_sbvh* h) { return h ? h->b->numNodes() : 0; }
extern "C" uint32_t gmupt_sbvh_num_references(const gmupt_sbvh* h) { return h ? h->b->numReferences() : 0; }
extern "C" float gmupt_sbvh_sah(const gmupt_sbvh* h) { return h ? h->b->sah() : 0.0f; }
extern "C" uint32_t gmupt_sbvh_depth(const gmupt_sbvh* h) { return h ? h->b->depth() : 0; }
extern "C" int gmupt_sbvh_flatten(const gmupt_sbvh* h, const uint32_t* vertex_material, gmupt_bvh_node* nodes, gmupt_triangle* triangles, int32_t* ref_triangle)
{
    if (!h || !nodes) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_sbvh_flatten: null argument");
    h->b->flatten(vertex_material, nodes, triangles, ref_triangle);
    return GMUPT_OK;
}
extern "C" void gmupt_sbvh_destroy(gmupt_sbvh* h) { if (h) { delete h->b; delete h; } }

// ------------------------------------------------------------------------------------------------ host: camera
extern "C" int gmupt_camera_create(uint32_t width, uint32_t height, gmupt_camera** out)
{
    if (!out || !width || !height) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_camera_create: bad argument");
    *out = new (std::nothrow) gmupt_camera(width, height);
    return *out ? GMUPT_OK : fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_camera_create: out of host memory");
}
extern "C" void gmupt_camera_destroy(gmupt_camera* c) { delete c; }
extern "C" void gmupt_camera_update_resolution(gmupt_camera* c, uint32_t width, uint32_t height) { if (c) c->cam.updateResolution(width, height); }
extern "C" void gmupt_camera_set_pose(gmupt_camera* c, float x, float y, float z, float pitch, float yaw) { if (c) { c->cam.setPosition(x, y, z); c->cam.setRotation(pitch, yaw); } }
extern "C" void gmupt_camera_update(gmupt_camera* c, float dt) { if (c) c->cam.update(dt); }
extern "C" void gmupt_camera_set_input(gmupt_camera* c, float mouse_dx, float mouse_dy, uint32_t keys_wsad)
{
    if (!c) return;
    c->cam.addMouseDelta(mouse_dx, mouse_dy);
    c->cam.setKeys((keys_wsad & 1u) != 0, (keys_wsad & 2u) != 0, (keys_wsad & 4u) != 0, (keys_wsad & 8u) != 0);
}

extern "C" void gmupt_camera_reset_accumulation(gmupt_camera* c) { if (c) c->cam.getBuffer()->iterationCounter = -1; }
extern "C" gmupt_camera_buffer* gmupt_camera_get_buffer(gmupt_camera* c) { return c ? c->cam.getBuffer() : nullptr; }
