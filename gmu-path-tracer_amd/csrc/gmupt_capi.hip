// C-ABI of libgmupt.so (see include/gmupt.h for the contract and the reference call sites each entry replaces).
// Host code only; the kernels live in pt_kernels.hip.
#include "gmupt_internal.hpp"

#include <cstdarg>
#include <cstdio>

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

// ------------------------------------------------------------------------------------------------ errors
thread_local std::string g_lastError;

int fail(int code, const char* fmt, ...)
{
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    g_lastError = buf;
    return code;
}

extern "C" const char* gmupt_last_error(void) { return g_lastError.c_str(); }
extern "C" const char* gmupt_version(void) { return "gmupt 0.1 (gfx950)"; }

// ------------------------------------------------------------------------------------------------ device
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
size_t kind_stride(gmupt_buffer_kind k)
{
    switch (k) {
    case GMUPT_BUFFER_BVH_NODES: return 48; case GMUPT_BUFFER_TRIANGLES: return 16; case GMUPT_BUFFER_VERTICES: return 12;
    case GMUPT_BUFFER_LIGHTS: return 32; case GMUPT_BUFFER_TRI_PROPS: return 32; case GMUPT_BUFFER_MATERIALS: return 48;
    case GMUPT_BUFFER_TEXTURE_ARRAY: return 4;
    }
    return 0;
}

// the handle and the device memory of a new buffer (gmupt_buffer_create, gmupt_lbvh_build): nullptr without host memory, else *e says
// whether the `bytes` bytes exist -- 16 more are allocated: 12-byte vertices are read with in-bounds dword loads only, the slack is for safety
gmupt_buffer* buffer_alloc(gmupt_device* dev, gmupt_buffer_kind kind, size_t elems, size_t bytes, hipError_t* e)
{
    gmupt_buffer* b = new (std::nothrow) gmupt_buffer();
    if (!b) return nullptr;
    b->dev = dev; b->kind = kind; b->bytes = bytes; b->elems = elems; b->dptr = nullptr;
    *e = hipSetDevice(dev->id);
    if (*e == hipSuccess) *e = hipMalloc(&b->dptr, bytes + 16);
    return b;
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
    hipError_t e = hipSuccess;
    gmupt_buffer* b = buffer_alloc(dev, kind, bytes / stride, alloc, &e);
    if (!b) return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_buffer_create: out of host memory");
    if (e == hipSuccess) e = hipMemset(b->dptr, 0, alloc + 16);
    if (e == hipSuccess && bytes) e = hipMemcpy(b->dptr, data, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { gmupt_buffer_destroy(b); return fail(GMUPT_ERR_HIP, "gmupt_buffer_create(%zu bytes): %s", alloc, hipGetErrorString(e)); }
    *out = b;
    return GMUPT_OK;
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
// one buffer of the path-state pool: owned by r->pool, its address in the kernel argument
template <class T> static int pool_alloc(gmupt_renderer* r, T** dst, size_t bytes, int fill)
{
    r->pool.emplace_back();
    GMUPT_TRY(r->pool.back().alloc(bytes, fill, r->stream));
    *dst = r->pool.back().as<T>();
    return GMUPT_OK;
}

// A cleared accumulation target of w x h pixels.  The renderer changes over only when both parts exist: a failure leaves it on what it
// had.  What it had (gmupt_resize) is freed on return: that caller has synchronised the stream, no launch uses it any more.
static int alloc_framebuffer(gmupt_renderer* r, uint32_t w, uint32_t h)
{
    const size_t npix = (size_t)w * h;
    DevMem fb, head;
    GMUPT_TRY(fb.alloc(npix * 16 + 16, 0, r->stream));           // createRenderTexture: no initial data => zero
    GMUPT_TRY(head.alloc(npix * 4 + 16, 0xFF, r->stream));
    r->fb = std::move(fb); r->listHead = std::move(head);
    r->p.fb = r->fb.as<float4>(); r->p.listHead = r->listHead.as<uint32_t>(); r->p.fbW = w; r->p.fbH = h;
    return GMUPT_OK;
}

extern "C" void gmupt_renderer_destroy(gmupt_renderer* r)
{
    if (!r) return;
    (void)hipSetDevice(r->dev->id);
    if (r->stream) (void)hipStreamSynchronize(r->stream);
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

// an unsigned setting from the environment; `fallback` where the variable is not set
static uint32_t env_u32(const char* name, uint32_t fallback) { const char* v = std::getenv(name); return v ? (uint32_t)std::atoi(v) : fallback; }

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
    p.raysPerWave = std::max(env_u32("GMUPT_RAYS_PER_WAVE", 128u), 64u);
    if (r->travMode >= 60 && p.raysPerWave > 128) p.raysPerWave = 128;        // the fused kernel keeps a chunk in two registers per lane
    const uint32_t db = deferred_block_threads();
    p.travGridBlocks = (uint32_t)dev->prop.multiProcessorCount * ((env_u32("GMUPT_WAVES_PER_CU", 16u) * 64 + db - 1) / db);
    p.travGridBlocks = std::max(std::min(p.travGridBlocks, p.ovfStride / db), 1u);   // no more threads than the overflow stacks serve
    p.extendPrune = env_u32("GMUPT_EXTEND_PRUNE", 0u); p.shadowPrune = env_u32("GMUPT_SHADOW_PRUNE", 0u);
    p.tuneWideSteps = env_u32("GMUPT_WIDE_STEPS", 0u);
    p.castLoopCap = env_u32("GMUPT_CAST_LOOP_CAP", 1u << 20);
    if (p.castLoopCap == 0) p.castLoopCap = 1u << 20;
    p.tuneRefill = env_u32("GMUPT_REFILL", 20u);
    p.tuneTriThresh = env_u32("GMUPT_TRI_THRESH", (r->travMode == 60 || r->travMode == 63 || r->travMode == 70) ? 24u : 32u);   // fused fetches make a burst cheaper

    int rc = GMUPT_OK;
    // Renderer::createBuffers creates the UAV buffers without initial data: D3D11 zero-initialises them
    // the fields of the path state 17 x 256 bytes further apart than the pool size: with P a power of two, the ~50 streams a stage reads and
    // writes would otherwise all be at the same point of the HBM channel rotation (k_logic / k_material: -2 to -3 % on config 3)
    p.PS = P + (env_u32("GMUPT_STATE_PAD", 1088u) & ~63u);
    if (rc == GMUPT_OK) rc = pool_alloc(r, &p.state, (size_t)F_COUNT * p.PS * 4, 0);
    if (rc == GMUPT_OK) rc = pool_alloc(r, &p.cls, (size_t)P, CLS_ENDED);
    if (rc == GMUPT_OK) rc = pool_alloc(r, &p.listNext, (size_t)P * 4, 0xFF);
    if (rc == GMUPT_OK) rc = pool_alloc(r, &p.sample, (size_t)P * 12, 0);
    if (rc == GMUPT_OK) rc = pool_alloc(r, &p.blockCounts, (size_t)p.nBlocks * 4 * kNumCounts, 0);
    p.nGroups = (p.nBlocks + kScanGroup - 1) / kScanGroup; p.groupParity = 0;
    if (rc == GMUPT_OK) rc = pool_alloc(r, &p.groupTotals, (size_t)2 * kNumCounts * p.nGroups * 4, 0);
    if (rc == GMUPT_OK) rc = pool_alloc(r, &p.queues, (size_t)P * 20, 0);
    if (rc == GMUPT_OK) rc = pool_alloc(r, &p.qc, 32, 0);
    if (rc == GMUPT_OK) rc = pool_alloc(r, &p.stats, sizeof(DevStats), 0);
    if (rc == GMUPT_OK) rc = pool_alloc(r, &p.travCounters, 128, 0);
    if (rc == GMUPT_OK) rc = pool_alloc(r, &p.ovfStack, (size_t)p.ovfStride * traversal_overflow_entries() * 4, 0);
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
    GMUPT_TRY(build_traversal_copy(r, nodes, triangles, vertices));
    r->boundProps = tri_props;
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
    const gmupt_adaptive* plan = doShade ? r->adaptive : nullptr;   // adaptive sampling: null = the launches below are all there is
    if (plan && (uint64_t)plan->W * plan->H != (uint64_t)r->p.fbW * r->p.fbH)
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_iterate: the attached sampling plan is for %ux%u pixels, the renderer's rectangle is %ux%u", plan->W, plan->H, r->p.fbW, r->p.fbH);
    HIP_TRY(hipSetDevice(r->dev->id));
    const RenderParams& p = r->p;
    const int clearFrame = (p.cam.iterationCounter == 0) ? 1 : 0; // logic.hlsl:206
    const bool stats = r->desc.collect_stats != 0;
    StageEvents* ev = nullptr;
    const bool extOnly = r->timing == 2;
    if (r->timing && doShade && doExtend && doShadow) {
        if (r->evUsed == r->evPool.size()) {
            if (r->evPool.size() >= 4096) GMUPT_TRY(resolve_timing(r));
            else { StageEvents se; GMUPT_TRY(se.create()); r->evPool.push_back(std::move(se)); }
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
        if (plan && plan->count) launch_adaptive_retarget(p, plan->sc.list, plan->count, plan->uniformEvery, r->stream);   // re-aims the fresh camera paths
        if (r->shutterAttached) launch_shutter_retarget(p, r->shutter, r->lens, r->projection, r->stream);   // shutter: in place of the two below, whose rule it runs on the camera at the path's time
        else if (r->lens.aperture_radius > 0.0f) launch_lens_retarget(p, r->lens.aperture_radius, r->lens.focus_distance, r->stream);   // thin lens: after the re-aim, it reads the pixel from the state
        else if (r->projection.kind != GMUPT_PROJ_PINHOLE) launch_proj_retarget(p, r->projection, r->stream);   // camera projection: where the lens would be (the two do not combine)
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
    GMUPT_TRY(copy_sync(&flags, &r->p.stats->stackOverflow, 4, hipMemcpyDeviceToHost, r->stream));
    if (flags & 2u) return fail(GMUPT_ERR_CAST_FAULT, "%s: a wave of the ray cast left its loop at the iteration limit (GMUPT_STAT_CAST_ABORTED): the frame is invalid", who);
    if (flags & 1u) return fail(GMUPT_ERR_CAST_FAULT, "%s: a traversal stack overflowed (GMUPT_STAT_STACK_OVERFLOW): the frame is invalid", who);
    return GMUPT_OK;
}

// fn's copy of `need` bytes between the renderer's memory and the `bytes` its caller has, on the stream and waited for
static int sized_copy(gmupt_renderer* r, const char* fn, void* dst, const void* src, size_t need, size_t bytes, hipMemcpyKind kind)
{
    if (bytes < need) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: %zu bytes given, %zu needed", fn, bytes, need);
    HIP_TRY(hipSetDevice(r->dev->id));
    return copy_sync(dst, src, need, kind, r->stream);
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
    GMUPT_TRY(alloc_framebuffer(r, width, height));   // a failed allocation leaves the renderer on its old, still valid target
    HIP_TRY(hipStreamSynchronize(r->stream));
    r->desc.width = width; r->desc.height = height;
    r->accumGeneration++;
    r->adaptive = nullptr;                            // a sampling plan is a plan for the old rectangle
    r->shutterAttached = false;                       // a close pose is one of the old aspect: its `horizontal` no longer matches the camera's
    return GMUPT_OK;
}

extern "C" int gmupt_read_framebuffer(gmupt_renderer* r, float* rgba, size_t bytes)
{
    if (!r || !rgba) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_read_framebuffer: null argument");
    GMUPT_TRY(sized_copy(r, "gmupt_read_framebuffer", rgba, r->p.fb, (size_t)r->p.fbW * r->p.fbH * 16, bytes, hipMemcpyDeviceToHost));
    return check_cast_flags(r, "gmupt_read_framebuffer");
}

extern "C" int gmupt_copy_framebuffer_to_device(gmupt_renderer* r, void* device_dst, size_t bytes)
{
    if (!r || !device_dst) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_copy_framebuffer_to_device: null argument");
    GMUPT_TRY(sized_copy(r, "gmupt_copy_framebuffer_to_device", device_dst, r->p.fb, (size_t)r->p.fbW * r->p.fbH * 16, bytes, hipMemcpyDeviceToDevice));
    return check_cast_flags(r, "gmupt_copy_framebuffer_to_device");
}

extern "C" int gmupt_get_counters(gmupt_renderer* r, uint32_t out[8])
{
    if (!r || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_get_counters: null argument");
    return sized_copy(r, "gmupt_get_counters", out, r->p.qc, 32, 32, hipMemcpyDeviceToHost);
}

extern "C" int gmupt_enable_timing(gmupt_renderer* r, int enabled)
{
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_enable_timing: null renderer");
    if (!enabled) GMUPT_TRY(resolve_timing(r));
    r->timing = enabled < 0 ? 0 : enabled;
    return GMUPT_OK;
}

extern "C" int gmupt_get_stats(gmupt_renderer* r, gmupt_stats* out)
{
    if (!r || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_get_stats: null argument");
    HIP_TRY(hipSetDevice(r->dev->id));
    GMUPT_TRY(resolve_timing(r));
    DevStats ds;
    GMUPT_TRY(copy_sync(&ds, r->p.stats, sizeof(ds), hipMemcpyDeviceToHost, r->stream));
    std::memset(out, 0, sizeof(*out));
    out->iterations = r->iterations;
    out->paths_generated = ds.pathsGenerated; out->paths_completed = ds.pathsCompleted; out->segments = ds.segments;
    out->active_paths = ds.activePaths; out->flags = cast_fault_flags(ds) | r->castFlags;
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
    GMUPT_TRY(resolve_timing(r));
    DevStats ds;
    GMUPT_TRY(copy_sync(&ds, r->p.stats, sizeof(ds), hipMemcpyDeviceToHost, r->stream));
    const uint32_t active = ds.activePaths;
    std::memset(&ds, 0, sizeof(ds)); ds.activePaths = active;
    GMUPT_TRY(copy_sync(r->p.stats, &ds, sizeof(ds), hipMemcpyHostToDevice, r->stream));
    for (double& m : r->msStage) m = 0.0;
    r->timedIters = 0; r->iterations = 0; r->castFlags = 0;
    return GMUPT_OK;
}

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
    GMUPT_TRY(copy_sync(soa.data(), r->p.state, soa.size() * 4, hipMemcpyDeviceToHost, r->stream));
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
    GMUPT_TRY(copy_sync(r->p.state, soa.data(), soa.size() * 4, hipMemcpyHostToDevice, r->stream));
    return GMUPT_OK;
}

extern "C" int gmupt_debug_read_queues(gmupt_renderer* r, uint32_t* dst, size_t bytes)
{
    if (!r || !dst) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_read_queues: null argument");
    return sized_copy(r, "gmupt_debug_read_queues", dst, r->p.queues, (size_t)r->p.P * 20, bytes, hipMemcpyDeviceToHost);
}

extern "C" int gmupt_debug_write_queues(gmupt_renderer* r, const uint32_t* src, size_t bytes)
{
    if (!r || !src) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_write_queues: null argument");
    return sized_copy(r, "gmupt_debug_write_queues", r->p.queues, src, (size_t)r->p.P * 20, bytes, hipMemcpyHostToDevice);
}

extern "C" int gmupt_debug_write_counters(gmupt_renderer* r, const uint32_t in[8])
{
    if (!r || !in) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_write_counters: null argument");
    return sized_copy(r, "gmupt_debug_write_counters", r->p.qc, in, 32, 32, hipMemcpyHostToDevice);
}

extern "C" int gmupt_debug_write_framebuffer(gmupt_renderer* r, const float* rgba, size_t bytes)
{
    if (!r || !rgba) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_write_framebuffer: null argument");
    return sized_copy(r, "gmupt_debug_write_framebuffer", r->p.fb, rgba, (size_t)r->p.fbW * r->p.fbH * 16, bytes, hipMemcpyHostToDevice);
}

extern "C" int gmupt_debug_detmath(gmupt_device* dev, int fn, const float* x, const float* y, float* out, uint32_t n)
{
    if (!dev || !x || !y || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_detmath: null argument");
    if (n == 0) return GMUPT_OK;
    HIP_TRY(hipSetDevice(dev->id));
    DevMem dx, dy, dout;
    GMUPT_TRY(dx.grow(nullptr, (size_t)n * 4)); GMUPT_TRY(dy.grow(nullptr, (size_t)n * 4)); GMUPT_TRY(dout.grow(nullptr, (size_t)n * 4));
    HIP_TRY(hipMemcpy(dx.ptr, x, (size_t)n * 4, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(dy.ptr, y, (size_t)n * 4, hipMemcpyHostToDevice));
    launch_detmath(fn, dx.as<float>(), dy.as<float>(), dout.as<float>(), n, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout.ptr, (size_t)n * 4, hipMemcpyDeviceToHost));
    return GMUPT_OK;
}
