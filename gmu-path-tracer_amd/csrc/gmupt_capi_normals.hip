// C-ABI of libgmupt.so: smooth vertex normals on the device (gmupt_normals_*, pt_normals.hip) and the device-to-device buffer update that
// lets a pose computed on the GPU reach the vertex buffer.
#include "gmupt_internal.hpp"

static_assert(sizeof(gmupt_normals_info) == 24 && offsetof(gmupt_normals_info, ms) == 16, "gmupt_normals_info layout");

extern "C" int gmupt_buffer_update_device(gmupt_buffer* buf, const void* device_src, size_t bytes)
{
    if (!buf || (!device_src && bytes)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_buffer_update_device: null argument");
    if (bytes > buf->bytes) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_buffer_update_device: %zu bytes into a %zu-byte buffer", bytes, buf->bytes);
    HIP_TRY(hipSetDevice(buf->dev->id));
    if (bytes) {
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, device_src) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != buf->dev->id) {
            (void)hipGetLastError();
            return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_buffer_update_device: the source is not device memory of device %d", buf->dev->id);
        }
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(buf->dptr, device_src, bytes, hipMemcpyDeviceToDevice));
    HIP_TRY(hipDeviceSynchronize());     // a device-to-device copy may return before it has run; the renderer's stream does not wait for the null stream
    return GMUPT_OK;
}

// the kernel argument of a handle; verts / props are filled in by update, the sort's arrays (in `scratch`, create only) by create
static NmArgs normals_args(const gmupt_normals* n, char* scratch = nullptr)
{
    char* base = n->mem.as<char>();
    NmArgs a{};
    a.indices = (const int32_t*)(base + n->off.indices); a.numTris = n->numTris; a.numVerts = n->numVerts;
    a.corners = (uint32_t*)(base + n->off.corners); a.offsets = (uint32_t*)(base + n->off.offsets); a.faces = (float4*)(base + n->off.faces);
    a.words = (uint32_t*)(base + n->off.words);
    if (scratch) {
        a.keysIn = (uint32_t*)(scratch + (n->off.keysIn - n->off.kept)); a.keys = (uint32_t*)(scratch + (n->off.keys - n->off.kept));
        a.valsIn = (uint32_t*)(scratch + (n->off.valsIn - n->off.kept));
    }
    return a;
}

extern "C" int gmupt_normals_create(gmupt_renderer* r, const int32_t* device_indices, uint32_t num_tris, gmupt_normals** out)
{
    if (out) *out = nullptr;
    if (!r || !device_indices || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_normals_create: null argument");
    if (!r->sceneBound) return fail(GMUPT_ERR_NOT_BOUND, "gmupt_normals_create: no scene bound");
    const size_t V = r->boundVerts->elems;
    if (num_tris == 0 || V == 0) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_normals_create: empty mesh");
    if (num_tris > kNmMaxTris || V > 0x7FFFFFFFu) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_normals_create: more than 2^30 triangles or 2^31 - 1 vertices");
    if ((uintptr_t)device_indices & 3) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_normals_create: misaligned pointer");
    HIP_TRY(hipSetDevice(r->dev->id));
    gmupt_normals* n = new (std::nothrow) gmupt_normals();
    if (!n) return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_normals_create: out of host memory");
    n->r = r; n->numVerts = (uint32_t)V; n->numTris = num_tris;
    DevMem scratch;                       // the sort's keys, values and temporary storage: freed when create returns (it has synchronised)
    auto build = [&]() -> int {
        size_t sortTemp = 0;
        HIP_TRY(normals_sort_temp_bytes(num_tris, n->numVerts, &sortTemp));
        n->off = normals_layout(num_tris, n->numVerts, sortTemp);
        GMUPT_TRY(n->mem.grow(r->stream, n->off.kept));
        GMUPT_TRY(scratch.grow(r->stream, n->off.total - n->off.kept));
        const NmArgs a = normals_args(n, scratch.as<char>());
        HIP_TRY(hipMemcpyAsync(n->mem.as<char>() + n->off.indices, device_indices, 3 * (size_t)num_tris * 4, hipMemcpyDeviceToDevice, r->stream));
        HIP_TRY(launch_normals_create(a, scratch.as<char>() + (n->off.sortTemp - n->off.kept), sortTemp, r->stream));
        uint32_t back[2] = { 0, 0 };
        GMUPT_TRY(copy_sync(back, a.words, sizeof(back), hipMemcpyDeviceToHost, r->stream));
        if (back[0] & kNmFlagBadIndex) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_normals_create: a triangle references a vertex outside the vertex buffer (%zu vertices)", V);
        n->maxValence = back[1];
        return GMUPT_OK;
    };
    const int rc = build();
    if (rc != GMUPT_OK) { (void)hipStreamSynchronize(r->stream); delete n; return rc; }
    *out = n;
    return GMUPT_OK;
}

extern "C" void gmupt_normals_destroy(gmupt_normals* n)
{
    if (!n) return;
    (void)hipSetDevice(n->r->dev->id);
    (void)hipStreamSynchronize(n->r->stream);
    delete n;
}

extern "C" int gmupt_normals_update(gmupt_normals* n, gmupt_normals_info* info)
{
    if (!n) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_normals_update: null handle");
    if (info) *info = gmupt_normals_info{};
    gmupt_renderer* r = n->r;
    if (!r->sceneBound) return fail(GMUPT_ERR_NOT_BOUND, "gmupt_normals_update: no scene bound");
    if (r->boundVerts->elems != n->numVerts)
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_normals_update: the bound vertex buffer holds %zu vertices, the handle was created for %u", r->boundVerts->elems, n->numVerts);
    if (r->boundProps->elems < n->numVerts)
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_normals_update: %zu property records for %u vertices", r->boundProps->elems, n->numVerts);
    HIP_TRY(hipSetDevice(r->dev->id));
    NmArgs a = normals_args(n);
    a.verts = (const float*)r->boundVerts->dptr; a.props = (gmupt_tri_props*)r->boundProps->dptr;
    if (info) GMUPT_TRY(n->ev.start(r->stream));
    launch_normals_update(a, r->stream);
    HIP_TRY(hipGetLastError());
    if (!info) return GMUPT_OK;
    GMUPT_TRY(n->ev.stop(r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    float ms = 0.0f;
    GMUPT_TRY(n->ev.elapsed_ms(&ms));
    info->num_verts = n->numVerts; info->num_tris = n->numTris; info->max_valence = n->maxValence; info->ms = (double)ms;
    return GMUPT_OK;
}
