// C-ABI of libgmupt.so: the treelet optimiser on the device (gmupt_treeopt_*, pt_treeopt.hip).
#include "gmupt_internal.hpp"

extern "C" int gmupt_treeopt_create(gmupt_device* dev, gmupt_treeopt** out)
{
    if (!dev || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_treeopt_create: null argument");
    *out = nullptr;
    gmupt_treeopt* h = new (std::nothrow) gmupt_treeopt();
    if (!h) return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_treeopt_create: out of host memory");
    h->dev = dev;
    hipError_t e = hipSetDevice(dev->id);
    if (e == hipSuccess) e = hipStreamCreate(&h->stream);
    if (e != hipSuccess) { gmupt_treeopt_destroy(h); return fail(GMUPT_ERR_HIP, "gmupt_treeopt_create: %s", hipGetErrorString(e)); }
    *out = h;
    return GMUPT_OK;
}

extern "C" void gmupt_treeopt_destroy(gmupt_treeopt* h)
{
    if (!h) return;
    (void)hipSetDevice(h->dev->id);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    delete h;
}

extern "C" int gmupt_treeopt_run(gmupt_treeopt* h, const gmupt_buffer* nodes, const gmupt_treeopt_params* params, gmupt_buffer** nodes_out, gmupt_treeopt_info* info)
{
    if (nodes_out) *nodes_out = nullptr;
    if (!h || !nodes || !nodes_out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_treeopt_run: null argument");
    if (nodes->kind != GMUPT_BUFFER_BVH_NODES || nodes->dev != h->dev) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_treeopt_run: not a node buffer of the optimiser's device");
    if (nodes->elems == 0 || nodes->elems > 0x7FFFFFFFull || nodes->elems * sizeof(gmupt_bvh_node) > nodes->bytes)
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_treeopt_run: %zu node records (1 .. 2^31 - 1)", nodes->elems);
    uint32_t passes;
    GMUPT_TRY(treeopt_passes("gmupt_treeopt_run", params, &passes));
    const uint32_t n = (uint32_t)nodes->elems;
    HIP_TRY(hipSetDevice(h->dev->id));
    size_t sortTemp = 0;
    HIP_TRY(treeopt_sort_temp_bytes(n, &sortTemp));
    if (n > h->capNodes || sortTemp > h->sortTemp) {
        const uint32_t cap = std::max(n, h->capNodes);
        h->capNodes = 0; h->sortTemp = 0;                                       // should the scratch fail to grow
        GMUPT_TRY(h->scratch.grow(h->stream, treeopt_scratch_layout(cap, sortTemp).total));
        h->capNodes = cap; h->sortTemp = sortTemp;
    }
    const ToScratch off = treeopt_scratch_layout(h->capNodes, h->sortTemp);    // placed for the capacity: a smaller tree uses the front of each part

    const void* words = nullptr; const void* staged = nullptr;
    GMUPT_TRY(h->ev.start(h->stream));
    HIP_TRY(launch_treeopt(h->scratch.ptr, off, h->sortTemp, (const gmupt_bvh_node*)nodes->dptr, n, passes, h->stream, &words, &staged));
    GMUPT_TRY(h->ev.stop(h->stream));
    uint32_t back[kToWordCost + 4] = { 0 };
    GMUPT_TRY(copy_sync(back, words, sizeof(back), hipMemcpyDeviceToHost, h->stream));
    if (back[0] & kToFlagBadLink) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_treeopt_run: an inner node has a child link at or below its own number, or outside the %u records", n);
    if (back[0] & kToFlagNotTree) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_treeopt_run: a record is not the child of exactly one node: not a tree over all %u records", n);
    for (uint32_t j = 0; j <= passes; j++)
        if (back[kToWordDepth + j] > kToMaxDepth)
            return j == 0 ? fail(GMUPT_ERR_UNSUPPORTED, "gmupt_treeopt_run: the tree is %u levels deep, the traversal stacks hold %u", back[kToWordDepth], kToMaxDepth)
                          : fail(GMUPT_ERR_UNSUPPORTED, "gmupt_treeopt_run: the tree is %u levels deep after pass %u, the traversal stacks hold %u", back[kToWordDepth + j], j, kToMaxDepth);
    if (back[0]) return fail(GMUPT_ERR_HIP, "gmupt_treeopt_run: the device reported flags %#x", back[0]);
    float ms = 0.0f;
    GMUPT_TRY(h->ev.elapsed_ms(&ms));

    hipError_t e = hipSuccess;
    gmupt_buffer* nb = buffer_alloc(h->dev, GMUPT_BUFFER_BVH_NODES, n, (size_t)n * sizeof(gmupt_bvh_node), &e);
    if (!nb) return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_treeopt_run: out of host memory");
    if (e == hipSuccess) e = hipMemsetAsync((char*)nb->dptr + nb->bytes, 0, 16, h->stream);      // the slack
    if (e == hipSuccess) e = hipMemcpyAsync(nb->dptr, staged, nb->bytes, hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { gmupt_buffer_destroy(nb); return fail(GMUPT_ERR_HIP, "gmupt_treeopt_run(%zu bytes): %s", (size_t)n * sizeof(gmupt_bvh_node), hipGetErrorString(e)); }
    *nodes_out = nb;
    ToResult res{};
    res.numNodes = n; res.depthBefore = back[kToWordDepth]; res.depthAfter = back[kToWordDepth + passes]; res.rewritten = back[kToWordRewritten];
    std::memcpy(&res.costBefore, &back[kToWordCost], 8); std::memcpy(&res.costAfter, &back[kToWordCost + 2], 8);
    treeopt_fill_info(info, res, (double)ms);
    return GMUPT_OK;
}
