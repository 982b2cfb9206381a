// C-ABI of libgmupt.so: the treelet optimiser on the device (gmupt_treeopt_*, pt_treeopt.hip).
#include "gmupt_work.hpp"

extern "C" int gmupt_treeopt_create(gmupt_device* dev, gmupt_treeopt** out) { return work_create("gmupt_treeopt_create", dev, out); }
extern "C" void gmupt_treeopt_destroy(gmupt_treeopt* h) { work_destroy(h); }

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
    GMUPT_TRY(h->reserve(n, sortTemp, treeopt_scratch_bytes));

    const void* words = nullptr; const void* staged = nullptr;
    GMUPT_TRY(h->ev.start(h->stream));
    HIP_TRY(launch_treeopt(h->scratch.ptr, h->cap, h->sortTemp, (const gmupt_bvh_node*)nodes->dptr, n, passes, h->stream, &words, &staged));
    GMUPT_TRY(h->ev.stop(h->stream));
    uint32_t back[kToWordCost + 4] = { 0 };
    GMUPT_TRY(copy_sync(back, words, sizeof(back), hipMemcpyDeviceToHost, h->stream));
    if (back[0] & kToFlagBadLink) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_treeopt_run: an inner node has a child link at or below its own number, or outside the %u records", n);
    if (back[0] & kToFlagNotTree) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_treeopt_run: a record is not the child of exactly one node: not a tree over all %u records", n);
    for (uint32_t j = 0; j <= passes; j++)
        if (back[kToWordDepth + j] > kMaxTreeDepth)
            return j == 0 ? fail(GMUPT_ERR_UNSUPPORTED, "gmupt_treeopt_run: the tree is %u levels deep, the traversal stacks hold %u", back[kToWordDepth], kMaxTreeDepth)
                          : fail(GMUPT_ERR_UNSUPPORTED, "gmupt_treeopt_run: the tree is %u levels deep after pass %u, the traversal stacks hold %u", back[kToWordDepth + j], j, kMaxTreeDepth);
    if (back[0]) return fail(GMUPT_ERR_HIP, "gmupt_treeopt_run: the device reported flags %#x", back[0]);
    float ms = 0.0f;
    GMUPT_TRY(h->ev.elapsed_ms(&ms));

    gmupt_buffer* nb = nullptr;
    GMUPT_TRY(output_buffer(h->dev, GMUPT_BUFFER_BVH_NODES, n, staged, h->stream, "gmupt_treeopt_run", &nb));
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { gmupt_buffer_destroy(nb); return fail(GMUPT_ERR_HIP, "gmupt_treeopt_run(%zu bytes): %s", (size_t)n * sizeof(gmupt_bvh_node), hipGetErrorString(e)); }
    *nodes_out = nb;
    ToResult res{};
    res.numNodes = n; res.depthBefore = back[kToWordDepth]; res.depthAfter = back[kToWordDepth + passes]; res.rewritten = back[kToWordRewritten];
    std::memcpy(&res.costBefore, &back[kToWordCost], 8); std::memcpy(&res.costAfter, &back[kToWordCost + 2], 8);
    treeopt_fill_info(info, res, (double)ms);
    return GMUPT_OK;
}
