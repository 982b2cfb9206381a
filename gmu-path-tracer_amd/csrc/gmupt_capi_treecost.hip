// C-ABI of libgmupt.so: the tree cost of a node buffer on the device (gmupt_renderer_tree_cost, pt_treecost.hip).
#include "gmupt_internal.hpp"

static_assert(sizeof(gmupt_tree_cost_info) == 64 && offsetof(gmupt_tree_cost_info, num_refs) == 24 && offsetof(gmupt_tree_cost_info, root_half_area) == 40 &&
              offsetof(gmupt_tree_cost_info, ms) == 56, "gmupt_tree_cost_info layout");

extern "C" int gmupt_renderer_tree_cost(gmupt_renderer* r, gmupt_buffer* nodes_or_null, gmupt_tree_cost_info* info)
{
    if (!r || !info) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_tree_cost: null argument");
    const gmupt_buffer* nodes = nodes_or_null;
    if (!nodes) {
        if (!r->sceneBound) return fail(GMUPT_ERR_NOT_BOUND, "gmupt_renderer_tree_cost: no scene bound");
        nodes = r->boundNodes;
    }
    if (nodes->kind != GMUPT_BUFFER_BVH_NODES) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_tree_cost: a buffer of kind %d, not GMUPT_BUFFER_BVH_NODES", (int)nodes->kind);
    if (nodes->dev->id != r->dev->id) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_tree_cost: the buffer lives on device %d, the renderer on device %d", nodes->dev->id, r->dev->id);
    if (nodes->elems == 0 || nodes->elems > 0xFFFFFFFFull || nodes->elems * sizeof(gmupt_bvh_node) > nodes->bytes)
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_tree_cost: %zu node records (1 .. 2^32 - 1)", nodes->elems);
    const uint32_t n = (uint32_t)nodes->elems;
    HIP_TRY(hipSetDevice(r->dev->id));
    GMUPT_TRY(r->tcScratch.grow(r->stream, tree_cost_scratch_partials(n) * sizeof(TcPartial)));
    GMUPT_TRY(r->tcEv.start(r->stream));
    const TcPartial* last = launch_tree_cost((const gmupt_bvh_node*)nodes->dptr, n, r->tcScratch.as<TcPartial>(), r->stream);
    HIP_TRY(hipGetLastError());
    GMUPT_TRY(r->tcEv.stop(r->stream));
    TcPartial total;
    GMUPT_TRY(copy_sync(&total, last, sizeof(total), hipMemcpyDeviceToHost, r->stream));
    float ms = 0.0f;
    GMUPT_TRY(r->tcEv.elapsed_ms(&ms));
    tc_fill_info(total, info);
    info->ms = (double)ms;
    return GMUPT_OK;
}
