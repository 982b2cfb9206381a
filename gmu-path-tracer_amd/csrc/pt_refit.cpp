// The host refit (gmupt_bvh_refit_host): the box rule of pt_refit.hpp on a validated tree.  Leaves in chunks on up to `threads`
// std::threads (every leaf reads only the inputs), then the inner nodes by falling index on the calling thread (children have larger
// indices than their parent).
#include "pt_refit.hpp"
#include "pt_bands.hpp"

namespace gmupt {

void refit_host(gmupt_bvh_node* nodes, size_t N, const gmupt_triangle* tris, const float* verts, int threads)
{
    constexpr size_t kChunk = 4096;
    auto store = [&](gmupt_bvh_node& n, const RfBox& b) { for (int k = 0; k < 3; k++) { n.min[k] = b.mn[k]; n.max[k] = b.mx[k]; } };
    host_bands((int)((N + kChunk - 1) / kChunk), threads, [&](int c0, int c1) {
        for (size_t i = (size_t)c0 * kChunk; i < std::min(N, (size_t)c1 * kChunk); i++)
            if (nodes[i].isLeaf && nodes[i].right > nodes[i].left) store(nodes[i], rf_leaf_box(tris, verts, nodes[i].left, nodes[i].right));
    });
    for (size_t i = N; i-- > 0;) {
        if (nodes[i].isLeaf) continue;
        const gmupt_bvh_node& l = nodes[(size_t)nodes[i].left];
        const gmupt_bvh_node& r = nodes[(size_t)nodes[i].right];
        store(nodes[i], rf_union(l.min, l.max, r.min, r.max));
    }
}

} // namespace gmupt
