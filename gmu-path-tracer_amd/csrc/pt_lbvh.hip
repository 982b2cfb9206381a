// The GPU LBVH builder (gmupt_lbvh_build; include/gmupt.h states the rule): Morton keys, radix sort, Karras's hierarchy, and the reference
// node / triangle layout that bind, refit and the ray casts take.  One enqueue of launches on the builder's stream, no host
// synchronisation in between; every kernel is safe on invalid input (an index outside the vertex array is flagged and never followed).
//
//   k_lb_bounds   one thread per triangle: indices in range, vertices finite (else a flag bit), centre; min / max of the block's centres
//                 (lb_block_minmax)
//   k_lb_bounds2  one block: min / max over the blocks' partial results (lb_block_minmax again) -> cmin, cmax
//   k_lb_keys     one thread per triangle: the 63-bit Morton key of its centre, value = its index
//   (sort)        rocPRIM radix sort of (key, index) on bits 0..62: stable, so equal keys keep index order
//   k_lb_hier     one thread per inner node of the binary radix tree (Karras 2012): range, split, parent links of both children.
//                 Node ids: inner node i = i (0 = root), sorted position p = numTris - 1 + p
//   k_lb_depth    one thread per node id: depth by walking the parent links (level_depth); kept = root, or the parent's range holds
//                 more than L positions; sort key = level_key(depth, first), which leaves a dropped node out
//   (sort)        level_sort of (that key, node id): the sorted position of a kept node IS its number (rule 7)
//   k_lb_levels   one thread per sorted entry: where each depth starts (level_offsets); number of each node id, node count, depth
//   k_lb_tris     one thread per sorted position: triangle record, ref_triangle
//   k_lb_nodes    one thread per kept node: links; a leaf also gets its box (rf_leaf_box on the records just written)
//   k_lb_level    inner boxes, one launch per depth 63 .. 0 on a fixed grid that strides over the nodes of that depth (the range comes
//                 from device memory, an absent depth is an empty range): children are one level down, so no atomics and no waiting
#include "pt_lbvh.hpp"
#include "pt_launch.hpp"
#include "pt_levels.hpp"          // the level step, the scratch carver, rocPRIM's radix sort

#include <cstring>

namespace gmupt {

constexpr int kLbBlock = 256;
constexpr uint32_t kLbLevelBlocks = 1024;        // grid of k_lb_level

// device words of a build (kLevelWords of them): [0] flags, [1] kept nodes, [2] depth, [4..11] the root's box rows, [16..21] cmin, cmax,
// then levelOff (pt_levels.hpp)
struct LbArgs {
    const float* verts; uint32_t numVerts;
    const int32_t* indices; uint32_t n;
    const uint32_t* vertexMaterial;
    uint32_t maxLeaf;
    float* partial; uint32_t numPartial;          // 6 floats per block of k_lb_bounds
    uint32_t* words;
    uint64_t* keysIn; uint64_t* keys; uint32_t* valsIn; uint32_t* src;          // first sort: keys / src are its outputs
    uint64_t* keys2In; uint64_t* keys2; uint32_t* vals2In; uint32_t* ids;       // second sort over 2n - 1 node ids
    int32_t* parent;      // 2n - 1
    int32_t* split;       // n - 1
    int2* range;          // n - 1
    uint32_t* number;     // 2n - 1: node id -> number
    DNode* nodes; gmupt_triangle* tris; int32_t* ref;                          // staging of the outputs
};

__device__ __forceinline__ bool lb_load_tri(const LbArgs& a, size_t i, int32_t* t)
{
    t[0] = a.indices[3 * i]; t[1] = a.indices[3 * i + 1]; t[2] = a.indices[3 * i + 2];
    return (uint32_t)t[0] < a.numVerts && (uint32_t)t[1] < a.numVerts && (uint32_t)t[2] < a.numVerts;
}

// The block's min (rows 0..2) and max (rows 3..5) of every thread's mn / mx, by halving in LDS: the result of row r is at [r][0]
using LbRow = float[kLbBlock];
__device__ __forceinline__ const LbRow* lb_block_minmax(const float* mn, const float* mx)
{
    __shared__ float red[6][kLbBlock];
    for (int k = 0; k < 3; k++) { red[k][threadIdx.x] = mn[k]; red[3 + k][threadIdx.x] = mx[k]; }
    __syncthreads();
    for (int s = kLbBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int k = 0; k < 3; k++) {
                red[k][threadIdx.x] = rf_lo(red[k][threadIdx.x], red[k][threadIdx.x + s]);
                red[3 + k][threadIdx.x] = rf_hi(red[3 + k][threadIdx.x], red[3 + k][threadIdx.x + s]);
            }
        __syncthreads();
    }
    return red;
}

__global__ __launch_bounds__(kLbBlock) void k_lb_bounds(LbArgs a)
{
    const size_t i = (size_t)blockIdx.x * kLbBlock + threadIdx.x;
    const float inf = u2f(0x7F800000u);
    float mn[3] = { inf, inf, inf }, mx[3] = { -inf, -inf, -inf };
    if (i < a.n) {
        int32_t t[3];
        uint32_t bad = 0;
        if (!lb_load_tri(a, i, t)) bad = kLbFlagBadIndex;
        else {
            const float* v0 = a.verts + 3 * (size_t)t[0]; const float* v1 = a.verts + 3 * (size_t)t[1]; const float* v2 = a.verts + 3 * (size_t)t[2];
            bool fin = true;
            for (int k = 0; k < 3; k++) fin = fin && lb_finite(v0[k]) && lb_finite(v1[k]) && lb_finite(v2[k]);
            if (!fin) bad = kLbFlagNonFinite;
            else {
                float c[3];
                lb_centre(v0, v1, v2, c);
                for (int k = 0; k < 3; k++) mn[k] = mx[k] = c[k];
            }
        }
        if (bad) atomicOr(a.words, bad);
    }
    const LbRow* red = lb_block_minmax(mn, mx);
    if (threadIdx.x < 6 && blockIdx.x < a.numPartial) a.partial[6 * (size_t)blockIdx.x + threadIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(kLbBlock) void k_lb_bounds2(LbArgs a)
{
    const float inf = u2f(0x7F800000u);
    float mn[3] = { inf, inf, inf }, mx[3] = { -inf, -inf, -inf };
    for (size_t b = threadIdx.x; b < a.numPartial; b += kLbBlock)
        for (int k = 0; k < 3; k++) { mn[k] = rf_lo(mn[k], a.partial[6 * b + k]); mx[k] = rf_hi(mx[k], a.partial[6 * b + 3 + k]); }
    const LbRow* red = lb_block_minmax(mn, mx);
    if (threadIdx.x < 6) a.words[16 + threadIdx.x] = f2u(red[threadIdx.x][0]);
}

__global__ __launch_bounds__(kLbBlock) void k_lb_keys(LbArgs a)
{
    const size_t i = (size_t)blockIdx.x * kLbBlock + threadIdx.x;
    if (i >= a.n) return;
    int32_t t[3];
    uint64_t key = 0;
    if (lb_load_tri(a, i, t)) {
        float c[3], cmin[3], ext[3];
        lb_centre(a.verts + 3 * (size_t)t[0], a.verts + 3 * (size_t)t[1], a.verts + 3 * (size_t)t[2], c);
        for (int k = 0; k < 3; k++) { cmin[k] = u2f(a.words[16 + k]); ext[k] = u2f(a.words[19 + k]) - cmin[k]; }
        key = lb_key(c, cmin, ext);
    }
    a.keysIn[i] = key;
    a.valsIn[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kLbBlock) void k_lb_hier(LbArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kLbBlock + threadIdx.x;
    const int64_t n = a.n;
    if (i == 0) a.parent[0] = -1;
    if (i >= n - 1) return;
    const uint64_t* keys = a.keys;
    // Karras 2012, figure 4: direction, an upper bound of the length, the other end by binary search
    const int64_t d = lb_delta_r(keys, n, i, i + 1) > lb_delta_r(keys, n, i, i - 1) ? 1 : -1;
    const int dmin = lb_delta_r(keys, n, i, i - d);
    int64_t lmax = 2;
    while (lb_delta_r(keys, n, i, i + lmax * d) > dmin) lmax <<= 1;
    int64_t l = 0;
    for (int64_t t = lmax >> 1; t >= 1; t >>= 1)
        if (lb_delta_r(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int64_t first = d > 0 ? i : j, last = d > 0 ? j : i;
    if (last <= first) return;                                       // (cannot happen: (key, position) pairs are distinct)
    const int64_t s = lb_split(keys, first, last);
    a.range[i] = make_int2((int)first, (int)last);
    a.split[i] = (int32_t)s;
    const int64_t leftId = s == first ? n - 1 + s : s, rightId = s + 1 == last ? n - 1 + s + 1 : s + 1;
    a.parent[leftId] = (int32_t)i;
    a.parent[rightId] = (int32_t)i;
}

__global__ __launch_bounds__(kLbBlock) void k_lb_depth(LbArgs a)
{
    const int64_t id = (int64_t)blockIdx.x * kLbBlock + threadIdx.x;
    const int64_t n = a.n, M = 2 * n - 1;
    if (id >= M) return;
    const uint32_t first = id < n - 1 ? (uint32_t)a.range[id].x : (uint32_t)(id - (n - 1));
    const int32_t par = a.parent[id];                                  // the root's is -1 (k_lb_hier)
    const uint32_t depth = level_depth(a.parent, par, (uint32_t)(n - 1));
    bool kept = id == 0;
    if (par >= 0 && (int64_t)par < n - 1) { const int2 r = a.range[par]; kept = (uint32_t)(r.y - r.x + 1) > a.maxLeaf; }
    a.keys2In[id] = level_key(kept, depth, first);
    a.vals2In[id] = (uint32_t)id;
}

__global__ __launch_bounds__(kLbBlock) void k_lb_levels(LbArgs a)
{
    const int64_t pos = (int64_t)blockIdx.x * kLbBlock + threadIdx.x;
    const int64_t M = 2 * (int64_t)a.n - 1;
    if (pos >= M) return;
    const LevelEntry e = level_offsets(a.keys2, (size_t)pos, (size_t)M, a.words + kLevelWord);
    if (e.depth != kLevelDropped) a.number[a.ids[pos]] = (uint32_t)pos;
    if (e.count) { a.words[1] = e.count; a.words[2] = e.last; }
}

__global__ __launch_bounds__(kLbBlock) void k_lb_tris(LbArgs a)
{
    const size_t pos = (size_t)blockIdx.x * kLbBlock + threadIdx.x;
    if (pos >= a.n) return;
    const uint32_t src = a.src[pos];
    int32_t t[3];
    gmupt_triangle rec;
    if (src < a.n && lb_load_tri(a, src, t)) rec = lb_record(t, a.vertexMaterial);
    else { rec.v[0] = rec.v[1] = rec.v[2] = 0; rec.materialID = 0; }
    *reinterpret_cast<int4*>(a.tris + pos) = make_int4(rec.v[0], rec.v[1], rec.v[2], (int)rec.materialID);
    a.ref[pos] = (int32_t)src;
}

__global__ __launch_bounds__(kLbBlock) void k_lb_nodes(LbArgs a)
{
    const int64_t pos = (int64_t)blockIdx.x * kLbBlock + threadIdx.x;
    const int64_t n = a.n, M = 2 * n - 1;
    if (pos >= M) return;
    const uint64_t key = a.keys2[pos];
    if (level_key_depth(key) == kLevelDropped) return;
    const int64_t id = a.ids[pos];
    if (id >= M) return;
    const int64_t first = (uint32_t)key;
    const int64_t last = id < n - 1 ? (int64_t)a.range[id].y : first;
    if (first > last || last >= n) return;
    DNode o;
    o.mn = make_float4(0.0f, 0.0f, 0.0f, 0.0f); o.mx = o.mn;
    if ((uint64_t)(last - first + 1) <= a.maxLeaf) {
        const RfBox b = rf_leaf_box(a.tris, a.verts, (int32_t)first, (int32_t)last + 1);
        o.mn = make_float4(b.mn[0], b.mn[1], b.mn[2], 0.0f); o.mx = make_float4(b.mx[0], b.mx[1], b.mx[2], 0.0f);
        o.link = make_int4((int)first, (int)last + 1, 1, 0);
    } else {
        const int64_t s = a.split[id];
        const int64_t leftId = s == first ? n - 1 + s : s;
        const int left = leftId >= 0 && leftId < M ? (int)a.number[leftId] : 0;
        o.link = make_int4(left, left + 1, 0, 0);
    }
    a.nodes[pos] = o;
}

__global__ __launch_bounds__(kLbBlock) void k_lb_level(LbArgs a, uint32_t depth)
{
    const uint32_t begin = a.words[kLevelWord + depth], end = a.words[kLevelWord + depth + 1];
    const uint32_t kept = a.words[1];
    for (size_t i = (size_t)begin + (size_t)blockIdx.x * kLbBlock + threadIdx.x; i < end && i < kept; i += (size_t)gridDim.x * kLbBlock) {
        const int4 link = a.nodes[i].link;
        if (link.z || (uint32_t)link.x >= kept || (uint32_t)link.y >= kept) continue;
        const float4 lmn = a.nodes[link.x].mn, lmx = a.nodes[link.x].mx, rmn = a.nodes[link.y].mn, rmx = a.nodes[link.y].mx;
        const RfBox b = rf_union(&lmn.x, &lmx.x, &rmn.x, &rmx.x);
        a.nodes[i].mn = make_float4(b.mn[0], b.mn[1], b.mn[2], 0.0f);
        a.nodes[i].mx = make_float4(b.mx[0], b.mx[1], b.mx[2], 0.0f);
    }
}

static inline uint32_t lb_grid(size_t n) { return grid_for(n, kLbBlock); }

// ---- host side (gmupt_capi_accel.hip: gmupt_lbvh_build) ----

// bytes of temporary storage the two sorts of a build of n triangles need
hipError_t lbvh_sort_temp_bytes(uint32_t n, size_t* bytes)
{
    size_t b1 = 0, b2 = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, b1, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0u, 63u, (hipStream_t)0);
    if (e == hipSuccess) e = level_sort_temp_bytes(2 * (size_t)n - 1, &b2);
    *bytes = std::max(scratch_align(std::max(b1, (size_t)256)), b2);
    return e;
}

// The parts of a build's scratch, taken for a capacity of `cap` triangles; returns the sort's temporary storage (sortTemp bytes), the
// last part.  Staged outputs: nodes, tris, ref.
static void* lbvh_carve(Scratch& sc, uint32_t cap, size_t sortTemp, LbArgs& a)
{
    const size_t n = cap, M = 2 * n - 1;
    a.words = sc.take<uint32_t>(kLevelWords);
    a.partial = sc.take<float>(6 * (size_t)lb_grid(n));
    a.keysIn = sc.take<uint64_t>(n); a.keys = sc.take<uint64_t>(n); a.valsIn = sc.take<uint32_t>(n); a.src = sc.take<uint32_t>(n);
    a.keys2In = sc.take<uint64_t>(M); a.keys2 = sc.take<uint64_t>(M); a.vals2In = sc.take<uint32_t>(M); a.ids = sc.take<uint32_t>(M);
    a.parent = sc.take<int32_t>(M); a.split = sc.take<int32_t>(n); a.range = sc.take<int2>(n); a.number = sc.take<uint32_t>(M);
    a.nodes = sc.take<DNode>(M);
    a.tris = sc.take<gmupt_triangle>(n + 1);                           // 16 bytes of slack, as a triangle buffer has
    a.ref = sc.take<int32_t>(n);
    return sc.take<char>(sortTemp);
}

size_t lbvh_scratch_bytes(uint32_t cap, size_t sortTemp)
{
    Scratch sc(nullptr);
    LbArgs a{};
    lbvh_carve(sc, cap, sortTemp, a);
    return sc.used;
}

// enqueues the whole build in a scratch of lbvh_scratch_bytes(cap, sortTemp), cap >= n; the caller reads the words back from st.words afterwards
hipError_t launch_lbvh(void* scratch, uint32_t cap, size_t sortTemp, const float* verts, uint32_t numVerts, const int32_t* indices, uint32_t n,
                       const uint32_t* vertexMaterial, uint32_t maxLeaf, hipStream_t s, LbStaging& st)
{
    Scratch sc(scratch);
    LbArgs a{};
    a.verts = verts; a.numVerts = numVerts; a.indices = indices; a.n = n; a.vertexMaterial = vertexMaterial; a.maxLeaf = maxLeaf;
    a.numPartial = lb_grid(n);
    void* temp = lbvh_carve(sc, cap, sortTemp, a);
    st.words = a.words; st.nodes = a.nodes; st.tris = a.tris; st.ref = a.ref;
    const size_t M = 2 * (size_t)n - 1;

    hipError_t e = hipMemsetAsync(a.words, 0, kLevelWords * 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_lb_bounds, dim3(lb_grid(n)), dim3(kLbBlock), 0, s, a);
    hipLaunchKernelGGL(k_lb_bounds2, dim3(1), dim3(kLbBlock), 0, s, a);
    hipLaunchKernelGGL(k_lb_keys, dim3(lb_grid(n)), dim3(kLbBlock), 0, s, a);
    size_t tb = sortTemp;
    e = rocprim::radix_sort_pairs(temp, tb, a.keysIn, a.keys, a.valsIn, a.src, (size_t)n, 0u, 63u, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_lb_hier, dim3(lb_grid(n)), dim3(kLbBlock), 0, s, a);
    hipLaunchKernelGGL(k_lb_depth, dim3(lb_grid(M)), dim3(kLbBlock), 0, s, a);
    tb = sortTemp;
    e = level_sort(temp, tb, a.keys2In, a.keys2, a.vals2In, a.ids, M, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_lb_levels, dim3(lb_grid(M)), dim3(kLbBlock), 0, s, a);
    hipLaunchKernelGGL(k_lb_tris, dim3(lb_grid(n)), dim3(kLbBlock), 0, s, a);
    hipLaunchKernelGGL(k_lb_nodes, dim3(lb_grid(M)), dim3(kLbBlock), 0, s, a);
    const uint32_t levelGrid = std::min(lb_grid(M), kLbLevelBlocks);
    for (uint32_t d = kMaxTreeDepth; d-- > 0;) hipLaunchKernelGGL(k_lb_level, dim3(levelGrid), dim3(kLbBlock), 0, s, a, d);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(a.words + 4, a.nodes, 32, hipMemcpyDeviceToDevice, s);      // the root's box rows next to the counts
}

} // namespace gmupt
