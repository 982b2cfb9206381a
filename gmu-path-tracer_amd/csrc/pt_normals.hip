// Smooth vertex normals on the device (gmupt_normals_*; include/gmupt.h states the rule): the normals inside the property records
// recomputed from the vertex buffer the renderer is bound to.  No float atomics: a vertex's sum has a stated order.
//
// create, once per index list (one enqueue, no host synchronisation in between):
//   k_nm_keys     one thread per corner: its vertex index as the sort key (an index outside the vertex array: a flag bit, and the
//                 key numVerts, which sorts behind every vertex and is never followed), its corner number as the value
//   (sort)        rocPRIM radix sort of (vertex, corner) on the bits numVerts needs: stable, so a vertex's corners keep ascending order
//   k_nm_offsets  one thread per vertex 0 .. numVerts: the first sorted position whose key is not below it (binary search), and the
//                 largest valence (integer atomicMax, one per wave)
// update, per pose: two streaming launches
//   k_nm_faces    one thread per triangle: coalesced index read, three vertex gathers, one 16-byte face-vector store
//   k_nm_verts    one thread per vertex: walks its corner range in order, gathers the face vectors, sums, normalises, stores the normal.
//                 A vertex of very high valence serialises its thread; that is accepted (DESIGN.md "Normals").
// The index list is the handle's own copy, validated by create, and update refuses another vertex count: the update kernels follow the
// indices without a further check.  All arithmetic is pt_normals.hpp, which gmupt_vertex_normals_host runs too.
#include "pt_normals.hpp"
#include "pt_launch.hpp"
#include "pt_scratch.hpp"

#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>

namespace gmupt {

constexpr int kNmBlock = 256;
constexpr uint32_t kNmWords = 16;

__global__ __launch_bounds__(kNmBlock) void k_nm_keys(NmArgs a)
{
    const size_t c = (size_t)blockIdx.x * kNmBlock + threadIdx.x;
    if (c >= 3 * (size_t)a.numTris) return;
    uint32_t v = (uint32_t)a.indices[c];
    if (v >= a.numVerts) { atomicOr(a.words, kNmFlagBadIndex); v = a.numVerts; }
    a.keysIn[c] = v;
    a.valsIn[c] = (uint32_t)c;
}

__global__ __launch_bounds__(kNmBlock) void k_nm_offsets(NmArgs a)
{
    const size_t v = (size_t)blockIdx.x * kNmBlock + threadIdx.x;
    const size_t C = 3 * (size_t)a.numTris;
    uint32_t valence = 0;
    if (v <= a.numVerts) {
        // lower bound of v, and of v + 1 for the valence (the neighbour thread stores that one)
        size_t lo[2] = { 0, 0 };
        for (int k = 0; k < 2; k++) {
            size_t b = 0, e = C;
            while (b < e) { const size_t m = b + ((e - b) >> 1); if (a.keys[m] < (uint32_t)v + k) b = m + 1; else e = m; }
            lo[k] = b;
        }
        a.offsets[v] = (uint32_t)lo[0];
        if (v < a.numVerts) valence = (uint32_t)(lo[1] - lo[0]);
    }
    for (int s = 32; s > 0; s >>= 1) valence = max(valence, (uint32_t)__shfl_xor((int)valence, s, 64));
    if ((threadIdx.x & 63) == 0 && valence) atomicMax(a.words + 1, valence);
}

__global__ __launch_bounds__(kNmBlock) void k_nm_faces(NmArgs a)
{
    const size_t t = (size_t)blockIdx.x * kNmBlock + threadIdx.x;
    if (t >= a.numTris) return;
    const int32_t* i = a.indices + 3 * t;
    float f[3];
    nm_face(a.verts + 3 * (size_t)i[0], a.verts + 3 * (size_t)i[1], a.verts + 3 * (size_t)i[2], f);
    a.faces[t] = make_float4(f[0], f[1], f[2], 0.0f);
}

// The store is 12 bytes into a 32-byte-stride record.  The other candidate -- the whole record read and written back with 16-byte accesses,
// full lines -- measured the same (DESIGN.md "Normals") and was retired.
__global__ __launch_bounds__(kNmBlock) void k_nm_verts(NmArgs a)
{
    const size_t v = (size_t)blockIdx.x * kNmBlock + threadIdx.x;
    if (v >= a.numVerts) return;
    const uint32_t begin = a.offsets[v], end = a.offsets[v + 1];
    float s[3] = { 0.0f, 0.0f, 0.0f }, n[3];
    for (uint32_t i = begin; i < end; i++) {
        const float4 f = a.faces[a.corners[i] / 3u];
        s[0] = s[0] + f.x; s[1] = s[1] + f.y; s[2] = s[2] + f.z;
    }
    nm_finish(s, n);
    *reinterpret_cast<float3*>(a.props + v) = make_float3(n[0], n[1], n[2]);
}

static inline uint32_t nm_grid(size_t n) { return grid_for(n, kNmBlock); }
static inline unsigned nm_key_bits(uint32_t numVerts) { unsigned b = 1; while (b < 32 && (numVerts >> b)) b++; return b; }   // the keys are 0 .. numVerts

// ---- host side (gmupt_capi_normals.hip) ----

hipError_t normals_sort_temp_bytes(uint32_t numTris, uint32_t numVerts, size_t* bytes)
{
    size_t b = 0;
    const hipError_t e = rocprim::radix_sort_pairs(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                                   3 * (size_t)numTris, 0u, nm_key_bits(numVerts), (hipStream_t)0);
    *bytes = scratch_align(std::max(b, (size_t)256));
    return e;
}

NmLayout normals_layout(uint32_t numTris, uint32_t numVerts, size_t sortTemp)
{
    const size_t C = 3 * (size_t)numTris;
    NmLayout L{};
    size_t total = 0;
    auto place = [&total](size_t& off, size_t bytes) { off = total; total += scratch_align(bytes); };
    place(L.words, kNmWords * 4);
    place(L.indices, C * 4);
    place(L.corners, C * 4);
    place(L.offsets, ((size_t)numVerts + 1) * 4);
    place(L.faces, (size_t)numTris * 16);
    L.kept = total;
    place(L.keysIn, C * 4);
    place(L.keys, C * 4);
    place(L.valsIn, C * 4);
    place(L.sortTemp, sortTemp);
    L.total = total;
    return L;
}

// enqueues the adjacency build; a.words (kNmWords words, cleared here) is read back by the caller afterwards
hipError_t launch_normals_create(const NmArgs& a, void* sortTemp, size_t sortTempBytes, hipStream_t s)
{
    const size_t C = 3 * (size_t)a.numTris;
    hipError_t e = hipMemsetAsync(a.words, 0, kNmWords * 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_nm_keys, dim3(nm_grid(C)), dim3(kNmBlock), 0, s, a);
    e = rocprim::radix_sort_pairs(sortTemp, sortTempBytes, a.keysIn, a.keys, a.valsIn, a.corners, C, 0u, nm_key_bits(a.numVerts), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_nm_offsets, dim3(nm_grid((size_t)a.numVerts + 1)), dim3(kNmBlock), 0, s, a);
    return hipGetLastError();
}

void launch_normals_update(const NmArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_nm_faces, dim3(nm_grid(a.numTris)), dim3(kNmBlock), 0, s, a);
    hipLaunchKernelGGL(k_nm_verts, dim3(nm_grid(a.numVerts)), dim3(kNmBlock), 0, s, a);
}

} // namespace gmupt
