// The treelet optimiser on the device (gmupt_treeopt_run; include/gmupt.h "Tree optimisation" states the rule): restructures a node buffer
// so that its surface-area cost falls (Karras & Aila 2013, section 3).  One enqueue of launches on the optimiser's stream, no host
// synchronisation in between; no launch depends on another workgroup of the same launch -- a level is a launch and the stream orders the
// levels, as in k_lb_level.  Every kernel checks what it indexes with; once a flag is set the later kernels return at once.
//
//   k_to_init     one thread per record: the working copy, parent links and reference counts (a child link outside (i, N) is flagged and
//                 not followed), the cost of a leaf
//   k_to_check    one thread per record: the child of exactly one node (the root: of none), else a flag
//   k_to_depth    one thread per working id: depth by walking the parent links (level_depth); sort key = level_key(depth, id), which
//                 leaves a leaf out of the sort of a pass; the largest depth of the launch, a flag when it is beyond 64
//   (sort)        level_sort of (key, id)
//   k_to_levels   one thread per sorted entry: where each depth starts (level_offsets); in the last sort also the number of each id
//   k_to_level    one launch per depth 63 .. 0 and pass, one WAVE per inner node of that depth on a fixed grid that strides over the level:
//                 lane 0 grows the treelet (to_form) and refreshes the node; the lanes share out the 2^k subsets -- half areas first, then
//                 the subsets of 2, 3, .. k leaves, a barrier between two sizes -- with a[], c[] and the partitions in LDS (2.5 KiB per
//                 wave); lane 0 rewrites the treelet when the optimum is cheaper (to_rewrite)
//   k_to_emit     one thread per sorted position: the record with its links renumbered
//   k_to_finish   one thread: the two costs next to the other words of the readback
#include "pt_treeopt.hpp"
#include "pt_launch.hpp"
#include "pt_levels.hpp"          // the level step (its sort is the only one of a run), the scratch carver

namespace gmupt {

constexpr int kToBlock = 256;
constexpr uint32_t kToWaves = kToBlock / 64;     // treelets per block of k_to_level
constexpr uint32_t kToLevelBlocks = 2048;        // grid of k_to_level

struct ToArgs {
    const gmupt_bvh_node* in; uint32_t n;
    uint32_t* words;
    gmupt_bvh_node* work; gmupt_bvh_node* out;
    int32_t* parent; uint32_t* refs;
    double* cost; double* cost0;
    uint64_t* keysIn; uint64_t* keys; uint32_t* valsIn; uint32_t* ids;
    uint32_t* number;
};

__global__ __launch_bounds__(kToBlock) void k_to_init(ToArgs a)
{
    const size_t i = (size_t)blockIdx.x * kToBlock + threadIdx.x;
    if (i >= a.n) return;
    const gmupt_bvh_node x = a.in[i];
    a.work[i] = x;
    if (i == 0) a.parent[0] = -1;
    if (x.isLeaf) { const double c = to_leaf_cost(x); a.cost[i] = c; a.cost0[i] = c; return; }
    a.cost[i] = 0.0; a.cost0[i] = 0.0;
    if (x.left <= (int32_t)i || x.right <= (int32_t)i || (uint32_t)x.left >= a.n || (uint32_t)x.right >= a.n) { atomicOr(a.words, kToFlagBadLink); return; }
    atomicAdd(a.refs + x.left, 1u); atomicAdd(a.refs + x.right, 1u);
    a.parent[x.left] = (int32_t)i; a.parent[x.right] = (int32_t)i;
}

__global__ __launch_bounds__(kToBlock) void k_to_check(ToArgs a)
{
    const size_t i = (size_t)blockIdx.x * kToBlock + threadIdx.x;
    if (i >= a.n) return;
    if (a.refs[i] != (i ? 1u : 0u)) atomicOr(a.words, kToFlagNotTree);
}

__global__ __launch_bounds__(kToBlock) void k_to_depth(ToArgs a, uint32_t call, uint32_t last)
{
    // only flags of earlier launches end this one: kToFlagDeep is set by this very kernel, and a block that left on seeing it would
    // leave its depths out of the maximum the error message quotes
    if (a.words[0] & (kToFlagBadLink | kToFlagNotTree)) return;
    const size_t id = (size_t)blockIdx.x * kToBlock + threadIdx.x;
    uint32_t depth = 0;
    if (id < a.n) {
        depth = level_depth(a.parent, a.parent[id], a.n);
        a.keysIn[id] = level_key(last || a.work[id].isLeaf == 0, depth, (uint32_t)id);
        a.valsIn[id] = (uint32_t)id;
    }
    uint32_t top = depth;
    for (int s = 32; s > 0; s >>= 1) top = max(top, (uint32_t)__shfl_xor((int)top, s, 64));
    if ((threadIdx.x & 63u) == 0 && top) {
        atomicMax(a.words + kToWordDepth + call, top);
        if (top > kMaxTreeDepth) atomicOr(a.words, kToFlagDeep);
    }
}

__global__ __launch_bounds__(kToBlock) void k_to_levels(ToArgs a, uint32_t last)
{
    if (a.words[0]) return;
    const size_t pos = (size_t)blockIdx.x * kToBlock + threadIdx.x;
    const size_t M = a.n;
    if (pos >= M) return;
    const LevelEntry e = level_offsets(a.keys, pos, M, a.words + kLevelWord);
    if (e.depth != kLevelDropped) {
        const uint32_t id = a.ids[pos];
        if (last && id < a.n) a.number[id] = (uint32_t)pos;
    }
}

// the LDS of one wave of k_to_level
struct ToWave {
    ToTreelet t;
    double a[kToSubsets], c[kToSubsets];
    uint8_t part[kToSubsets];
    double cX;
    uint32_t run;
};

__global__ __launch_bounds__(kToBlock) void k_to_level(ToArgs a, uint32_t depth, uint32_t firstPass)
{
    __shared__ ToWave sh[kToWaves];
    __shared__ uint32_t flagged;
    // another workgroup of this launch may set a flag (to_form below): one thread reads the word, so that the whole block takes the same
    // way round the barriers of the loop
    if (threadIdx.x == 0) flagged = a.words[0];
    __syncthreads();
    if (flagged) return;
    const uint32_t begin = a.words[kLevelWord + depth], end = min(a.words[kLevelWord + depth + 1], a.n);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    ToWave& S = sh[wave];
    // the trip count is the same for the waves of a block: the barriers below are met by all of them
    for (size_t base = (size_t)begin + (size_t)blockIdx.x * kToWaves; base < end; base += (size_t)gridDim.x * kToWaves) {
        const size_t idx = base + wave;
        if (lane == 0) {
            S.run = 0;
            const uint32_t X = idx < end ? a.ids[idx] : 0xFFFFFFFFu;
            if (X < a.n && a.work[X].isLeaf == 0) {
                if (!to_form(a.work, a.n, (int32_t)X, S.t)) atomicOr(a.words, kToFlagBadLink);
                else {
                    const int32_t l0 = a.work[X].left, r0 = a.work[X].right;
                    const double aX = to_refresh(a.work, (int32_t)X);
                    const double cX = to_inner_cost(aX, a.cost[l0], a.cost[r0]);
                    if (firstPass) a.cost0[X] = to_inner_cost(aX, a.cost0[l0], a.cost0[r0]);
                    a.cost[X] = cX;
                    S.cX = cX;
                    S.run = S.t.k >= 3 ? 1u : 0u;
                }
            }
        }
        __syncthreads();
        const uint32_t run = S.run, k = run ? S.t.k : 0u, count = 1u << k;
        if (run)
            for (uint32_t s = lane; s < count; s += 64) {
                if (!s) continue;
                S.a[s] = to_subset_area(S.t, s);
                if (!(s & (s - 1u))) { S.c[s] = a.cost[S.t.slot[to_lowest_slot(s)]]; S.part[s] = 0; }
            }
        __syncthreads();
        for (uint32_t m = 2; m <= kToLeaves; m++) {
            if (run && m <= k)
                for (uint32_t s = lane; s < count; s += 64) {
                    if ((uint32_t)__popc(s) != m) continue;
                    uint32_t p;
                    const double v = to_partition_scan(S.c, s, &p);
                    S.c[s] = S.a[s] * 2.0 + v; S.part[s] = (uint8_t)p;
                }
            __syncthreads();
        }
        if (run && lane == 0 && S.c[count - 1u] < S.cX) {
            to_rewrite(a.work, a.parent, a.cost, (int32_t)a.ids[idx], S.t, S.c, S.part);
            atomicAdd(a.words + kToWordRewritten, 1u);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kToBlock) void k_to_emit(ToArgs a)
{
    if (a.words[0]) return;
    const size_t pos = (size_t)blockIdx.x * kToBlock + threadIdx.x;
    if (pos >= a.n) return;
    const uint32_t id = a.ids[pos];
    if (id >= a.n) return;
    gmupt_bvh_node o = a.work[id];
    if (o.isLeaf == 0) {
        if ((uint32_t)o.left >= a.n || (uint32_t)o.right >= a.n) { atomicOr(a.words, kToFlagBadLink); return; }
        o.left = (int32_t)a.number[o.left]; o.right = (int32_t)a.number[o.right];
    }
    a.out[pos] = o;
}

__global__ void k_to_finish(ToArgs a)
{
    double* c = reinterpret_cast<double*>(a.words + kToWordCost);
    c[0] = a.cost0[0]; c[1] = a.cost[0];
}

// ---- host side (gmupt_capi_treeopt.hip) ----

// bytes of temporary storage the sorts of a run over n nodes need
hipError_t treeopt_sort_temp_bytes(uint32_t n, size_t* bytes) { return level_sort_temp_bytes(n, bytes); }

// The parts of a run's scratch, taken for a capacity of `cap` nodes; returns the sort's temporary storage (sortTemp bytes), the last
// part.  a.out is the staged output.
static void* treeopt_carve(Scratch& sc, uint32_t cap, size_t sortTemp, ToArgs& a)
{
    const size_t N = cap;
    a.words = sc.take<uint32_t>(kLevelWords);
    a.work = sc.take<gmupt_bvh_node>(N); a.out = sc.take<gmupt_bvh_node>(N);
    a.parent = sc.take<int32_t>(N); a.refs = sc.take<uint32_t>(N);
    a.cost = sc.take<double>(N); a.cost0 = sc.take<double>(N);
    a.keysIn = sc.take<uint64_t>(N); a.keys = sc.take<uint64_t>(N); a.valsIn = sc.take<uint32_t>(N); a.ids = sc.take<uint32_t>(N);
    a.number = sc.take<uint32_t>(N);
    return sc.take<char>(sortTemp);
}

size_t treeopt_scratch_bytes(uint32_t cap, size_t sortTemp)
{
    Scratch sc(nullptr);
    ToArgs a{};
    treeopt_carve(sc, cap, sortTemp, a);
    return sc.used;
}

// enqueues the whole run in a scratch of treeopt_scratch_bytes(cap, sortTemp), cap >= n; the caller reads the words back from *words
// afterwards, the staged output is at *staged
hipError_t launch_treeopt(void* scratch, uint32_t cap, size_t sortTemp, const gmupt_bvh_node* nodes, uint32_t n, uint32_t passes, hipStream_t s,
                          const void** words, const void** staged)
{
    Scratch sc(scratch);
    ToArgs a{};
    a.in = nodes; a.n = n;
    void* temp = treeopt_carve(sc, cap, sortTemp, a);
    *words = a.words; *staged = a.out;
    const uint32_t grid = grid_for(n, kToBlock), levelGrid = std::min((n + kToWaves - 1) / kToWaves, kToLevelBlocks);

    hipError_t e = hipMemsetAsync(a.words, 0, kLevelWords * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(a.refs, 0, (size_t)n * 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_to_init, dim3(grid), dim3(kToBlock), 0, s, a);
    hipLaunchKernelGGL(k_to_check, dim3(grid), dim3(kToBlock), 0, s, a);
    for (uint32_t call = 0; call <= passes; call++) {
        const uint32_t last = call == passes ? 1u : 0u;
        if (call) { e = hipMemsetAsync(a.words + kLevelWord, 0, 256 * 4, s); if (e != hipSuccess) return e; }
        hipLaunchKernelGGL(k_to_depth, dim3(grid), dim3(kToBlock), 0, s, a, call, last);
        size_t tb = sortTemp;
        e = level_sort(temp, tb, a.keysIn, a.keys, a.valsIn, a.ids, (size_t)n, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_to_levels, dim3(grid), dim3(kToBlock), 0, s, a, last);
        if (last) break;
        for (uint32_t d = kMaxTreeDepth; d-- > 0;) hipLaunchKernelGGL(k_to_level, dim3(levelGrid), dim3(kToBlock), 0, s, a, d, call == 0 ? 1u : 0u);
    }
    hipLaunchKernelGGL(k_to_emit, dim3(grid), dim3(kToBlock), 0, s, a);
    hipLaunchKernelGGL(k_to_finish, dim3(1), dim3(1), 0, s, a);
    return hipGetLastError();
}

} // namespace gmupt
