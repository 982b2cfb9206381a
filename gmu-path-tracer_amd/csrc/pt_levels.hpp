// The level step of the tree stages (pt_lbvh.hip, pt_treeopt.hip): the ids of a tree sorted by (depth, a caller's number), and where each
// depth starts in that order, so that a level is one launch over a range read from device memory.  A caller's depth kernel writes
// level_key() per id, level_sort() orders (key, id), and its levels kernel calls level_offsets() per sorted entry.
#pragma once
#include "detmath.hpp"
#include "pt_scratch.hpp"

#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>

namespace gmupt {

// the device words of a stage: the first kLevelWord are the stage's own, then levelOff[256] -- the nodes of depth d are the sorted
// positions [levelOff[d], levelOff[d + 1]), an absent depth is an empty range
constexpr uint32_t kLevelWord = 32, kLevelWords = kLevelWord + 256;
constexpr uint32_t kLevelDropped = 255u;         // depth byte of an entry that is not part of the order (a depth is at most 128: level_depth)

// all ones for an entry that is left out of the order: it sorts behind every other
GM_HD uint64_t level_key(bool kept, uint32_t depth, uint32_t x) { return kept ? ((uint64_t)depth << 32) | x : ~0ull; }
GM_HD uint32_t level_key_depth(uint64_t key) { return (uint32_t)(key >> 32) & 0xFFu; }

// the depth of a node whose parent is p: the links are followed while they name an id in [0, limit), 128 steps at the most
__device__ __forceinline__ uint32_t level_depth(const int32_t* parent, int32_t p, uint32_t limit)
{
    uint32_t depth = 0;
    for (; p >= 0 && (uint32_t)p < limit && depth < 128u; p = parent[p]) depth++;
    return depth;
}

// the sort of (level_key, id) over `count` entries; temp = nullptr asks for the bytes of temporary storage
inline hipError_t level_sort(void* temp, size_t& tempBytes, uint64_t* keysIn, uint64_t* keys, uint32_t* idsIn, uint32_t* ids, size_t count, hipStream_t s)
{
    return rocprim::radix_sort_pairs(temp, tempBytes, keysIn, keys, idsIn, ids, count, 0u, 40u, s);
}
inline hipError_t level_sort_temp_bytes(size_t count, size_t* bytes)
{
    size_t b = 0;
    const hipError_t e = level_sort(nullptr, b, nullptr, nullptr, nullptr, nullptr, count, (hipStream_t)0);
    *bytes = scratch_align(std::max(b, (size_t)256));
    return e;
}

// What sorted entry `pos` of M says about the order: its depth byte, and -- at the one entry where the order ends -- how many entries
// the order holds and its largest depth (count = 0 everywhere else).
struct LevelEntry { uint32_t depth, count, last; };

// one thread per sorted entry: writes where each depth starts, and the end of the last one
__device__ __forceinline__ LevelEntry level_offsets(const uint64_t* keys, size_t pos, size_t M, uint32_t* levelOff)
{
    LevelEntry r = { level_key_depth(keys[pos]), 0u, 0u };
    const uint32_t dprev = pos ? level_key_depth(keys[pos - 1]) : kLevelDropped;
    if (r.depth != kLevelDropped) {
        if (pos == 0 || r.depth != dprev) levelOff[r.depth] = (uint32_t)pos;
        if (pos == M - 1) { r.count = (uint32_t)M; r.last = r.depth; levelOff[r.depth + 1] = (uint32_t)M; }
    } else if (pos && dprev != kLevelDropped) {
        r.count = (uint32_t)pos; r.last = dprev; levelOff[dprev + 1] = (uint32_t)pos;
    }
    return r;
}

} // namespace gmupt
