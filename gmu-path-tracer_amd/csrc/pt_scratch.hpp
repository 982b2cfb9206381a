// The scratch of a device stage as one allocation: a cursor that hands out typed parts, each at a 256-byte boundary.  A stage has one
// function that takes its parts in a fixed order; run over a null base it only adds up the bytes (how the allocation is sized), run
// over the allocation it yields the pointers of a launch.  The parts are taken for a handle's capacity: a smaller input uses the front
// of each.  Also the grid of a one-thread-per-item launch.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gmupt {

inline size_t scratch_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
inline uint32_t grid_for(size_t n, uint32_t block) { return (uint32_t)((n + block - 1) / block); }

struct Scratch {
    char* base; size_t used = 0;                   // used: the bytes taken so far, the size of the allocation after the last part
    explicit Scratch(void* b) : base(static_cast<char*>(b)) {}
    template <class T> T* take(size_t count)
    {
        T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += scratch_align(count * sizeof(T));
        return p;
    }
};

} // namespace gmupt
