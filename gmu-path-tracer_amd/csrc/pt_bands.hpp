// What the host rules (pt_*.cpp) share: the bands a rule's rows, chunks or runs are handed out in, and the aligned copy of a caller's array.
#pragma once
#include "detmath.hpp"

#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

namespace gmupt {

// fn(y0, y1) over bands of H rows on up to `threads` std::threads
template <class F> void host_bands(int H, int threads, const F& fn)
{
    threads = std::max(1, std::min(threads, H));
    if (threads == 1) { fn(0, H); return; }
    const int per = (H + threads - 1) / threads;
    std::vector<std::thread> pool;
    pool.reserve((size_t)threads);
    int y0 = 0;
    try {
        for (; y0 < H; y0 += per) pool.emplace_back([&fn, y0, per, H]() { fn(y0, std::min(H, y0 + per)); });
    } catch (...) {
        // a thread could not be started: the bands not yet handed out run here (the bands never depend on who computes them)
        for (; y0 < H; y0 += per) fn(y0, std::min(H, y0 + per));
    }
    for (std::thread& t : pool) t.join();
}

// a caller's array of n 16-byte words, at any alignment, as aligned float4; a null array gives none
inline std::vector<float4> host_words(const void* src, size_t n)
{
    std::vector<float4> v(src ? n : 0);
    if (!v.empty()) std::memcpy(v.data(), src, n * 16);
    return v;
}

} // namespace gmupt
