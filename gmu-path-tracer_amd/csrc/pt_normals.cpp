// gmupt_vertex_normals_host: the rule of include/gmupt.h ("Normals") on host arrays, the reference of the device path (pt_normals.hip).
// The arithmetic is pt_normals.hpp, shared with the kernels.  A loop over the corners in ascending number that adds each corner's face
// vector to its vertex IS the summation order of the rule; with threads, every thread runs that loop over all corners and keeps the
// vertices of its own band, so the order per vertex -- and with it every bit of the result -- does not depend on the thread count.
#include "pt_normals.hpp"
#include "pt_bands.hpp"

#include <algorithm>
#include <vector>

namespace gmupt {

void normals_host(const float* verts, uint32_t numVerts, const int32_t* indices, uint32_t numTris, float* normalsOut, int threads)
{
    constexpr size_t kChunk = 4096;
    const size_t V = numVerts, T = numTris;
    std::vector<float> faces(3 * T);
    host_bands((int)((T + kChunk - 1) / kChunk), threads, [&](int c0, int c1) {
        for (size_t t = (size_t)c0 * kChunk; t < std::min(T, (size_t)c1 * kChunk); t++) {
            const int32_t* i = indices + 3 * t;
            nm_face(verts + 3 * (size_t)i[0], verts + 3 * (size_t)i[1], verts + 3 * (size_t)i[2], &faces[3 * t]);
        }
    });
    host_bands((int)((V + kChunk - 1) / kChunk), threads, [&](int c0, int c1) {
        const size_t v0 = (size_t)c0 * kChunk, v1 = std::min(V, (size_t)c1 * kChunk);
        std::vector<float> sum(3 * (v1 - v0), 0.0f);
        for (size_t c = 0; c < 3 * T; c++) {
            const size_t v = (size_t)indices[c];
            if (v < v0 || v >= v1) continue;
            const float* f = &faces[3 * (c / 3)];
            float* s = &sum[3 * (v - v0)];
            s[0] = s[0] + f[0]; s[1] = s[1] + f[1]; s[2] = s[2] + f[2];
        }
        for (size_t v = v0; v < v1; v++) nm_finish(&sum[3 * (v - v0)], normalsOut + 3 * v);
    });
}

} // namespace gmupt
