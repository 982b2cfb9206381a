// The host function of the motion plane (gmupt_motion_host): k_mv_resolve's pixel rule (pt_motion.hpp) on host arrays.
#include "pt_motion.hpp"

#include <cstring>

namespace gmupt {

// the caller has validated every index.  Any alignment (records are copied in and out).
void motion_host(const gmupt_hit* hits, const gmupt_aov* aov, size_t n, const gmupt_triangle* tris, const float* now, const float* prev, gmupt_motion* out)
{
    for (size_t i = 0; i < n; i++) {
        gmupt_hit h; gmupt_aov a;
        std::memcpy(&h, (const char*)hits + i * sizeof(h), sizeof(h)); std::memcpy(&a, (const char*)aov + i * sizeof(a), sizeof(a));
        float4 rec = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (h.triangle >= 0 && h.light == 0u) {
            gmupt_triangle T;
            std::memcpy(&T, (const char*)tris + (size_t)h.triangle * sizeof(T), sizeof(T));
            rec = mv_pixel(h.triangle, h.u, h.v, h.light, T.v, now, prev, mk3(a.position[0], a.position[1], a.position[2]));
        }
        std::memcpy((char*)out + i * 16, &rec, 16);
    }
}

} // namespace gmupt
