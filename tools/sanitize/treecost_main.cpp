// Stand-alone driver of the host tree cost (csrc/pt_treecost.cpp) for the sanitizer runs of tools/sanitize/run.sh: the sizes around the run
// and level boundaries of the rule, with NaN / inf / inverted boxes and wrapped leaf ranges mixed in, at 1, 3 and 16 threads, which must
// agree in every bit.  CPU only; nothing here touches a device.
#include "../../gmu-path-tracer_amd/csrc/pt_treecost.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace gmupt;

static uint32_t g_state = 12345u;
static uint32_t rnd() { g_state = g_state * 1664525u + 1013904223u; return g_state >> 8; }
static float unit() { return (float)rnd() / 16777216.0f; }

int main()
{
    const uint32_t sizes[] = { 1, 2, 63, 64, 65, 255, 256, 257, 65536, 65537, 300000 };
    for (uint32_t n : sizes) {
        std::vector<gmupt_bvh_node> nodes(n);
        for (uint32_t i = 0; i < n; i++) {
            gmupt_bvh_node& nd = nodes[i];
            for (int k = 0; k < 3; k++) { nd.min[k] = unit() * 20.0f - 10.0f; nd.max[k] = nd.min[k] + unit() * 5.0f; }
            nd.isLeaf = (int32_t)(rnd() % 3u); nd.left = (int32_t)rnd(); nd.right = (int32_t)rnd();
            switch (rnd() % 16u) {
            case 0: nd.max[0] = std::numeric_limits<float>::quiet_NaN(); break;
            case 1: nd.max[1] = std::numeric_limits<float>::infinity(); break;
            case 2: nd.max[2] = nd.min[2] - 1.0f; break;
            case 3: nd.left = 10; nd.right = 3; break;
            default: break;
            }
        }
        const TcPartial one = tree_cost_host(nodes.data(), n, 1);
        for (int threads : { 3, 16 }) {
            const TcPartial t = tree_cost_host(nodes.data(), n, threads);
            if (std::memcmp(&t, &one, sizeof(t)) != 0) { std::fprintf(stderr, "treecost: %u records: %d threads differ from 1\n", n, threads); return 1; }
        }
        gmupt_tree_cost_info info{};
        tc_fill_info(one, &info);
        if (info.num_inner + info.num_leaves != n) { std::fprintf(stderr, "treecost: %u records: %u inner + %u leaves\n", n, info.num_inner, info.num_leaves); return 1; }
        std::printf("treecost %u records: sah %.17g, %u inner, %u leaves\n", n, info.sah, info.num_inner, info.num_leaves);
    }
    return 0;
}
