// A stand-alone host program for a sanitizer build of the treelet optimiser's host reference (csrc/pt_treeopt.cpp): a few crafted trees
// through gmupt::tree_optimize_host, the accepted ones checked for structure, the refused ones for untouched outputs.  run.sh builds and
// runs it (the host side of hipcc: the headers are HIP headers; no device code is built or run).
#include "../../gmu-path-tracer_amd/csrc/pt_treeopt.hpp"

#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using namespace gmupt;

// a random binary tree over `leaves` leaves, numbered breadth first (children above their parent), boxes by union
static std::vector<gmupt_bvh_node> random_tree(uint32_t leaves, uint32_t seed, bool chain)
{
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> pos(-10.0f, 10.0f), ext(0.0f, 2.0f);
    struct Item { uint32_t leaves; };
    std::vector<gmupt_bvh_node> nodes(1);
    std::vector<Item> todo(1, Item{ leaves });
    std::memset(nodes.data(), 0, sizeof(gmupt_bvh_node));
    uint32_t nextRef = 0;
    for (size_t i = 0; i < nodes.size(); i++) {
        const uint32_t n = todo[i].leaves;
        if (n == 1) {
            nodes[i].isLeaf = 1; nodes[i].left = (int32_t)nextRef; nextRef += 1 + rng() % 4; nodes[i].right = (int32_t)nextRef;
            for (int k = 0; k < 3; k++) { nodes[i].min[k] = pos(rng); nodes[i].max[k] = nodes[i].min[k] + (seed % 3 == 0 && k == 1 ? 0.0f : ext(rng)); }
            continue;
        }
        const uint32_t l = chain ? 1u : 1u + rng() % (n - 1);
        nodes[i].left = (int32_t)nodes.size(); nodes[i].right = nodes[i].left + 1;
        gmupt_bvh_node z; std::memset(&z, 0, sizeof(z));
        nodes.push_back(z); nodes.push_back(z);
        todo.push_back(Item{ l }); todo.push_back(Item{ n - l });
    }
    for (size_t i = nodes.size(); i-- > 0;)
        if (!nodes[i].isLeaf) {
            const RfBox b = rf_union(nodes[nodes[i].left].min, nodes[nodes[i].left].max, nodes[nodes[i].right].min, nodes[nodes[i].right].max);
            for (int k = 0; k < 3; k++) { nodes[i].min[k] = b.mn[k]; nodes[i].max[k] = b.mx[k]; }
        }
    return nodes;
}

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

int main()
{
    const struct { uint32_t leaves, seed; bool chain; int want; } cases[] = {
        { 1, 1, false, GMUPT_OK }, { 2, 2, false, GMUPT_OK }, { 3, 3, false, GMUPT_OK }, { 7, 4, false, GMUPT_OK }, { 8, 5, false, GMUPT_OK },
        { 37, 6, false, GMUPT_OK }, { 500, 7, false, GMUPT_OK }, { 65, 8, true, GMUPT_OK }, { 67, 9, true, GMUPT_ERR_UNSUPPORTED }, { 3000, 10, false, GMUPT_OK },
    };
    for (const auto& c : cases)
        for (uint32_t passes = 1; passes <= 3; passes++) {
            const std::vector<gmupt_bvh_node> in = random_tree(c.leaves, c.seed, c.chain);
            std::vector<gmupt_bvh_node> out(in.size());
            std::memset(out.data(), 0x5A, out.size() * sizeof(gmupt_bvh_node));
            const std::vector<gmupt_bvh_node> keep = out;
            ToResult res{};
            int status = 1;
            const std::string err = tree_optimize_host(in.data(), (uint32_t)in.size(), passes, out.data(), res, &status);
            CHECK(status == c.want);
            if (status != GMUPT_OK) { CHECK(!err.empty() && std::memcmp(out.data(), keep.data(), out.size() * sizeof(gmupt_bvh_node)) == 0); continue; }
            CHECK(res.costAfter <= res.costBefore && res.depthAfter <= kMaxTreeDepth && res.numNodes == in.size());
            uint32_t leaves = 0;
            for (size_t i = 0; i < out.size(); i++) {
                if (out[i].isLeaf) { leaves++; continue; }
                CHECK(out[i].left > (int32_t)i && out[i].right > (int32_t)i && (size_t)out[i].left < out.size() && (size_t)out[i].right < out.size());
            }
            CHECK(leaves == c.leaves);
            std::printf("%u leaves, %u passes: depth %u -> %u, %u treelets rewritten, cost %.6g -> %.6g\n", c.leaves, passes, res.depthBefore, res.depthAfter,
                        res.rewritten, res.costBefore, res.costAfter);
        }
    // a link at its own node, and a child shared by two nodes
    std::vector<gmupt_bvh_node> bad = random_tree(9, 11, false), out(bad.size());
    ToResult res{};
    int status = 1;
    bad[0].right = 0;
    tree_optimize_host(bad.data(), (uint32_t)bad.size(), 2, out.data(), res, &status);
    CHECK(status == GMUPT_ERR_INVALID_ARGUMENT);
    bad = random_tree(9, 11, false);
    bad[0].right = bad[0].left;
    tree_optimize_host(bad.data(), (uint32_t)bad.size(), 2, out.data(), res, &status);
    CHECK(status == GMUPT_ERR_INVALID_ARGUMENT);
    std::printf(failures ? "%d checks failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
