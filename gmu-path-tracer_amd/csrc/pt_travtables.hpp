// The traversal tables of a bound scene (record layouts: pt_device.hpp), built on the host from the reference-layout tree.  Pure host
// code: no device, no environment, no renderer.  gmupt_renderer_bind_scene uploads what this returns; a refit (pt_refit.hip) rewrites
// the same records in place through the maps, so the builder and the k_rf_* kernels share the rules of pt_refit.hpp.
#pragma once
#include "pt_device.hpp"
#include <string>
#include <vector>

namespace gmupt {

struct TravOptions {
    bool wantWide = true;          // build the 4-wide collapse, the triangle pairs and the first-equal-reference words
    bool topOrderBfs = false;      // LDS-resident top of the binary tree in breadth-first order instead of largest surface area first
    bool nodePairing = true;       // inner nodes below the top numbered so that a node shares its 128-byte line with its likelier inner child
    uint32_t (*topCapacity)(uint32_t maxDepth) = nullptr;   // Node64 records the ray-cast kernels keep in LDS for a tree of that depth
    uint32_t wideTopCapacity = 0;                           // WNode records the wide ray cast keeps in LDS
};

// what goes into TravScene besides the table pointers
struct TravScalars {
    uint32_t topCount, topCountDeep, maxDepth;
    int32_t rootDesc;
    float rootMin[3], rootMax[3];
    uint32_t triBase, wideTopCount, wideStackBound, numPairs, wideCount;
};

struct TravTables {
    std::vector<Node64> nodes;        // inner nodes in packed numbering (a filler record may keep the line parity)
    std::vector<Tri48> tris;          // one per reference, then the sentinel record of the empty leaves
    std::vector<TriPair> pairs;       // the leaves two references at a time; pairRef: 2 per pair, the reference in that slot
    std::vector<uint32_t> pairRef;
    std::vector<WNode> wide;          // empty: no wide copy (not wanted, the root is a leaf, or a child box sticks out of its parent's)
#ifdef GMUPT_VARIANTS
    std::vector<Rec64> recs;          // nodes, then tris with the reference's gmupt_triangle in the last quarter
#endif
    TravScalars s{};
    // refit maps: inner nodes by height, lowest first (levelOff[h] = end of height h); packed index -> reference node; 4 * wide node +
    // slot -> reference node; the nodes whose slot the collapse replaced by their children.  kRfNone names no node.
    std::vector<uint32_t> levelNodes, levelOff, nodeMap, wideMap, opened;
};

// "" for a tree the kernels can index with; otherwise the message, starting with `prefix`.  materialLimit != 0 also bounds the material ids.
std::string validate_tree(const char* prefix, const gmupt_bvh_node* nodes, size_t N, const gmupt_triangle* tris, size_t R, size_t V, uint32_t materialLimit);

// "" on success; the message of validate_tree("bind_scene", ...) on a malformed tree, `out` then holds nothing of use
std::string build_trav_tables(const gmupt_bvh_node* nodes, size_t N, const gmupt_triangle* tris, size_t R, const float* verts, size_t V,
                              const TravOptions& opt, TravTables& out);

// The wide ray cast (k_cast_w) addresses its three tables with signed 32-bit byte offsets: WNode records (128 bytes), Tri48 records and
// their sentinel (48 bytes), TriPair records (80 bytes).  True when every table stays below 2 GiB; otherwise the renderer's own cast falls
// back to the binary-tree kernels and the ray queries return GMUPT_ERR_UNSUPPORTED.
bool wide_tables_addressable(uint32_t wideCount, uint32_t numTris, uint32_t numPairs);

} // namespace gmupt
