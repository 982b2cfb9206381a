// Builds the traversal tables of pt_travtables.hpp: build_trav_tables at the end of the file is the list of steps.
#include "pt_travtables.hpp"
#include "pt_refit.hpp"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>

namespace gmupt {
namespace {

std::string msg(const char* fmt, ...)
{
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    return buf;
}

struct Tree {
    const gmupt_bvh_node* nodes; size_t N;
    const gmupt_triangle* tris; size_t R;
    const float* verts;
    const gmupt_bvh_node& operator[](int32_t i) const { return nodes[(size_t)i]; }
    bool inner(int32_t i) const { return !nodes[(size_t)i].isLeaf; }
    // an empty leaf cannot be expressed by "first record + last flag": it points at the degenerate sentinel record R
    int32_t leafDesc(int32_t i) const { const gmupt_bvh_node& c = nodes[(size_t)i]; return ~(c.right > c.left ? c.left : (int32_t)R); }
};

// (half) the surface area in binary64: the usual visit-probability estimate, behind every choice of the numbering and the collapse
double area(const gmupt_bvh_node& n)
{
    const double dx = (double)n.max[0] - n.min[0], dy = (double)n.max[1] - n.min[1], dz = (double)n.max[2] - n.min[2];
    return dx * dy + dy * dz + dz * dx;
}

// Grows a set from a root: always takes the frontier entry with the largest surface area, of equal ones the lower index, until the
// frontier is empty or `cap` are taken; returns the indices in the order taken.  expand(index, push) calls push(node, index) for every
// inner node that enters the frontier with `index`.
template <class Expand>
std::vector<int32_t> grow_by_area(const Tree& t, int32_t rootNode, int32_t rootIndex, size_t cap, Expand expand)
{
    std::vector<std::pair<double, int32_t>> frontier{ { area(t[rootNode]), rootIndex } };
    std::vector<int32_t> taken;
    while (!frontier.empty() && taken.size() < cap) {
        size_t best = 0;
        for (size_t k = 1; k < frontier.size(); k++) if (frontier[k].first > frontier[best].first || (frontier[k].first == frontier[best].first && frontier[k].second < frontier[best].second)) best = k;
        const int32_t index = frontier[best].second;
        frontier.erase(frontier.begin() + (long)best);
        taken.push_back(index);
        expand(index, [&](int32_t node, int32_t idx) { frontier.push_back({ area(t[node]), idx }); });
    }
    return taken;
}

std::vector<int32_t> node_depths(const Tree& t)
{
    std::vector<int32_t> depth(t.N, 0);
    for (size_t i = 0; i < t.N; i++) if (!t.nodes[i].isLeaf) { depth[(size_t)t.nodes[i].left] = depth[i] + 1; depth[(size_t)t.nodes[i].right] = depth[i] + 1; }
    return depth;
}

// The inner nodes that the ray-cast kernels keep in LDS (the part of the tree every ray walks), in their order: grown from the root by
// surface area, or plain breadth-first (0.5 % slower on the bench scene)
std::vector<int32_t> top_nodes(const Tree& t, size_t cap, bool breadthFirst)
{
    if (!t.inner(0)) return {};
    if (!breadthFirst)
        return grow_by_area(t, 0, 0, cap, [&](int32_t v, auto push) { for (int32_t c : { t[v].left, t[v].right }) if (t.inner(c)) push(c, c); });
    std::vector<int32_t> bfs{ 0 };
    for (size_t h = 0; h < bfs.size() && bfs.size() < cap; h++)
        for (int32_t c : { t[bfs[h]].left, t[bfs[h]].right }) if (t.inner(c) && bfs.size() < cap) bfs.push_back(c);
    return bfs;
}

// Packed numbering: the top first, then the remaining inner nodes.  Every memory-side read of the ray cast is a whole 128-byte line
// (TCC_EA0_RDREQ_128B is all of TCC_EA0_RDREQ: profiles/r02_micro/fetch_size_calibration.txt), i.e. TWO 64-byte records.  With `pairing` a
// node therefore shares its line with the inner child a ray is most likely to visit next (the one with the larger surface area): that
// visit then finds its record in the cache.  Nodes without such a partner share a line with the next one of their kind in flatten order
// (usually a sibling or cousin).  Without it: plain flatten order.  Returns the number of records; one may be an unused filler.
int32_t number_inner_nodes(const Tree& t, const std::vector<int32_t>& top, bool pairing, std::vector<int32_t>& innerIndex)
{
    const size_t N = t.N;
    int32_t nextIdx = 0;
    for (int32_t v : top) innerIndex[(size_t)v] = nextIdx++;
    if (!pairing) {
        for (size_t i = 0; i < N; i++) if (!t.nodes[i].isLeaf && innerIndex[i] < 0) innerIndex[i] = nextIdx++;
        return nextIdx;
    }
    if (nextIdx & 1) nextIdx++;                                   // lines start at even records (an unused record keeps the parity)
    std::vector<int32_t> partner(N, -1), singles;
    std::vector<uint8_t> taken(N, 0);
    for (size_t i = 0; i < N; i++) {                              // parents come before their children in the reference numbering
        if (t.nodes[i].isLeaf || innerIndex[i] >= 0 || taken[i]) continue;
        const int32_t l = t.nodes[i].left, r = t.nodes[i].right;
        const bool li = t.inner(l) && innerIndex[(size_t)l] < 0, ri = t.inner(r) && innerIndex[(size_t)r] < 0;
        int32_t c = -1;
        if (li && ri) c = area(t[l]) >= area(t[r]) ? l : r; else if (li) c = l; else if (ri) c = r;
        if (c >= 0) { partner[i] = c; taken[(size_t)c] = 1; } else singles.push_back((int32_t)i);
    }
    for (size_t i = 0; i < N; i++) if (partner[i] >= 0) { innerIndex[i] = nextIdx++; innerIndex[(size_t)partner[i]] = nextIdx++; }
    for (int32_t v : singles) innerIndex[(size_t)v] = nextIdx++;
    return nextIdx;
}

std::vector<Node64> pack_nodes(const Tree& t, const std::vector<int32_t>& innerIndex, const std::vector<int32_t>& depth, int32_t numPacked)
{
    std::vector<Node64> packed((size_t)numPacked ? (size_t)numPacked : 1);
    std::memset(packed.data(), 0, packed.size() * sizeof(Node64));
    auto desc = [&](int32_t child) { return t.inner(child) ? innerIndex[(size_t)child] : t.leafDesc(child); };
    for (size_t i = 0; i < t.N; i++) {
        if (t.nodes[i].isLeaf) continue;
        const gmupt_bvh_node& L = t[t.nodes[i].left];
        const gmupt_bvh_node& Rn = t[t.nodes[i].right];
        Node64& o = packed[(size_t)innerIndex[i]];
        o.a[0] = L.min[0]; o.a[1] = L.min[1]; o.a[2] = L.min[2]; o.a[3] = L.max[0];
        o.b[0] = L.max[1]; o.b[1] = L.max[2]; o.b[2] = Rn.min[0]; o.b[3] = Rn.min[1];
        o.c[0] = Rn.min[2]; o.c[1] = Rn.max[0]; o.c[2] = Rn.max[1]; o.c[3] = Rn.max[2];
        o.d[0] = desc(t.nodes[i].left); o.d[1] = desc(t.nodes[i].right); o.d[2] = depth[i]; o.d[3] = 0;
    }
    return packed;
}

// one record per reference (the nine floats of rf_tri9, then the last-of-leaf flag), then the sentinel: an all-zero triangle (det = 0,
// rejected) with the flag set
std::vector<Tri48> pack_tris(const Tree& t)
{
    std::vector<Tri48> ptris(t.R + 1);
    std::memset(ptris.data(), 0, ptris.size() * sizeof(Tri48));
    for (size_t i = 0; i < t.R; i++) {
        float c[9];
        rf_tri9(t.tris[i], t.verts, c);
        std::memcpy(&ptris[i], c, sizeof(c));
    }
    const uint32_t one = 1u;
    for (size_t i = 0; i < t.N; i++)
        if (t.nodes[i].isLeaf && t.nodes[i].right > t.nodes[i].left) std::memcpy(&ptris[(size_t)t.nodes[i].right - 1].r2[1], &one, 4);
    std::memcpy(&ptris[t.R].r2[1], &one, 4);
    return ptris;
}

// word 10 of a triangle record: the number of the first reference with the same (v0, v1, v2, material) -- duplicated references of one
// triangle (spatial splits) produce identical hit records, so a tie in t between them is no tie (pt_traverse_wide.hip)
void first_equal_words(const Tree& t, std::vector<Tri48>& ptris)
{
    const size_t R = t.R;
    struct Key { int32_t v[3]; uint32_t mat; uint32_t idx; };
    std::vector<Key> keys(R);
    for (size_t i = 0; i < R; i++) keys[i] = { { t.tris[i].v[0], t.tris[i].v[1], t.tris[i].v[2] }, t.tris[i].materialID, (uint32_t)i };
    std::sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) {
        if (a.v[0] != b.v[0]) return a.v[0] < b.v[0];
        if (a.v[1] != b.v[1]) return a.v[1] < b.v[1];
        if (a.v[2] != b.v[2]) return a.v[2] < b.v[2];
        if (a.mat != b.mat) return a.mat < b.mat;
        return a.idx < b.idx; });
    for (size_t i = 0; i < R;) {
        size_t j = i;
        while (j < R && keys[j].v[0] == keys[i].v[0] && keys[j].v[1] == keys[i].v[1] && keys[j].v[2] == keys[i].v[2] && keys[j].mat == keys[i].mat) {
            std::memcpy(&ptris[keys[j].idx].r2[2], &keys[i].idx, 4);
            j++;
        }
        i = j;
    }
    const uint32_t none = 0xFFFFFFFFu;
    std::memcpy(&ptris[R].r2[2], &none, 4);
}

// the leaves as triangle pairs (TriPair, pt_device.hpp): consecutive references of a leaf two by two.  Returns the first pair of every leaf.
std::vector<int32_t> build_pairs(const Tree& t, const std::vector<Tri48>& ptris, std::vector<TriPair>& pairs, std::vector<uint32_t>& pairRef)
{
    std::vector<int32_t> leafPair(t.N, -1);
    pairs.reserve(t.R / 2 + t.N / 2 + 2); pairRef.reserve(t.R + t.N + 4);
    auto put = [&](TriPair& pr, int slot, size_t ref) {
        float w[9]; std::memcpy(w, &ptris[ref], sizeof(w));      // v0.xyz, e1.xyz, e2.xyz: the first nine words of the record
        for (int k = 0; k < 9; k++) pr.w[2 * k + slot] = w[k];
    };
    const uint32_t one32 = 1u;
    for (size_t i = 0; i < t.N; i++) {
        if (!t.nodes[i].isLeaf) continue;
        leafPair[i] = (int32_t)pairs.size();
        const int32_t a = t.nodes[i].left, b = t.nodes[i].right;
        for (int32_t k = a; k < b || k == a; k += 2) {          // (an empty leaf gets one all-zero pair)
            TriPair pr; std::memset(&pr, 0, sizeof(pr));
            uint32_t r0 = 0xFFFFFFFFu, r1 = 0xFFFFFFFFu;
            if (k < b) { put(pr, 0, (size_t)k); r0 = (uint32_t)k; }
            if (k + 1 < b) { put(pr, 1, (size_t)k + 1); r1 = (uint32_t)k + 1; }
            if (k + 2 >= b) std::memcpy(&pr.w[18], &one32, 4);
            const uint32_t nrefs = (k < b ? 1u : 0u) + (k + 1 < b ? 1u : 0u); std::memcpy(&pr.w[19], &nrefs, 4);   // (statistics)
            pairs.push_back(pr); pairRef.push_back(r0); pairRef.push_back(r1);
        }
    }
    return leafPair;
}

// every child box inside its parent's box (what a bounding-volume hierarchy is; the wide walk's equivalence to the binary one rests on it)
bool children_contained(const Tree& t)
{
    for (size_t i = 0; i < t.N; i++) {
        if (t.nodes[i].isLeaf) continue;
        for (int32_t c : { t.nodes[i].left, t.nodes[i].right })
            for (int k = 0; k < 3; k++)
                if (!(t[c].min[k] >= t.nodes[i].min[k] && t[c].max[k] <= t.nodes[i].max[k] && t[c].min[k] <= t[c].max[k])) return false;
    }
    return true;
}

struct Slots { int32_t s[4]; int n; int32_t bin; };    // the reference nodes in the slots of one wide node, and the node it grew from
struct Collapse {
    std::vector<Slots> created;                        // creation order (depth-first): parents before children
    std::vector<int32_t> createdOf;                    // reference node -> the wide node that grew from it
};

// 4-wide collapse: the two children of an inner node, the inner one with the largest surface area replaced by ITS children (they take its
// place, later slots shift up) until four slots are taken; every inner slot becomes a wide node in turn.
// Opening a slot drops ITS box test for the rays that reach its children.  "Child hit implies parent hit" holds for every ray unless a
// child is flat on an axis on which the parent is not, in the plane of one of the parent's faces (a ray with d = 0 on that axis that
// starts in this plane gets NaNs from the child's two planes -- no condition -- and +-inf from the parent's: a miss;
// pt_traverse_wide.hip).  Such a node keeps its own slot: rf_child_ok, the test a refit repeats on the new boxes.
Collapse collapse(const Tree& t, std::vector<uint32_t>& opened)
{
    auto opens = [&](int32_t c) {
        const gmupt_bvh_node& p = t[c];
        return rf_child_ok(p.min, p.max, t[p.left].min, t[p.left].max) && rf_child_ok(p.min, p.max, t[p.right].min, t[p.right].max);
    };
    Collapse col;
    col.createdOf.assign(t.N, -1);
    std::vector<int32_t> todo{ 0 };
    while (!todo.empty()) {
        const int32_t v = todo.back(); todo.pop_back();
        Slots w; w.bin = v; w.n = 2; w.s[0] = t[v].left; w.s[1] = t[v].right; w.s[2] = w.s[3] = -1;
        while (w.n < 4) {
            int best = -1;
            for (int k = 0; k < w.n; k++) if (t.inner(w.s[k]) && opens(w.s[k]) && (best < 0 || area(t[w.s[k]]) > area(t[w.s[best]]))) best = k;
            if (best < 0) break;
            const int32_t c = w.s[best];
            opened.push_back((uint32_t)c);
            for (int k = w.n; k > best + 1; k--) w.s[k] = w.s[k - 1];
            w.s[best] = t[c].left; w.s[best + 1] = t[c].right; w.n++;
        }
        col.createdOf[(size_t)v] = (int32_t)col.created.size();
        col.created.push_back(w);
        for (int k = w.n - 1; k >= 0; k--) if (t.inner(w.s[k])) todo.push_back(w.s[k]);
    }
    return col;
}

// numbering of the wide nodes: the LDS-resident top first (grown from the root by surface area, ties to the lower creation index), then
// creation order
std::vector<int32_t> number_wide(const Tree& t, const Collapse& col, size_t cap, uint32_t& wideTop)
{
    const std::vector<int32_t> top = grow_by_area(t, 0, 0, cap, [&](int32_t c, auto push) {
        const Slots& w = col.created[(size_t)c];
        for (int k = 0; k < w.n; k++) if (t.inner(w.s[k])) push(w.s[k], col.createdOf[(size_t)w.s[k]]);
    });
    std::vector<int32_t> number(col.created.size(), -1);
    int32_t nextW = 0;
    for (int32_t c : top) number[(size_t)c] = nextW++;
    wideTop = (uint32_t)nextW;
    for (int32_t& n : number) if (n < 0) n = nextW++;
    return number;
}

// the WNode records and, for refit, 4 * wide node + slot -> reference node
void fill_wide(const Tree& t, const Collapse& col, const std::vector<int32_t>& number, const std::vector<int32_t>& leafPair,
               const std::vector<int32_t>& depth, std::vector<WNode>& wide, std::vector<uint32_t>& wideMap)
{
    const size_t W = col.created.size();
    wide.resize(W);
    wideMap.assign(4 * W, kRfNone);
    const float qnan = std::numeric_limits<float>::quiet_NaN();
    for (size_t c = 0; c < W; c++) {
        const Slots& w = col.created[c];
        WNode& o = wide[(size_t)number[c]];
        for (int k = 0; k < 4; k++) {
            if (k < w.n) {
                const gmupt_bvh_node& b = t[w.s[k]];
                for (int a = 0; a < 3; a++) { o.p[a][k] = b.min[a]; o.p[5 - a][k] = b.max[a]; }   // rows: min x, y, z, max z, y, x
                o.link[k] = b.isLeaf ? ~leafPair[(size_t)w.s[k]] : number[(size_t)col.createdOf[(size_t)w.s[k]]];
                wideMap[4 * (size_t)number[c] + (size_t)k] = (uint32_t)w.s[k];
            } else {
                for (int a = 0; a < 6; a++) o.p[a][k] = qnan;      // never hit
                o.link[k] = (int32_t)0x80000000;
            }
        }
        o.aux[0] = depth[(size_t)w.bin]; o.aux[1] = w.n; o.aux[2] = o.aux[3] = 0;
    }
}

// most entries the inner stack of a walk can hold: every inner slot hit on every level, the deepest child visited last
uint32_t wide_stack_bound(const Tree& t, const Collapse& col)
{
    std::vector<uint32_t> occ(col.created.size(), 0);
    for (size_t c = col.created.size(); c-- > 0;) {
        const Slots& w = col.created[c];
        uint32_t inner = 0, deepest = 0;
        for (int k = 0; k < w.n; k++) if (t.inner(w.s[k])) { inner++; deepest = std::max(deepest, occ[(size_t)col.createdOf[(size_t)w.s[k]]]); }
        occ[c] = inner ? inner - 1 + deepest : 0;
    }
    return occ[0];
}

// inner nodes by height (a leaf has height 0), lowest first: every node comes after its children, whatever the shape of the tree.
// `height` comes in as the depths, which nothing needs any more, and is overwritten.
void level_lists(const Tree& t, std::vector<int32_t>& height, std::vector<uint32_t>& levelNodes, std::vector<uint32_t>& levelOff)
{
    const size_t N = t.N;
    int32_t top = 0;
    for (size_t i = N; i-- > 0;) { height[i] = t.nodes[i].isLeaf ? 0 : 1 + std::max(height[(size_t)t.nodes[i].left], height[(size_t)t.nodes[i].right]); top = std::max(top, height[i]); }
    levelOff.assign((size_t)top + 1, 0);
    for (size_t i = 0; i < N; i++) if (height[i] > 0) levelOff[(size_t)height[i]]++;
    for (size_t h = 1; h <= (size_t)top; h++) levelOff[h] += levelOff[h - 1];    // levelOff[h] = end of height h
    levelNodes.resize(levelOff[(size_t)top]);
    std::vector<uint32_t> at(levelOff.begin(), levelOff.end());
    for (size_t i = N; i-- > 0;) if (height[i] > 0) levelNodes[--at[(size_t)height[i]]] = (uint32_t)i;
}

#ifdef GMUPT_VARIANTS
// unified 64-byte records for the cooperative kernels (rungs of the test build only)
std::vector<Rec64> unified_records(const Tree& t, const std::vector<Node64>& packed, const std::vector<Tri48>& ptris)
{
    std::vector<Rec64> recs(packed.size() + ptris.size());
    std::memset(recs.data(), 0, recs.size() * sizeof(Rec64));
    for (size_t i = 0; i < packed.size(); i++) std::memcpy(&recs[i], &packed[i], 64);
    for (size_t i = 0; i < ptris.size(); i++) {
        std::memcpy(&recs[packed.size() + i], &ptris[i], 48);
        if (i < t.R) std::memcpy(&recs[packed.size() + i].q[12], &t.tris[i], 16); // (v0, v1, v2, materialID)
    }
    return recs;
}
#endif

} // namespace

// what the kernels will index with: a malformed tree must not become an out-of-bounds access on the GPU
std::string validate_tree(const char* prefix, const gmupt_bvh_node* nodes, size_t N, const gmupt_triangle* tris, size_t R, size_t V, uint32_t materialLimit)
{
    for (size_t i = 0; i < N; i++) {
        const gmupt_bvh_node& n = nodes[i];
        if (n.isLeaf) {
            if (n.left < 0 || n.right < n.left || (size_t)n.right > R) return msg("%s: leaf %zu has triangle range [%d, %d) outside [0, %zu)", prefix, i, n.left, n.right, R);
        } else if (n.left <= (int32_t)i || n.right <= (int32_t)i || (size_t)n.left >= N || (size_t)n.right >= N) {
            return msg("%s: inner node %zu has children (%d, %d) outside (%zu, %zu)", prefix, i, n.left, n.right, i, N);
        }
    }
    for (size_t i = 0; i < R; i++) {
        for (int k = 0; k < 3; k++)
            if (tris[i].v[k] < 0 || (size_t)tris[i].v[k] >= V) return msg("%s: triangle record %zu references vertex %d of %zu", prefix, i, tris[i].v[k], V);
        if (materialLimit && tris[i].materialID >= materialLimit) return msg("%s: triangle record %zu has material %u (the material table holds %u entries, logic.hlsl:8)", prefix, i, tris[i].materialID, materialLimit);
    }
    return std::string();
}

std::string build_trav_tables(const gmupt_bvh_node* nodes, size_t N, const gmupt_triangle* tris, size_t R, const float* verts, size_t V,
                              const TravOptions& opt, TravTables& out)
{
    const std::string err = validate_tree("bind_scene", nodes, N, tris, R, V, (uint32_t)GMUPT_MAX_LIGHTS);
    if (!err.empty()) return err;
    const Tree t{ nodes, N, tris, R, verts };
    out = TravTables();
    TravScalars& s = out.s;

    std::vector<int32_t> depth = node_depths(t);
    s.maxDepth = (uint32_t)*std::max_element(depth.begin(), depth.end());
    // how many nodes fit the LDS depends on the kernel instantiation this tree will run: a tree that needs the spilling stack keeps fewer
    // stack entries and more nodes there (pt_traverse_deferred.hpp: kDefLdsStack / kDefLdsTop); one numbering serves both as a prefix
    const std::vector<int32_t> top = top_nodes(t, opt.topCapacity(s.maxDepth), opt.topOrderBfs);
    s.topCountDeep = (uint32_t)top.size();
    s.topCount = (uint32_t)std::min(top.size(), (size_t)kTopTreeNodes);
    std::vector<int32_t> innerIndex(N, -1);
    const int32_t numPacked = number_inner_nodes(t, top, opt.nodePairing, innerIndex);

    out.nodes = pack_nodes(t, innerIndex, depth, numPacked);
    out.tris = pack_tris(t);
    s.triBase = (uint32_t)out.nodes.size();
    s.rootDesc = t.inner(0) ? innerIndex[0] : t.leafDesc(0);
    for (int k = 0; k < 3; k++) { s.rootMin[k] = nodes[0].min[k]; s.rootMax[k] = nodes[0].max[k]; }
    out.nodeMap.assign(out.nodes.size(), kRfNone);
    for (size_t i = 0; i < N; i++) if (!nodes[i].isLeaf) out.nodeMap[(size_t)innerIndex[i]] = (uint32_t)i;

    if (opt.wantWide) {
        first_equal_words(t, out.tris);
        const std::vector<int32_t> leafPair = build_pairs(t, out.tris, out.pairs, out.pairRef);
        s.numPairs = (uint32_t)out.pairs.size();
        if (children_contained(t) && t.inner(0)) {
            const Collapse col = collapse(t, out.opened);
            const std::vector<int32_t> number = number_wide(t, col, opt.wideTopCapacity, s.wideTopCount);
            fill_wide(t, col, number, leafPair, depth, out.wide, out.wideMap);
            s.wideStackBound = wide_stack_bound(t, col);
            s.wideCount = (uint32_t)out.wide.size();
        }
    }
#ifdef GMUPT_VARIANTS
    out.recs = unified_records(t, out.nodes, out.tris);
#endif
    level_lists(t, depth, out.levelNodes, out.levelOff);   // (takes the depths' storage: last)
    return std::string();
}

bool wide_tables_addressable(uint32_t wideCount, uint32_t numTris, uint32_t numPairs)
{
    constexpr uint64_t kLimit = 1ull << 31;
    return (uint64_t)wideCount * sizeof(WNode) < kLimit && ((uint64_t)numTris + 1ull) * sizeof(Tri48) < kLimit && (uint64_t)numPairs * sizeof(TriPair) < kLimit;
}

} // namespace gmupt
