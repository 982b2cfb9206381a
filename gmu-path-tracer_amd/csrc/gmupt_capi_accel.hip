// C-ABI of libgmupt.so: the traversal tables of a bound scene (upload, refit, debug reads) and the LBVH builder handle.
#include "gmupt_work.hpp"

// GMUPT_TOP_ORDER=bfs and GMUPT_NODE_PAIRING=0 are A/B switches of the numbering (pt_travtables.cpp); results do not depend on them
static TravOptions trav_options(bool wantWide, bool topOrderBfs, bool nodePairing)
{
    TravOptions o;
    o.wantWide = wantWide; o.topOrderBfs = topOrderBfs; o.nodePairing = nodePairing;
    o.topCapacity = traversal_top_capacity; o.wideTopCapacity = traversal_wide_top_capacity();
    return o;
}

// Downloads the bound tree, has pt_travtables.cpp build the traversal tables, uploads them.  Once per bind (and per refit that rebuilds).
// The renderer changes over after the last upload (until then both sets exist): a failure leaves it on the tables, TravScene and refit maps it had.
int build_traversal_copy(gmupt_renderer* r, const gmupt_buffer* nodesB, const gmupt_buffer* trisB, const gmupt_buffer* vertsB)
{
    HIP_TRY(hipSetDevice(r->dev->id));
    HIP_TRY(hipStreamSynchronize(r->stream));
    const size_t N = nodesB->elems, R = trisB->elems, V = vertsB->elems;
    std::vector<gmupt_bvh_node> nodes(N);
    std::vector<gmupt_triangle> tris(R ? R : 1);
    std::vector<float> verts(V ? V * 3 : 3);
    HIP_TRY(hipMemcpy(nodes.data(), nodesB->dptr, N * sizeof(gmupt_bvh_node), hipMemcpyDeviceToHost));
    if (R) HIP_TRY(hipMemcpy(tris.data(), trisB->dptr, R * sizeof(gmupt_triangle), hipMemcpyDeviceToHost));
    if (V) HIP_TRY(hipMemcpy(verts.data(), vertsB->dptr, V * 12, hipMemcpyDeviceToHost));

    // nothing of the renderer or on the device is touched before the tables exist
    TravTables tt;
    const char* order = std::getenv("GMUPT_TOP_ORDER");
    const char* pairing = std::getenv("GMUPT_NODE_PAIRING");
    const std::string err = build_trav_tables(nodes.data(), N, tris.data(), R, verts.data(), V,
                                              trav_options(r->travMode == 70, order && std::strcmp(order, "bfs") == 0, !(pairing && std::atoi(pairing) == 0)), tt);
    if (!err.empty()) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s", err.c_str());

    const bool haveWide = !tt.wide.empty();   // without a wide copy the pairs stay on the host
    const void* recs = nullptr; size_t recBytes = 0;
#ifdef GMUPT_VARIANTS
    recs = tt.recs.data(); recBytes = tt.recs.size() * sizeof(Rec64);
#endif
    const struct { const void* data; size_t bytes; } up[TT_COUNT] = {      // in the order of TravTable
        { tt.nodes.data(), tt.nodes.size() * sizeof(Node64) }, { tt.tris.data(), tt.tris.size() * sizeof(Tri48) }, { recs, recBytes },
        { tt.wide.data(), tt.wide.size() * sizeof(WNode) }, { tt.pairs.data(), haveWide ? tt.pairs.size() * sizeof(TriPair) : 0 },
        { tt.pairRef.data(), haveWide ? tt.pairRef.size() * 4 : 0 } };
    DevMem fresh[TT_COUNT];
    for (int k = 0; k < TT_COUNT; k++) {
        if (!up[k].bytes) continue;
        GMUPT_TRY(fresh[k].grow(r->stream, up[k].bytes));
        HIP_TRY(hipMemcpy(fresh[k].ptr, up[k].data, up[k].bytes, hipMemcpyHostToDevice));
    }
    for (int k = 0; k < TT_COUNT; k++) r->trav[k] = std::move(fresh[k]);    // the old tables end with `fresh`: the stream was synchronised above
    TravScene& t = r->p.trav;
    t.recs = r->trav[TT_RECS].as<const Rec64>(); t.nodes = r->trav[TT_NODES].as<const Node64>(); t.tris = r->trav[TT_TRIS].as<const Tri48>();
    t.wnodes = r->trav[TT_WIDE].as<const WNode>(); t.pairs = r->trav[TT_PAIRS].as<const TriPair>(); t.pairRef = r->trav[TT_PAIRREF].as<const uint32_t>();
    t.triBase = tt.s.triBase; t.rootDesc = tt.s.rootDesc; t.topCount = tt.s.topCount; t.topCountDeep = tt.s.topCountDeep; t.maxDepth = tt.s.maxDepth;
    for (int k = 0; k < 3; k++) { t.rootMin[k] = tt.s.rootMin[k]; t.rootMax[k] = tt.s.rootMax[k]; }
    t.wideCount = tt.s.wideCount; t.wideTopCount = tt.s.wideTopCount; t.wideStackBound = tt.s.wideStackBound; t.wideRootDesc = 0; t.numPairs = tt.s.numPairs;

    // what a refit needs to rewrite these tables in place (host vectors; the first gmupt_renderer_refit uploads them)
    r->rfDev = DevMem();
    r->rfLevelNodes.swap(tt.levelNodes); r->rfLevelOff.swap(tt.levelOff); r->rfNodeMap.swap(tt.nodeMap); r->rfWideMap.swap(tt.wideMap); r->rfOpened.swap(tt.opened);
    r->boundNodes = nodesB; r->boundTris = trisB; r->boundVerts = vertsB;
    r->boundElems[0] = N; r->boundElems[1] = R; r->boundElems[2] = V;
    return GMUPT_OK;
}

static_assert(sizeof(gmupt_refit_info) == 24 && offsetof(gmupt_refit_info, ms) == 16, "gmupt_refit_info layout");

extern "C" int gmupt_renderer_refit(gmupt_renderer* r, gmupt_refit_info* info)
{
    if (!r) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_refit: null renderer");
    if (info) *info = gmupt_refit_info{};
    if (!r->sceneBound) return fail(GMUPT_ERR_NOT_BOUND, "gmupt_renderer_refit: no scene bound");
    if (r->boundNodes->elems != r->boundElems[0] || r->boundTris->elems != r->boundElems[1] || r->boundVerts->elems != r->boundElems[2])
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_refit: the bound buffers hold (%zu, %zu, %zu) nodes / triangle records / vertices, at bind time (%zu, %zu, %zu)",
                    r->boundNodes->elems, r->boundTris->elems, r->boundVerts->elems, r->boundElems[0], r->boundElems[1], r->boundElems[2]);
    HIP_TRY(hipSetDevice(r->dev->id));
    HIP_TRY(hipStreamSynchronize(r->stream));
    // one allocation: 16 words of flags and results, then the maps (each starts at a multiple of 16 bytes)
    const std::vector<uint32_t>* maps[4] = { &r->rfLevelNodes, &r->rfNodeMap, &r->rfWideMap, &r->rfOpened };
    size_t off[4], words = 16;
    for (int k = 0; k < 4; k++) { off[k] = words; words += (maps[k]->size() + 3) & ~(size_t)3; }
    if (!r->rfDev.ptr) {
        GMUPT_TRY(r->rfDev.grow(r->stream, words * 4));
        for (int k = 0; k < 4; k++)
            if (!maps[k]->empty()) HIP_TRY(hipMemcpy(r->rfDev.as<uint32_t>() + off[k], maps[k]->data(), maps[k]->size() * 4, hipMemcpyHostToDevice));
    }
    uint32_t* dev = r->rfDev.as<uint32_t>();
    const TravScene& t = r->p.trav;
    RfArgs a{};
    a.nodes = (DNode*)r->boundNodes->dptr; a.tris = (const gmupt_triangle*)r->boundTris->dptr; a.verts = (const float*)r->boundVerts->dptr;
    a.numNodes = (uint32_t)r->boundElems[0]; a.numTris = (uint32_t)r->boundElems[1]; a.numVerts = (uint32_t)r->boundElems[2];
    a.levelNodes = dev + off[0];
    a.ttris = r->trav[TT_TRIS].as<Tri48>(); a.pairs = r->trav[TT_PAIRS].as<TriPair>(); a.pairRef = t.pairRef; a.numPairs = t.numPairs;
    a.tnodes = r->trav[TT_NODES].as<Node64>(); a.nodeMap = dev + off[1]; a.numPacked = (uint32_t)r->rfNodeMap.size();
    a.wnodes = r->trav[TT_WIDE].as<WNode>(); a.wideMap = dev + off[2]; a.wideCount = a.wnodes ? t.wideCount : 0u;
    a.opened = dev + off[3]; a.numOpened = a.wnodes ? (uint32_t)r->rfOpened.size() : 0u;
    a.flags = dev;

    uint32_t back[16] = { 0 };
    HIP_TRY(hipMemsetAsync(dev, 0, 64, r->stream));
    launch_refit_check(a, r->stream);
    HIP_TRY(hipGetLastError());
    GMUPT_TRY(copy_sync(back, dev, 4, hipMemcpyDeviceToHost, r->stream));
    if (back[0] & kRfFlagBadIndex) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_refit: a triangle record references a vertex outside the vertex buffer (the triangle records changed since bind)");
    if (back[0] & kRfFlagNonFinite) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_renderer_refit: a vertex used by a triangle record is not finite; nothing was written");

    uint32_t reason = 0;
#ifdef GMUPT_VARIANTS
    reason = GMUPT_REFIT_VARIANTS_BUILD;
#endif
    GMUPT_TRY(r->rfEv.start(r->stream));
    const uint32_t levels = launch_refit_boxes(a, r->rfLevelOff, r->stream);
    if (!reason) launch_refit_tables(a, r->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(dev + 4, a.nodes, 32, hipMemcpyDeviceToDevice, r->stream));      // the root box next to the flags
    GMUPT_TRY(r->rfEv.stop(r->stream));
    GMUPT_TRY(copy_sync(back, dev, 64, hipMemcpyDeviceToHost, r->stream));
    float ms = 0.0f;
    GMUPT_TRY(r->rfEv.elapsed_ms(&ms));
    if (back[1]) reason |= GMUPT_REFIT_FLAT_CHILD;
    const uint32_t openedNodes = a.numOpened;
    if (reason) {
        GMUPT_TRY(build_traversal_copy(r, r->boundNodes, r->boundTris, r->boundVerts));
    } else {
        for (int k = 0; k < 3; k++) { std::memcpy(&r->p.trav.rootMin[k], &back[4 + k], 4); std::memcpy(&r->p.trav.rootMax[k], &back[8 + k], 4); }
    }
    r->geomGeneration++;
    if (info) { info->rebuilt = reason ? 1u : 0u; info->reason = reason; info->levels = levels; info->opened_nodes = openedNodes; info->ms = (double)ms; }
    return GMUPT_OK;
}

extern "C" int gmupt_debug_travtables_build(const gmupt_bvh_node* nodes, uint32_t num_nodes, const gmupt_triangle* tris, uint32_t num_tris,
                                            const float* verts, uint32_t num_verts, int want_wide, int top_order_bfs, int node_pairing, gmupt_travtables** out)
{
    if (!out || !nodes || num_nodes == 0 || (!tris && num_tris) || (!verts && num_verts)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_travtables_build: null or empty array");
    *out = nullptr;
    gmupt_travtables* h = new (std::nothrow) gmupt_travtables();
    if (!h) return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_debug_travtables_build: out of host memory");
    const std::string err = build_trav_tables(nodes, num_nodes, tris, num_tris, verts, num_verts, trav_options(want_wide != 0, top_order_bfs != 0, node_pairing != 0), h->t);
    if (!err.empty()) { delete h; return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s", err.c_str()); }
    *out = h;
    return GMUPT_OK;
}

extern "C" const void* gmupt_debug_travtables_data(const gmupt_travtables* h, int which, size_t* bytes)
{
    if (!h || !bytes) return nullptr;
    const TravTables& t = h->t;
    auto of = [&](const auto& v) -> const void* { *bytes = v.size() * sizeof(v[0]); return v.data(); };
    switch (which) {
    case GMUPT_TT_NODE64: return of(t.nodes); case GMUPT_TT_TRI48: return of(t.tris); case GMUPT_TT_TRIPAIR: return of(t.pairs);
    case GMUPT_TT_PAIRREF: return of(t.pairRef); case GMUPT_TT_WNODE: return of(t.wide);
#ifdef GMUPT_VARIANTS
    case GMUPT_TT_REC64: return of(t.recs);
#endif
    case GMUPT_TT_SCALARS: *bytes = sizeof(TravScalars); return &t.s;
    case GMUPT_TT_LEVEL_NODES: return of(t.levelNodes); case GMUPT_TT_LEVEL_OFF: return of(t.levelOff); case GMUPT_TT_NODE_MAP: return of(t.nodeMap);
    case GMUPT_TT_WIDE_MAP: return of(t.wideMap); case GMUPT_TT_OPENED: return of(t.opened);
    }
    *bytes = 0;
    return nullptr;
}

extern "C" void gmupt_debug_travtables_destroy(gmupt_travtables* h) { delete h; }

// What the renderer holds of the tables above: the device tables as bind uploaded and refit rewrote them, the scalars of its TravScene,
// the refit maps it keeps on the host.  Reads only.
extern "C" int gmupt_debug_read_travtable(gmupt_renderer* r, int which, void* dst, size_t bytes, size_t* needed)
{
    if (!r || !needed) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_read_travtable: null argument");
    *needed = 0;
    if (!r->sceneBound) return fail(GMUPT_ERR_NOT_BOUND, "gmupt_debug_read_travtable: no scene bound");
    HIP_TRY(hipSetDevice(r->dev->id));
    HIP_TRY(hipStreamSynchronize(r->stream));
    const TravScene& t = r->p.trav;
    TravScalars s{};
    s.topCount = t.topCount; s.topCountDeep = t.topCountDeep; s.maxDepth = t.maxDepth; s.rootDesc = t.rootDesc;
    for (int k = 0; k < 3; k++) { s.rootMin[k] = t.rootMin[k]; s.rootMax[k] = t.rootMax[k]; }
    s.triBase = t.triBase; s.wideTopCount = t.wideTopCount; s.wideStackBound = t.wideStackBound; s.numPairs = t.numPairs; s.wideCount = t.wideCount;
    const void* src = nullptr; size_t need = 0; bool onDevice = false;
    auto table = [&](TravTable k) { src = r->trav[k].ptr; need = r->trav[k].bytes; onDevice = true; };
    auto map = [&](const std::vector<uint32_t>& v) { src = v.data(); need = v.size() * 4; };
    switch (which) {
    case GMUPT_TT_NODE64: table(TT_NODES); break; case GMUPT_TT_TRI48: table(TT_TRIS); break; case GMUPT_TT_REC64: table(TT_RECS); break;
    case GMUPT_TT_WNODE: table(TT_WIDE); break; case GMUPT_TT_TRIPAIR: table(TT_PAIRS); break; case GMUPT_TT_PAIRREF: table(TT_PAIRREF); break;
    case GMUPT_TT_SCALARS: src = &s; need = sizeof(s); break;
    case GMUPT_TT_LEVEL_NODES: map(r->rfLevelNodes); break; case GMUPT_TT_LEVEL_OFF: map(r->rfLevelOff); break;
    case GMUPT_TT_NODE_MAP: map(r->rfNodeMap); break; case GMUPT_TT_WIDE_MAP: map(r->rfWideMap); break; case GMUPT_TT_OPENED: map(r->rfOpened); break;
    default: return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_read_travtable: %d is no gmupt_travtable_kind", which);
    }
    *needed = need;
    if (!dst && bytes == 0) return GMUPT_OK;                         // the size query
    if (!dst || bytes < need) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_debug_read_travtable: %zu bytes given, %zu needed", bytes, need);
    if (!need) return GMUPT_OK;
    if (onDevice) HIP_TRY(hipMemcpy(dst, src, need, hipMemcpyDeviceToHost));
    else std::memcpy(dst, src, need);
    return GMUPT_OK;
}

extern "C" int gmupt_debug_wide_tables_addressable(uint32_t wide_nodes, uint32_t num_tris, uint32_t num_pairs)
{
    return wide_tables_addressable(wide_nodes, num_tris, num_pairs) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ LBVH: the GPU builder (pt_lbvh.hip)
extern "C" int gmupt_lbvh_create(gmupt_device* dev, gmupt_lbvh** out) { return work_create("gmupt_lbvh_create", dev, out); }
extern "C" void gmupt_lbvh_destroy(gmupt_lbvh* h) { work_destroy(h); }

extern "C" int gmupt_lbvh_build(gmupt_lbvh* h, const gmupt_buffer* vertices, const int32_t* device_indices, uint32_t num_tris, const uint32_t* device_vertex_material,
                                const gmupt_lbvh_params* params, gmupt_buffer** nodes_out, gmupt_buffer** triangles_out, int32_t* device_ref_triangle,
                                gmupt_lbvh_info* info)
{
    if (nodes_out) *nodes_out = nullptr;
    if (triangles_out) *triangles_out = nullptr;
    if (!h || !vertices || !device_indices || !nodes_out || !triangles_out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_lbvh_build: null argument");
    if (vertices->kind != GMUPT_BUFFER_VERTICES || vertices->dev != h->dev) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_lbvh_build: not a vertex buffer of the builder's device");
    if (vertices->elems == 0 || num_tris == 0) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_lbvh_build: empty mesh");
    if (num_tris > kLbMaxTris || vertices->elems > 0x7FFFFFFFu) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_lbvh_build: more than 2^30 triangles or 2^31 - 1 vertices");
    if (((uintptr_t)device_indices | (uintptr_t)device_vertex_material | (uintptr_t)device_ref_triangle) & 3) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_lbvh_build: misaligned pointer");
    uint32_t L;
    GMUPT_TRY(lbvh_leaf_size("gmupt_lbvh_build", params, &L));
    HIP_TRY(hipSetDevice(h->dev->id));
    size_t sortTemp = 0;
    HIP_TRY(lbvh_sort_temp_bytes(num_tris, &sortTemp));
    GMUPT_TRY(h->reserve(num_tris, sortTemp, lbvh_scratch_bytes));

    LbStaging st{};
    GMUPT_TRY(h->ev.start(h->stream));
    HIP_TRY(launch_lbvh(h->scratch.ptr, h->cap, h->sortTemp, (const float*)vertices->dptr, (uint32_t)vertices->elems, device_indices, num_tris, device_vertex_material, L, h->stream, st));
    GMUPT_TRY(h->ev.stop(h->stream));
    uint32_t back[16] = { 0 };
    GMUPT_TRY(copy_sync(back, st.words, sizeof(back), hipMemcpyDeviceToHost, h->stream));
    if (back[0] & kLbFlagBadIndex) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_lbvh_build: a triangle references a vertex outside the vertex buffer (%zu vertices)", vertices->elems);
    if (back[0] & kLbFlagNonFinite) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_lbvh_build: a vertex used by a triangle is not finite");
    LbResult res{};
    res.numNodes = back[1]; res.numLeaves = (back[1] + 1) / 2; res.depth = back[2];
    for (int k = 0; k < 3; k++) { std::memcpy(&res.rootMin[k], &back[4 + k], 4); std::memcpy(&res.rootMax[k], &back[8 + k], 4); }
    if (res.depth > kMaxTreeDepth) return fail(GMUPT_ERR_UNSUPPORTED, "gmupt_lbvh_build: the tree is %u levels deep, the traversal stacks hold %u", res.depth, kMaxTreeDepth);
    if (res.numNodes == 0 || res.numNodes > 2 * (size_t)num_tris - 1) return fail(GMUPT_ERR_HIP, "gmupt_lbvh_build: the device reported %u nodes for %u triangles", res.numNodes, num_tris);
    float ms = 0.0f;
    GMUPT_TRY(h->ev.elapsed_ms(&ms));

    gmupt_buffer* nb = nullptr; gmupt_buffer* tb = nullptr;
    int rc = output_buffer(h->dev, GMUPT_BUFFER_BVH_NODES, res.numNodes, st.nodes, h->stream, "gmupt_lbvh_build", &nb);
    if (rc == GMUPT_OK) rc = output_buffer(h->dev, GMUPT_BUFFER_TRIANGLES, num_tris, st.tris, h->stream, "gmupt_lbvh_build", &tb);
    hipError_t e = hipSuccess;
    if (rc == GMUPT_OK && device_ref_triangle) e = hipMemcpyAsync(device_ref_triangle, st.ref, (size_t)num_tris * 4, hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (rc == GMUPT_OK && e != hipSuccess) rc = fail(GMUPT_ERR_HIP, "gmupt_lbvh_build: %s", hipGetErrorString(e));
    if (rc != GMUPT_OK) { gmupt_buffer_destroy(nb); gmupt_buffer_destroy(tb); return rc; }
    *nodes_out = nb; *triangles_out = tb;
    lbvh_fill_info(info, res, num_tris, (double)ms);
    return GMUPT_OK;
}
