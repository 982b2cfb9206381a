// C-ABI of libgmupt.so: the entry points that never touch a device -- images, SBVH, camera, the *_host references, default parameters.
#include "gmupt_internal.hpp"
#include "../host/TextureLoader.hpp"
#include "../host/png_reader.hpp"

static int clamp_threads(uint32_t threads) { return (int)std::min(std::max(threads, 1u), 16u); }   // of the *_host references
// what an image (or the rectangle of a record set) may measure
static bool image_size_ok(uint32_t W, uint32_t H) { return W >= 1 && H >= 1 && W <= 65535 && H <= 65535 && (uint64_t)W * H <= (1ull << 28); }

extern "C" int gmupt_image_decode_png(const void* png, size_t bytes, uint32_t* width, uint32_t* height, uint8_t** rgba)
{
    if (!png || !width || !height || !rgba) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_image_decode_png: null argument");
    *rgba = nullptr; *width = *height = 0;
    try {
        gmupt::png::Image img = gmupt::png::decode(static_cast<const uint8_t*>(png), bytes);
        uint8_t* mem = static_cast<uint8_t*>(std::malloc(img.rgba.size()));
        if (!mem) return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_image_decode_png: out of host memory");
        std::memcpy(mem, img.rgba.data(), img.rgba.size());
        *rgba = mem; *width = img.width; *height = img.height;
    } catch (const std::exception& e) { return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_image_decode_png: %s", e.what()); }
    return GMUPT_OK;
}

extern "C" void gmupt_image_free(uint8_t* rgba) { std::free(rgba); }

extern "C" int gmupt_image_resize_square(const uint8_t* rgba, uint32_t old_size, uint32_t new_size, uint8_t* dst)
{
    if (!rgba || !dst || old_size == 0 || new_size == 0) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_image_resize_square: null or empty argument");
    try {
        const std::vector<uint8_t> out = gmupt::resizeSquare(rgba, old_size, new_size);
        std::memcpy(dst, out.data(), out.size());
    } catch (const std::exception& e) { return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_image_resize_square: %s", e.what()); }
    return GMUPT_OK;
}

extern "C" uint32_t gmupt_texture_common_size(const size_t* layer_bytes, uint32_t layers)
{
    if (!layer_bytes || layers == 0) return 0;
    return gmupt::commonDimension(std::vector<size_t>(layer_bytes, layer_bytes + layers));
}

extern "C" int gmupt_bvh_refit_host(gmupt_bvh_node* nodes, uint32_t num_nodes, const gmupt_triangle* tris, uint32_t num_tris,
                                    const float* verts, uint32_t num_verts, uint32_t threads)
{
    if (!nodes || num_nodes == 0 || (!tris && num_tris) || (!verts && num_verts)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_bvh_refit_host: null or empty array");
    const std::string err = validate_tree("gmupt_bvh_refit_host", nodes, num_nodes, tris, num_tris, num_verts, 0);
    if (!err.empty()) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s", err.c_str());
    refit_host(nodes, num_nodes, tris, verts, clamp_threads(threads));
    return GMUPT_OK;
}

// ------------------------------------------------------------------------------------------------ denoiser
static_assert(sizeof(gmupt_denoise_params) == 20 && offsetof(gmupt_denoise_params, sigma_color) == 4 && offsetof(gmupt_denoise_params, sigma_normal) == 8 &&
              offsetof(gmupt_denoise_params, sigma_plane) == 12 && offsetof(gmupt_denoise_params, sigma_albedo) == 16, "gmupt_denoise_params layout");

extern "C" void gmupt_denoise_default_params(gmupt_denoise_params* p)
{
    if (!p) return;
    p->passes = 5; p->sigma_color = 4.0f; p->sigma_normal = 128.0f; p->sigma_plane = 0.02f; p->sigma_albedo = 0.1f;
}

int denoise_params(const char* fn, const gmupt_denoise_params* p, DnParams& out)
{
    gmupt_denoise_params d;
    if (!p) { gmupt_denoise_default_params(&d); p = &d; }
    if (p->passes < 1 || p->passes > GMUPT_DENOISE_MAX_PASSES) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: passes = %u (1..%d)", fn, p->passes, GMUPT_DENOISE_MAX_PASSES);
    const float s[4] = { p->sigma_color, p->sigma_normal, p->sigma_plane, p->sigma_albedo };
    const char* names[4] = { "sigma_color", "sigma_normal", "sigma_plane", "sigma_albedo" };
    for (int k = 0; k < 4; k++)
        if (!(std::isfinite(s[k]) && s[k] > 0.0f)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: %s = %g (finite and > 0)", fn, names[k], (double)s[k]);
    out.passes = (int)p->passes; out.sigmaColor = s[0]; out.sigmaNormal = s[1]; out.sigmaPlane = s[2]; out.sigmaAlbedo = s[3];
    return GMUPT_OK;
}

// the image arguments every denoiser and infill entry checks; device pointers must be 16-byte aligned
int image_args(const char* fn, const void* beauty, const void* aov, uint32_t W, uint32_t H, const void* out, size_t bytes, bool device)
{
    if (!beauty || !aov || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null beauty, aov or output", fn);
    if (device && (((uintptr_t)beauty | (uintptr_t)aov | (uintptr_t)out) & 15u)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: misaligned pointer (16 bytes)", fn);
    if (!image_size_ok(W, H)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: image of %ux%u (1..65535 each, at most 2^28 pixels)", fn, W, H);
    {   // the last pass reads beauty texels of other pixels while it writes the output: the two ranges must not overlap at all
        const uintptr_t b0 = (uintptr_t)beauty, o0 = (uintptr_t)out, n = (uintptr_t)W * H * 16;
        if (o0 < b0 + n && b0 < o0 + n) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: the output overlaps the beauty image", fn);
    }
    if (bytes < (size_t)W * H * 16) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: %zu output bytes for %ux%u RGBA32F texels", fn, bytes, W, H);
    return GMUPT_OK;
}

extern "C" int gmupt_denoise_host(const float* beauty_rgba, const gmupt_aov* aov, uint32_t width, uint32_t height, const gmupt_denoise_params* p,
                                  float* out_rgba, size_t out_bytes, uint32_t threads)
{
    DnParams prm;
    GMUPT_TRY(image_args("gmupt_denoise_host", beauty_rgba, aov, width, height, out_rgba, out_bytes, false));
    GMUPT_TRY(denoise_params("gmupt_denoise_host", p, prm));
    try {
        denoise_host(beauty_rgba, aov, (int)width, (int)height, prm, out_rgba, clamp_threads(threads));
    } catch (const std::bad_alloc&) {
        return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_denoise_host: out of host memory for %ux%u pixels", width, height);
    } catch (const std::exception& e) {
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_denoise_host: %s", e.what());
    }
    return GMUPT_OK;
}

// ------------------------------------------------------------------------------------------------ infill
static_assert(sizeof(gmupt_infill_params) == 16 && offsetof(gmupt_infill_params, sigma_normal) == 4 && offsetof(gmupt_infill_params, sigma_plane) == 8 &&
              offsetof(gmupt_infill_params, sigma_albedo) == 12, "gmupt_infill_params layout");
static_assert(sizeof(gmupt_infill_info) == 24 && offsetof(gmupt_infill_info, filled) == 8 && offsetof(gmupt_infill_info, ms) == 16, "gmupt_infill_info layout");

extern "C" void gmupt_infill_default_params(gmupt_infill_params* p)
{
    if (!p) return;
    p->passes = 6; p->sigma_normal = 32.0f; p->sigma_plane = 0.02f; p->sigma_albedo = 0.1f;
}

int infill_params(const char* fn, const gmupt_infill_params* p, IfParams& out)
{
    gmupt_infill_params d;
    if (!p) { gmupt_infill_default_params(&d); p = &d; }
    if (p->passes < 1 || p->passes > GMUPT_INFILL_MAX_PASSES) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: infill passes = %u (1..%d)", fn, p->passes, GMUPT_INFILL_MAX_PASSES);
    const float s[3] = { p->sigma_normal, p->sigma_plane, p->sigma_albedo };
    const char* names[3] = { "sigma_normal", "sigma_plane", "sigma_albedo" };
    for (int k = 0; k < 3; k++)
        if (!(std::isfinite(s[k]) && s[k] > 0.0f)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: infill %s = %g (finite and > 0)", fn, names[k], (double)s[k]);
    out.passes = (int)p->passes; out.sigmaNormal = s[0]; out.sigmaPlane = s[1]; out.sigmaAlbedo = s[2];
    return GMUPT_OK;
}

extern "C" int gmupt_infill_host(const float* beauty_rgba, const gmupt_aov* aov, uint32_t width, uint32_t height, const gmupt_infill_params* p,
                                 float* out_rgba, size_t out_bytes, gmupt_infill_info* info, uint32_t threads)
{
    IfParams prm;
    GMUPT_TRY(image_args("gmupt_infill_host", beauty_rgba, aov, width, height, out_rgba, out_bytes, false));
    GMUPT_TRY(infill_params("gmupt_infill_host", p, prm));
    IfCounters c{};
    try {
        infill_host(beauty_rgba, aov, (int)width, (int)height, prm, out_rgba, &c, clamp_threads(threads));
    } catch (const std::bad_alloc&) {
        return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_infill_host: out of host memory for %ux%u pixels", width, height);
    } catch (const std::exception& e) {
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_infill_host: %s", e.what());
    }
    if (info) { info->sources = c.sources; info->holes = c.holes; info->filled = c.filled; info->open_left = c.openLeft; info->ms = 0.0; }
    return GMUPT_OK;
}

static_assert(sizeof(gmupt_temporal_params) == 32 && offsetof(gmupt_temporal_params, history_cap) == 20 && offsetof(gmupt_temporal_params, min_normal_cos) == 24 &&
              offsetof(gmupt_temporal_params, plane_dist) == 28, "gmupt_temporal_params layout");
extern "C" void gmupt_temporal_default_params(gmupt_temporal_params* p)
{
    if (!p) return;
    gmupt_denoise_default_params(&p->spatial);
    p->history_cap = 32.0f; p->min_normal_cos = 0.9f; p->plane_dist = 0.02f;
}

int temporal_params(const char* fn, const gmupt_temporal_params* p, DnParams& dn, TpParams& tp)
{
    gmupt_temporal_params d;
    if (!p) { gmupt_temporal_default_params(&d); p = &d; }
    GMUPT_TRY(denoise_params(fn, &p->spatial, dn));
    if (!(std::isfinite(p->history_cap) && p->history_cap >= 0.0f && p->history_cap <= GMUPT_TEMPORAL_MAX_CAP))
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: history_cap = %g (0..%g)", fn, (double)p->history_cap, (double)GMUPT_TEMPORAL_MAX_CAP);
    if (!(std::isfinite(p->min_normal_cos) && p->min_normal_cos <= 1.0f)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: min_normal_cos = %g (finite, <= 1)", fn, (double)p->min_normal_cos);
    if (!(std::isfinite(p->plane_dist) && p->plane_dist >= 0.0f)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: plane_dist = %g (finite and >= 0)", fn, (double)p->plane_dist);
    tp.cap = p->history_cap; tp.minCos = p->min_normal_cos; tp.planeDist = p->plane_dist;
    return GMUPT_OK;
}

static int temporal_integrate_host(const char* fn, const float* beauty_rgba, const gmupt_aov* aov, const gmupt_motion* motion, uint32_t width, uint32_t height,
                                   const gmupt_history* prev, const gmupt_camera_buffer* prev_cam, uint32_t prev_x0, uint32_t prev_y0,
                                   uint32_t prev_width, uint32_t prev_height, const gmupt_temporal_params* p,
                                   float* out_rgba, gmupt_history* out_history, uint32_t threads)
{
    if (!beauty_rgba || !aov || !out_rgba || !out_history) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null beauty, aov or output", fn);
    if (!image_size_ok(width, height)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: image of %ux%u (1..65535 each, at most 2^28 pixels)", fn, width, height);
    if (prev) {
        if (!prev_cam) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: a previous record set without its camera", fn);
        if (!image_size_ok(prev_width, prev_height) || prev_x0 > 65535 || prev_y0 > 65535)
            return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: previous rectangle of %ux%u at (%u, %u) (1..65535 each, at most 2^28 pixels)", fn, prev_width, prev_height, prev_x0, prev_y0);
    }
    {   // the outputs may not overlap each other or any input
        const size_t n = (size_t)width * height;
        const uintptr_t o[2] = { (uintptr_t)out_rgba, (uintptr_t)out_history }, on[2] = { n * 16, n * sizeof(gmupt_history) };
        const uintptr_t i[5] = { (uintptr_t)beauty_rgba, (uintptr_t)aov, (uintptr_t)prev, (uintptr_t)motion, (uintptr_t)out_history },
                        in[5] = { n * 16, n * sizeof(gmupt_aov), prev ? (size_t)prev_width * prev_height * sizeof(gmupt_history) : 0,
                                  motion ? n * sizeof(gmupt_motion) : 0, n * sizeof(gmupt_history) };
        for (int a = 0; a < 2; a++)
            for (int b = 0; b < (a == 0 ? 5 : 4); b++)
                if (in[b] && o[a] < i[b] + in[b] && i[b] < o[a] + on[a]) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: an output overlaps another array", fn);
    }
    gmupt_temporal_params d;
    if (!p) { gmupt_temporal_default_params(&d); p = &d; }
    DnParams dn; TpParams tp;
    GMUPT_TRY(temporal_params(fn, p, dn, tp));
    try {
        temporal_host(beauty_rgba, aov, motion, (int)width, (int)height, prev, prev_cam, (int)prev_x0, (int)prev_y0, (int)prev_width, (int)prev_height, tp,
                      out_rgba, out_history, clamp_threads(threads));
    } catch (const std::bad_alloc&) {
        return fail(GMUPT_ERR_OUT_OF_MEMORY, "%s: out of host memory for %ux%u pixels", fn, width, height);
    } catch (const std::exception& e) {
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: %s", fn, e.what());
    }
    return GMUPT_OK;
}

extern "C" int gmupt_temporal_integrate_host(const float* beauty_rgba, const gmupt_aov* aov, uint32_t width, uint32_t height,
                                             const gmupt_history* prev, const gmupt_camera_buffer* prev_cam, uint32_t prev_x0, uint32_t prev_y0,
                                             uint32_t prev_width, uint32_t prev_height, const gmupt_temporal_params* p,
                                             float* out_rgba, gmupt_history* out_history, uint32_t threads)
{
    return temporal_integrate_host("gmupt_temporal_integrate_host", beauty_rgba, aov, nullptr, width, height, prev, prev_cam, prev_x0, prev_y0, prev_width,
                                   prev_height, p, out_rgba, out_history, threads);
}

extern "C" int gmupt_temporal_integrate_motion_host(const float* beauty_rgba, const gmupt_aov* aov, const gmupt_motion* motion, uint32_t width, uint32_t height,
                                                    const gmupt_history* prev, const gmupt_camera_buffer* prev_cam, uint32_t prev_x0, uint32_t prev_y0,
                                                    uint32_t prev_width, uint32_t prev_height, const gmupt_temporal_params* p,
                                                    float* out_rgba, gmupt_history* out_history, uint32_t threads)
{
    return temporal_integrate_host("gmupt_temporal_integrate_motion_host", beauty_rgba, aov, motion, width, height, prev, prev_cam, prev_x0, prev_y0, prev_width,
                                   prev_height, p, out_rgba, out_history, threads);
}

extern "C" int gmupt_motion_host(const gmupt_hit* hits, const gmupt_aov* aov, size_t n, const gmupt_triangle* tris, uint32_t num_tris,
                                 const float* verts_now, const float* verts_prev, uint32_t num_verts, gmupt_motion* out)
{
    const char* fn = "gmupt_motion_host";
    if (n == 0) return GMUPT_OK;
    if (!hits || !aov || !out || !tris || !verts_now || !verts_prev) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null array", fn);
    for (size_t i = 0; i < n; i++) {
        gmupt_hit h;
        std::memcpy(&h, (const char*)hits + i * sizeof(h), sizeof(h));
        if (h.triangle < 0 || h.light > 0u) continue;
        if ((uint32_t)h.triangle >= num_tris) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: hit %zu names triangle record %d of %u", fn, i, h.triangle, num_tris);
        gmupt_triangle T;
        std::memcpy(&T, (const char*)tris + (size_t)h.triangle * sizeof(T), sizeof(T));
        for (int k = 0; k < 3; k++)
            if (T.v[k] < 0 || (uint32_t)T.v[k] >= num_verts) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: triangle record %d references vertex %d of %u", fn, h.triangle, T.v[k], num_verts);
    }
    motion_host(hits, aov, n, tris, verts_now, verts_prev, out);
    return GMUPT_OK;
}

// ------------------------------------------------------------------------------------------------ LBVH: the GPU builder (pt_lbvh.hip) and its host reference (pt_lbvh.cpp)
static_assert(sizeof(gmupt_lbvh_info) == 48 && offsetof(gmupt_lbvh_info, ms) == 40, "gmupt_lbvh_info layout");

extern "C" void gmupt_lbvh_default_params(gmupt_lbvh_params* p) { if (p) p->max_leaf_size = 4; }

void lbvh_fill_info(gmupt_lbvh_info* info, const LbResult& res, uint32_t numTris, double ms)
{
    if (!info) return;
    info->num_nodes = res.numNodes; info->num_leaves = res.numLeaves; info->depth = res.depth; info->num_tris = numTris;
    for (int k = 0; k < 3; k++) { info->root_min[k] = res.rootMin[k]; info->root_max[k] = res.rootMax[k]; }
    info->ms = ms;
}

int lbvh_leaf_size(const char* fn, const gmupt_lbvh_params* params, uint32_t* L)
{
    *L = params ? params->max_leaf_size : 4u;
    if (*L < 1 || *L > kLbMaxLeaf) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: max_leaf_size %u outside 1..%u", fn, *L, kLbMaxLeaf);
    return GMUPT_OK;
}

extern "C" int gmupt_lbvh_build_host(const float* verts, uint32_t num_verts, const int32_t* indices, uint32_t num_tris, const uint32_t* vertex_material,
                                     const gmupt_lbvh_params* params, gmupt_bvh_node* nodes_out, gmupt_triangle* tris_out, int32_t* ref_triangle_out,
                                     gmupt_lbvh_info* info)
{
    if (!verts || !indices || !nodes_out || !tris_out || num_verts == 0 || num_tris == 0) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_lbvh_build_host: null or empty array");
    if (num_tris > kLbMaxTris) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_lbvh_build_host: more than 2^30 triangles");
    uint32_t L;
    GMUPT_TRY(lbvh_leaf_size("gmupt_lbvh_build_host", params, &L));
    LbResult res{};
    int status = GMUPT_OK;
    const std::string err = lbvh_build_host(verts, num_verts, indices, num_tris, vertex_material, L, nodes_out, tris_out, ref_triangle_out, res, &status);
    if (status != GMUPT_OK) return fail(status, "gmupt_lbvh_build_host: %s", err.c_str());
    lbvh_fill_info(info, res, num_tris, 0.0);
    return GMUPT_OK;
}

// ------------------------------------------------------------------------------------------------ tree optimisation: the host reference (pt_treeopt.cpp) of gmupt_treeopt_run
static_assert(sizeof(gmupt_treeopt_info) == 40 && offsetof(gmupt_treeopt_info, cost_before) == 16 && offsetof(gmupt_treeopt_info, ms) == 32, "gmupt_treeopt_info layout");

extern "C" void gmupt_treeopt_default_params(gmupt_treeopt_params* p) { if (p) p->passes = 3; }

void treeopt_fill_info(gmupt_treeopt_info* info, const ToResult& res, double ms)
{
    if (!info) return;
    info->num_nodes = res.numNodes; info->depth_before = res.depthBefore; info->depth_after = res.depthAfter; info->treelets_rewritten = res.rewritten;
    info->cost_before = res.costBefore; info->cost_after = res.costAfter; info->ms = ms;
}

int treeopt_passes(const char* fn, const gmupt_treeopt_params* params, uint32_t* passes)
{
    *passes = params ? params->passes : 3u;
    if (*passes < 1 || *passes > kToMaxPasses) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: passes %u outside 1..%u", fn, *passes, kToMaxPasses);
    return GMUPT_OK;
}

extern "C" int gmupt_tree_optimize_host(const gmupt_bvh_node* nodes, uint32_t n, const gmupt_treeopt_params* params, gmupt_bvh_node* nodes_out, gmupt_treeopt_info* info)
{
    if (!nodes || !nodes_out || n == 0 || n > 0x7FFFFFFFu) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_tree_optimize_host: null or empty array, or more than 2^31 - 1 records");
    uint32_t passes;
    GMUPT_TRY(treeopt_passes("gmupt_tree_optimize_host", params, &passes));
    ToResult res{};
    int status = GMUPT_OK;
    try {
        const std::string err = tree_optimize_host(nodes, n, passes, nodes_out, res, &status);
        if (status != GMUPT_OK) return fail(status, "gmupt_tree_optimize_host: %s", err.c_str());
    } catch (const std::bad_alloc&) {
        return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_tree_optimize_host: out of host memory for %u records", n);
    }
    treeopt_fill_info(info, res, 0.0);
    return GMUPT_OK;
}

// ------------------------------------------------------------------------------------------------ normals: the host reference (pt_normals.cpp) of gmupt_normals_update
extern "C" int gmupt_vertex_normals_host(const float* verts, uint32_t num_verts, const int32_t* indices, uint32_t num_tris, float* normals_out, uint32_t threads)
{
    if (!verts || !indices || !normals_out || num_verts == 0 || num_tris == 0) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_vertex_normals_host: null or empty array");
    if (num_tris > kNmMaxTris) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_vertex_normals_host: more than 2^30 triangles");
    for (size_t c = 0; c < 3 * (size_t)num_tris; c++)
        if ((uint32_t)indices[c] >= num_verts) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_vertex_normals_host: triangle %zu references vertex %d of %u", c / 3, indices[c], num_verts);
    try {
        normals_host(verts, num_verts, indices, num_tris, normals_out, clamp_threads(threads));
    } catch (const std::bad_alloc&) {
        return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_vertex_normals_host: out of host memory for %u triangles", num_tris);
    }
    return GMUPT_OK;
}

// ------------------------------------------------------------------------------------------------ tree cost: the host reference (pt_treecost.cpp) of gmupt_renderer_tree_cost
extern "C" int gmupt_tree_cost_host(const gmupt_bvh_node* nodes, uint32_t n, gmupt_tree_cost_info* info, uint32_t threads)
{
    if (!nodes || !info || n == 0) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_tree_cost_host: null or empty array");
    TcPartial total;
    try {
        total = tree_cost_host(nodes, n, clamp_threads(threads));
    } catch (const std::bad_alloc&) {
        return fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_tree_cost_host: out of host memory for %u nodes", n);
    }
    tc_fill_info(total, info);
    info->ms = 0.0;
    return GMUPT_OK;
}

// ------------------------------------------------------------------------------------------------ convergence: parameters and the host reference (pt_converge.cpp) of gmupt_converge_update
static_assert(sizeof(gmupt_converge_pixel) == 40 && offsetof(gmupt_converge_pixel, s) == 16 && offsetof(gmupt_converge_pixel, m2) == 32, "gmupt_converge_pixel layout");
static_assert(sizeof(gmupt_converge_params) == 12 && offsetof(gmupt_converge_params, allow_pixels) == 8, "gmupt_converge_params layout");
static_assert(sizeof(gmupt_converge_info) == 56 && offsetof(gmupt_converge_info, max_error) == 24 && offsetof(gmupt_converge_info, sum_error) == 32 &&
              offsetof(gmupt_converge_info, ms) == 48, "gmupt_converge_info layout");

extern "C" void gmupt_converge_default_params(gmupt_converge_params* p)
{
    if (!p) return;
    p->threshold = 0.0f; p->min_batches = 2; p->allow_pixels = 0;
}

int converge_params(const char* fn, const gmupt_converge_params* p, CvParams& out)
{
    gmupt_converge_params d;
    if (!p) { gmupt_converge_default_params(&d); p = &d; }
    if (p->min_batches < 2) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: min_batches = %u (at least 2)", fn, p->min_batches);
    if (std::isnan(p->threshold)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: the threshold is a NaN", fn);
    out.threshold = p->threshold; out.minBatches = p->min_batches; out.allowPixels = p->allow_pixels;
    return GMUPT_OK;
}

extern "C" int gmupt_converge_host(gmupt_converge_pixel* state, const float* rgba, uint32_t width, uint32_t height, const gmupt_converge_params* params,
                                   float* error_or_null, gmupt_converge_info* info)
{
    const char* fn = "gmupt_converge_host";
    if (!state || !rgba || !info) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null state, image or info", fn);
    const uint64_t n = (uint64_t)width * height;
    if (n == 0 || n > 0xFFFFFFFFull) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: image of %ux%u (1 .. 2^32 - 1 pixels)", fn, width, height);
    CvParams prm;
    GMUPT_TRY(converge_params(fn, params, prm));
    CvPartial total;
    try {
        total = converge_host(state, rgba, (size_t)n, prm, error_or_null);
    } catch (const std::bad_alloc&) {
        return fail(GMUPT_ERR_OUT_OF_MEMORY, "%s: out of host memory for %ux%u pixels", fn, width, height);
    }
    cv_fill_info(total, (uint32_t)n, prm, info);
    info->ms = 0.0;
    return GMUPT_OK;
}

// ------------------------------------------------------------------------------------------------ adaptive sampling: parameters and the host rules (pt_adaptive.cpp, pt_adaptive.hpp)
static_assert(sizeof(gmupt_adaptive_params) == 12 && offsetof(gmupt_adaptive_params, uniform_every) == 8, "gmupt_adaptive_params layout");
static_assert(sizeof(gmupt_adaptive_info) == 32 && offsetof(gmupt_adaptive_info, max_rep) == 16 && offsetof(gmupt_adaptive_info, ms) == 24, "gmupt_adaptive_info layout");

extern "C" void gmupt_adaptive_default_params(gmupt_adaptive_params* p)
{
    if (!p) return;
    p->threshold = 0.0f; p->max_repeat = 1; p->uniform_every = 0;
}

int adaptive_params(const char* fn, const gmupt_adaptive_params* p, float monitorThreshold, AdParams& out)
{
    if (!p) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null parameters (there is no default threshold)", fn);
    const float T = p->threshold == 0.0f ? monitorThreshold : p->threshold;
    if (!(T > 0.0f) || !cv_finite(T)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: threshold = %g (finite and > 0)", fn, (double)T);
    if (p->max_repeat < 1 || p->max_repeat > kAdMaxRepeat) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: max_repeat = %u (1..%u)", fn, p->max_repeat, kAdMaxRepeat);
    out.threshold = T; out.maxRepeat = p->max_repeat;
    return GMUPT_OK;
}

extern "C" int gmupt_adaptive_select_host(const float* error, uint32_t width, uint32_t height, const gmupt_adaptive_params* params, uint32_t* list_out,
                                          size_t capacity, gmupt_adaptive_info* info)
{
    const char* fn = "gmupt_adaptive_select_host";
    if (!error || !info) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null error plane or info", fn);
    const uint64_t n = (uint64_t)width * height;
    if (n == 0 || n > 0xFFFFFFFFull) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: plane of %ux%u (1 .. 2^32 - 1 pixels)", fn, width, height);
    AdParams prm;
    GMUPT_TRY(adaptive_params(fn, params, 0.0f, prm));
    if (n * prm.maxRepeat > kAdMaxEntries) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: %ux%u pixels at max_repeat = %u are more than 2^28 entries", fn, width, height, prm.maxRepeat);
    const AdPartial total = adaptive_select_host(error, (size_t)n, prm, nullptr, 0);
    if (list_out) {
        if (capacity < total.entries) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: room for %zu entries given, %u needed", fn, capacity, total.entries);
        adaptive_select_host(error, (size_t)n, prm, list_out, capacity);
    }
    ad_fill_info(total, (uint32_t)n, info);
    info->ms = 0.0;
    return GMUPT_OK;
}

extern "C" int gmupt_adaptive_pixel_host(const uint32_t* list, uint32_t count, uint32_t uniform_every, uint32_t width, uint32_t height, uint32_t k, uint32_t* pix)
{
    const char* fn = "gmupt_adaptive_pixel_host";
    if (!list || !pix) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null list or result", fn);
    const uint64_t n = (uint64_t)width * height;
    if (n == 0 || n > 0xFFFFFFFFull) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: rectangle of %ux%u (1 .. 2^32 - 1 pixels)", fn, width, height);
    if (count == 0) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: an empty list re-aims nothing", fn);
    const uint32_t at = ad_pixel_of(list, count, uniform_every, (uint32_t)n, k);
    if (at >= n) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: list entry %u outside the %ux%u rectangle", fn, at, width, height);
    *pix = at;
    return GMUPT_OK;
}

// ------------------------------------------------------------------------------------------------ thin lens: parameters and the host rule (pt_lens.cpp, pt_lens.hpp)
static_assert(sizeof(gmupt_lens) == 8 && offsetof(gmupt_lens, focus_distance) == 4, "gmupt_lens layout");

extern "C" void gmupt_lens_default_params(gmupt_lens* lens)
{
    if (!lens) return;
    lens->aperture_radius = 0.0f; lens->focus_distance = 1.0f;
}

int lens_params(const char* fn, const gmupt_lens* lens)
{
    if (!lens) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null lens", fn);
    const float a = lens->aperture_radius, f = lens->focus_distance;
    if (!(a >= 0.0f) || !cv_finite(a)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: aperture_radius = %g (finite and >= 0)", fn, (double)a);
    if (a > 0.0f && (!(f > 0.0f) || !cv_finite(f))) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: focus_distance = %g (finite and > 0 while the aperture is open)", fn, (double)f);
    return GMUPT_OK;
}

extern "C" int gmupt_lens_ray_host(const gmupt_camera_buffer* cam, const gmupt_lens* lens, uint32_t q, uint32_t cx, uint32_t cy, gmupt_ray* out)
{
    const char* fn = "gmupt_lens_ray_host";
    if (!cam || !out) return fail(GMUPT_ERR_INVALID_ARGUMENT, "%s: null camera or result", fn);
    GMUPT_TRY(lens_params(fn, lens));
    lens_ray_host(*cam, *lens, q, cx, cy, out);
    return GMUPT_OK;
}

// ------------------------------------------------------------------------------------------------ pose: the host reference (pt_pose.cpp) of gmupt_pose_update
extern "C" int gmupt_pose_host(const float* rest, uint32_t num_verts, const uint16_t* joints, const float* weights, uint32_t influences, const float* joint_mats,
                               uint32_t num_joints, const float* deltas, const float* target_weights, uint32_t num_targets, float* verts_out, uint32_t threads)
{
    if (!rest || !verts_out || num_verts == 0) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_pose_host: null or empty array");
    if (num_joints == 0 && num_targets == 0) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_pose_host: neither joints nor morph targets");
    if (num_joints > kPsMaxJoints || num_targets > kPsMaxTargets)
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_pose_host: %u joints (at most %u), %u targets (at most %u)", num_joints, kPsMaxJoints, num_targets, kPsMaxTargets);
    if (num_joints && (influences < 1 || influences > kPsMaxInfluences)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_pose_host: influences = %u (1..%u)", influences, kPsMaxInfluences);
    if (num_joints && (!joints || !weights || !joint_mats)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_pose_host: %u joints without joint numbers, weights or matrices", num_joints);
    if (num_targets && (!deltas || !target_weights)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_pose_host: %u targets without deltas or weights", num_targets);
    if (num_joints) {
        const size_t bad = pose_first_bad_joint(joints, weights, influences, num_joints, num_verts);
        if (bad < num_verts) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_pose_host: an influence of vertex %zu with a weight that is not zero names a joint outside the %u joints", bad, num_joints);
    }
    pose_host(rest, num_verts, joints, weights, influences, joint_mats, num_joints, deltas, target_weights, num_targets, verts_out, clamp_threads(threads));
    return GMUPT_OK;
}

// ------------------------------------------------------------------------------------------------ host: SBVH
extern "C" void gmupt_sbvh_default_params(gmupt_sbvh_params* p)
{
    if (!p) return;
    p->split_alpha = 1.0e-5f; p->max_depth = 64; p->max_spatial_depth = 48; p->min_leaf_size = 1; p->max_leaf_size = 0x7FFFFFF;
    p->node_cost = 1.0f; p->tri_cost = 1.0f;
}

extern "C" int gmupt_sbvh_build(const float* vertices, uint32_t num_vertices, const int32_t* indices, uint32_t num_triangles,
                                const gmupt_sbvh_params* params, gmupt_sbvh** out)
{
    if (!out || (!vertices && num_vertices) || (!indices && num_triangles)) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_sbvh_build: null argument");
    *out = nullptr;
    gmupt_sbvh_params prm; gmupt_sbvh_default_params(&prm);
    if (params) prm = *params;
    if (prm.max_depth < 1 || prm.max_depth > 64) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_sbvh_build: max_depth %d outside [1, 64]", prm.max_depth);
    try {
        gmupt_sbvh* h = new gmupt_sbvh();
        h->b = new gmupt::SbvhBuilder(vertices, num_vertices, indices, num_triangles, prm);
        h->b->build();
        *out = h;
    } catch (const std::exception& e) {
        return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_sbvh_build: %s", e.what());
    }
    return GMUPT_OK;
}
extern "C" uint32_t gmupt_sbvh_num_nodes(const gmupt_sbvh* h) { return h ? h->b->numNodes() : 0; }
extern "C" uint32_t gmupt_sbvh_num_references(const gmupt_sbvh* h) { return h ? h->b->numReferences() : 0; }
extern "C" float gmupt_sbvh_sah(const gmupt_sbvh* h) { return h ? h->b->sah() : 0.0f; }
extern "C" uint32_t gmupt_sbvh_depth(const gmupt_sbvh* h) { return h ? h->b->depth() : 0; }
extern "C" int gmupt_sbvh_flatten(const gmupt_sbvh* h, const uint32_t* vertex_material, gmupt_bvh_node* nodes, gmupt_triangle* triangles, int32_t* ref_triangle)
{
    if (!h || !nodes) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_sbvh_flatten: null argument");
    h->b->flatten(vertex_material, nodes, triangles, ref_triangle);
    return GMUPT_OK;
}
extern "C" void gmupt_sbvh_destroy(gmupt_sbvh* h) { if (h) { delete h->b; delete h; } }

// ------------------------------------------------------------------------------------------------ host: camera
extern "C" int gmupt_camera_create(uint32_t width, uint32_t height, gmupt_camera** out)
{
    if (!out || !width || !height) return fail(GMUPT_ERR_INVALID_ARGUMENT, "gmupt_camera_create: bad argument");
    *out = new (std::nothrow) gmupt_camera(width, height);
    return *out ? GMUPT_OK : fail(GMUPT_ERR_OUT_OF_MEMORY, "gmupt_camera_create: out of host memory");
}
extern "C" void gmupt_camera_destroy(gmupt_camera* c) { delete c; }
extern "C" void gmupt_camera_update_resolution(gmupt_camera* c, uint32_t width, uint32_t height) { if (c) c->cam.updateResolution(width, height); }
extern "C" void gmupt_camera_set_pose(gmupt_camera* c, float x, float y, float z, float pitch, float yaw) { if (c) { c->cam.setPosition(x, y, z); c->cam.setRotation(pitch, yaw); } }
extern "C" void gmupt_camera_update(gmupt_camera* c, float dt) { if (c) c->cam.update(dt); }
extern "C" void gmupt_camera_set_input(gmupt_camera* c, float mouse_dx, float mouse_dy, uint32_t keys_wsad)
{
    if (!c) return;
    c->cam.addMouseDelta(mouse_dx, mouse_dy);
    c->cam.setKeys((keys_wsad & 1u) != 0, (keys_wsad & 2u) != 0, (keys_wsad & 4u) != 0, (keys_wsad & 8u) != 0);
}

extern "C" void gmupt_camera_reset_accumulation(gmupt_camera* c) { if (c) c->cam.getBuffer()->iterationCounter = -1; }
extern "C" gmupt_camera_buffer* gmupt_camera_get_buffer(gmupt_camera* c) { return c ? c->cam.getBuffer() : nullptr; }
