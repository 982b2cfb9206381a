// Headless driver of the C++ host classes: the reference's Window::loop (Source/Window.cpp:60-90: update(dt); draw();)
// without a window.  Used by tests/test_host_cpp_gpu.py.
//   gmupt_render --scene cornell|file.gmesh|file.gltf|file.glb --size WxH --frames N --pool P --live L [--capture] [--dump out.f32] [--pfm out.pfm]
//                [--build-only] [--dump-mesh out.gmesh]   (what the loader produced, for the tests that feed it to the oracle)
//                [--models-root DIR] [--list-scenes]      (SceneParams registry of the reference, Source/Scene.cpp:22-80)
//                [--ranks N --rank R --rendezvous FILE [--device D] [--no-gather]]   one process per GPU: this process renders row band R of N on
//                                                         device D (default R) and the bands are gathered on rank 0 over RCCL (TileGather.hpp);
//                                                         rank 0 writes --dump / --pfm of the whole frame; --no-gather: every rank dumps its band
//                [--print-bands H N]                      the row split, as JSON
//                [--pick X,Y]                             after the frames: what lies under whole-frame pixel (X, Y), as one JSON line
//                [--aov PREFIX [--aov-samples S]]         after the frames: the AOV buffers of the camera (gmupt_render_aovs, S = 1..8, default 1):
//                                                         PREFIX_albedo.pfm, PREFIX_normal.pfm ("PF"), PREFIX_depth.pfm ("Pf") and PREFIX.aov,
//                                                         the raw 64-byte gmupt_aov records, row-major from the top row (single process only)
//                [--denoise PREFIX [--aov-samples S]]     after the frames: the frame through the a-trous denoiser (gmupt_render_denoised, AOVs at
//                                                         S samples per axis): PREFIX.pfm ("PF") and PREFIX.png (the capture's truncation, alpha 255)
//                                                         (single process only)
//                [--infill]                               with --denoise and / or --temporal: surface pixels without a sample take a colour from the sampled
//                                                         pixels of their surface before the filter runs (Renderer::preview, gmupt_infill_default_params)
//                [--vertices FILE]                        before the frames: moved positions for all vertices of the scene (raw little-endian float32,
//                                                         3 per vertex) through Scene::setVertices + Renderer::refitScene; one JSON line with the
//                                                         refit info; not with --ranks
//                [--smooth-normals]                       with --vertices: smooth vertex normals recomputed on the GPU from the moved vertices before
//                                                         the refit (Renderer::refitScene(.., smoothNormals = true))
//                [--rig FILE --pose FILE]                 before the frames: the mesh posed on the GPU (Scene::loadRig + Renderer::poseScene): --rig a ".grig" rig
//                                                         of the scene's vertex count, --pose raw little-endian float32, 12 per joint of the rig, then
//                                                         one weight per morph target; one JSON line with the refit info.  --smooth-normals and
//                                                         --temporal act as with --vertices; not with --vertices, not with --ranks
//                [--tree-cost]                            the surface-area cost of the bound tree (Renderer::treeCost), once after bind and once more
//                                                         after --vertices is applied: one JSON line each with the gmupt_tree_cost_info fields, the
//                                                         doubles as hex bit patterns; not with --ranks
//                [--aperture R --focus D | --focus-at X,Y] depth of field (Renderer::setLens / focusAt, include/gmupt_lens.h): a thin lens of radius R
//                                                         (scene units, > 0) focused at distance D along the camera's forward axis, or on what
//                                                         whole-frame pixel (X, Y) sees after one camera update; one JSON line with the lens, the
//                                                         floats also as hex bit patterns; not with --ranks
//                [--lens-guides]                          with --aperture: --denoise and --aov use the lens-filtered records (Renderer::denoiseLens /
//                                                         renderAovsLens, include/gmupt_lens_aov.h), S*S rays per pixel through the lens; not with --infill
//                [--projection ortho:H | fisheye:DEG | equirect]   another camera (Renderer::setProjection, include/gmupt_projection.h); --pick, --aov and
//                                                         --denoise follow it; one JSON line with the projection; not with --aperture, --temporal, --infill, --ranks
//                [--shutter-to X,Y,Z,PITCH,YAW]           camera motion blur (Renderer::setShutter, include/gmupt_shutter.h): the scene's camera is the pose
//                                                         at shutter open, a camera at position (X, Y, Z) with PITCH and YAW in degrees the pose at shutter
//                                                         close; with --aperture or --projection as well; one JSON line with the close pose; not with --ranks
//                [--until-error T --adaptive [--max-repeat N] [--uniform-every N]]
//                                                         adaptive sampling in that loop (Renderer::renderAdaptive, include/gmupt_adaptive.h): the JSON
//                                                         line gains active, entries, max_rep, skipped_nonfinite of the last plan and paths_generated
//                [--until-error T [--check-every N] [--allow-pixels M] [--error-map FILE.pfm]]
//                                                         the frames run until the image is done (Renderer::renderUntil, include/gmupt.h "Convergence"):
//                                                         after every N frames (default 8) the per-pixel standard error of the tone-mapped luminance
//                                                         mean is estimated, and the loop ends when all but M pixels (default 0) lie at or below T, or
//                                                         after --frames frames; one JSON line with the gmupt_converge_info fields of the last check
//                                                         and the iterations run, the floats as hex bit patterns; FILE.pfm ("Pf") receives the
//                                                         last check's error per pixel (-1: unknown); not with --ranks
//                [--builder sbvh|lbvh [--leaf L]]         lbvh: before the frames (after --vertices) the tree is rebuilt on the GPU from the resident
//                                                         vertices (Renderer::rebuildScene: Scene::rebuildOnDevice + bind), leaves of at most L
//                                                         triangles (default 4); one JSON line with the build info; not with --ranks.
//                                                         With --build-only: BVHWrapper::buildLBVH, the host reference of that build
//                [--optimize N]                           with --builder lbvh: N passes (1..8; 0, the default: none) of the treelet optimiser on the new
//                                                         tree before it is bound (Scene::rebuildOnDevice -> BVHWrapper::optimizeOnDevice), one more
//                                                         JSON line with its info.  With --build-only: gmupt_tree_optimize_host, its host reference
//                [--dump-tree FILE]                       with --build-only: the flattened tree, raw: the 48-byte nodes, then the 16-byte triangle records
//                [--help]                                 this list
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <algorithm>
#include <exception>
#include <stdexcept>
#include <string>
#include "Renderer.hpp"
#include "TileGather.hpp"
#include "png_writer.hpp"
#include <hip/hip_runtime_api.h>
#include <memory>
#include <vector>

namespace {
void writeFloats(const std::string& path, const std::vector<float>& v)
{
	FILE* f = std::fopen(path.c_str(), "wb");
	if (!f || std::fwrite(v.data(), 4, v.size(), f) != v.size()) throw std::runtime_error("cannot write " + path);
	std::fclose(f);
}
void writePfmFile(const std::string& path, const std::vector<float>& rgba, unsigned w, unsigned h)   // "PF", little-endian, bottom row first
{
	std::FILE* f = std::fopen(path.c_str(), "wb");
	if (!f) throw std::runtime_error("Failed to write " + path);
	std::fprintf(f, "PF\n%u %u\n-1.0\n", w, h);
	std::vector<float> row(static_cast<size_t>(w) * 3);
	for (unsigned y = h; y-- > 0;)
	{
		for (unsigned x = 0; x < w; x++) for (int c = 0; c < 3; c++) row[static_cast<size_t>(x) * 3 + static_cast<size_t>(c)] = rgba[(static_cast<size_t>(y) * w + x) * 4 + static_cast<size_t>(c)];
		std::fwrite(row.data(), sizeof(float), row.size(), f);
	}
	std::fclose(f);
}
// one AOV plane as a PFM: "PF" (3 channels) or "Pf" (1), little-endian, bottom row first; offset / channels pick the floats of a record
void writeAovPfm(const std::string& path, const std::vector<gmupt_aov>& aov, unsigned w, unsigned h, size_t offset, int channels)
{
	std::FILE* f = std::fopen(path.c_str(), "wb");
	if (!f) throw std::runtime_error("Failed to write " + path);
	std::fprintf(f, "%s\n%u %u\n-1.0\n", channels == 3 ? "PF" : "Pf", w, h);
	std::vector<float> row(static_cast<size_t>(w) * channels);
	for (unsigned y = h; y-- > 0;)
	{
		for (unsigned x = 0; x < w; x++)
			std::memcpy(&row[static_cast<size_t>(x) * channels], reinterpret_cast<const char*>(&aov[static_cast<size_t>(y) * w + x]) + offset, sizeof(float) * channels);
		std::fwrite(row.data(), sizeof(float), row.size(), f);
	}
	std::fclose(f);
}
std::vector<float> readFloats(const std::string& path)   // a raw float32 file
{
	std::FILE* f = std::fopen(path.c_str(), "rb");
	if (!f) throw std::runtime_error("cannot read " + path);
	std::vector<float> v;
	float chunk[3072];
	for (size_t n; (n = std::fread(chunk, sizeof(float), 3072, f)) > 0;) v.insert(v.end(), chunk, chunk + n);
	std::fclose(f);
	return v;
}
// one float per pixel as a "Pf" PFM: little-endian, bottom row first
void writePlanePfm(const std::string& path, const std::vector<float>& plane, unsigned w, unsigned h)
{
	std::FILE* f = std::fopen(path.c_str(), "wb");
	if (!f) throw std::runtime_error("Failed to write " + path);
	std::fprintf(f, "Pf\n%u %u\n-1.0\n", w, h);
	for (unsigned y = h; y-- > 0;) std::fwrite(&plane[static_cast<size_t>(y) * w], sizeof(float), w, f);
	std::fclose(f);
}
// the gmupt_converge_info fields of the last check and the iterations run as one JSON line; the floats as hex bit patterns (ms as a decimal)
void printConverge(unsigned iterations, const gmupt_converge_info& c, const gmupt_adaptive_info* plan = nullptr, unsigned long long pathsGenerated = 0)
{
	auto bits = [](double d) { unsigned long long u; std::memcpy(&u, &d, sizeof(u)); return u; };
	unsigned m; std::memcpy(&m, &c.max_error, sizeof(m));
	std::printf("{\"converge\": {\"iterations\": %u, \"converged\": %u, \"pixels\": %u, \"unsampled\": %u, \"known\": %u, \"nonfinite\": %u, \"below\": %u, "
	            "\"max_error\": \"%08x\", \"sum_error\": \"%016llx\", \"mean_error\": \"%016llx\", \"ms\": %.6g",
	            iterations, c.converged, c.pixels, c.unsampled, c.known, c.nonfinite, c.below, m, bits(c.sum_error), bits(c.mean_error), c.ms);
	if (plan)   // --adaptive: the last plan's summary and the paths generated
		std::printf(", \"active\": %u, \"entries\": %u, \"max_rep\": %u, \"skipped_nonfinite\": %u, \"paths_generated\": %llu", plan->active, plan->entries, plan->max_rep,
		            plan->skipped_nonfinite, pathsGenerated);
	std::printf("}}\n");
}
// the gmupt_tree_cost_info fields as one JSON line; the doubles as the hex bit patterns of their binary64 values (ms as a decimal: it is a time)
void printTreeCost(const char* when, const gmupt_tree_cost_info& c)
{
	auto bits = [](double d) { unsigned long long u; std::memcpy(&u, &d, sizeof(u)); return u; };
	std::printf("{\"tree_cost\": {\"when\": \"%s\", \"sah\": \"%016llx\", \"sum_inner\": \"%016llx\", \"sum_leaf\": \"%016llx\", \"root_half_area\": \"%016llx\", "
	            "\"num_inner\": %u, \"num_leaves\": %u, \"num_refs\": %llu, \"max_leaf_refs\": %u, \"ms\": %.6g}}\n",
	            when, bits(c.sah), bits(c.sum_inner), bits(c.sum_leaf), bits(c.root_half_area), c.num_inner, c.num_leaves,
	            static_cast<unsigned long long>(c.num_refs), c.max_leaf_refs, c.ms);
}
}

int main(int argc, char** argv)
{
	std::string scene = "cornell", dump, pfm, dumpMesh;
	bool listScenes = false;
	unsigned w = WIDTH, h = HEIGHT, frames = 16, pool = PATHCOUNT, live = REFERENCE_LIVE_PATHS;
	bool capture = false, buildOnly = false, noGather = false;
	unsigned ranks = 1, rank = 0; int device = -1;
	std::string paramsOnly, rendezvous;
	bool doPick = false; float pickX = 0.f, pickY = 0.f;
	std::string verticesFile; bool smoothNormals = false;
	std::string rigFile, poseFile;
	std::string aovPrefix; unsigned aovSamples = 1;
	std::string denoisePrefix;
	std::string temporalPrefix;
	bool infill = false;
	std::string builder = "sbvh", dumpTree; unsigned leaf = 4, optimize = 0;
	bool treeCost = false;
	bool adaptive = false, maxRepeatGiven = false, uniformEveryGiven = false; unsigned maxRepeat = 1, uniformEvery = 0;
	bool lensGuides = false;
	bool projectionGiven = false; gmupt_projection projection{ GMUPT_PROJ_PINHOLE, 3.14159274f, 1.f, 0u };
	bool shutterGiven = false; float shutterTo[5] = { 0.f, 0.f, 0.f, 0.f, 0.f };
	bool apertureGiven = false, focusGiven = false, focusAtGiven = false; float aperture = 0.f, focus = 0.f, focusX = 0.f, focusY = 0.f;
	bool untilError = false, checkEveryGiven = false, allowPixelsGiven = false; float untilThreshold = 0.f; unsigned checkEvery = 8, allowPixels = 0; std::string errorMap;
	for (int i = 1; i < argc; i++) {
		const std::string a = argv[i];
		auto next = [&]() -> const char* { if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", a.c_str()); std::exit(2); } return argv[++i]; };
		if (a == "--scene") scene = next();
		else if (a == "--size") { if (std::sscanf(next(), "%ux%u", &w, &h) != 2) return 2; }
		else if (a == "--frames") frames = std::strtoul(next(), nullptr, 10);
		else if (a == "--pool") pool = std::strtoul(next(), nullptr, 10);
		else if (a == "--live") live = std::strtoul(next(), nullptr, 10);
		else if (a == "--dump") dump = next();
		else if (a == "--pfm") pfm = next();
		else if (a == "--capture") capture = true;
		else if (a == "--build-only") buildOnly = true;
		else if (a == "--params") paramsOnly = next();
		else if (a == "--dump-mesh") dumpMesh = next();
		else if (a == "--models-root") SceneParams::instance.loadScenes(next());
		else if (a == "--list-scenes") listScenes = true;
		else if (a == "--ranks") ranks = std::strtoul(next(), nullptr, 10);
		else if (a == "--rank") rank = std::strtoul(next(), nullptr, 10);
		else if (a == "--rendezvous") rendezvous = next();
		else if (a == "--device") device = std::atoi(next());
		else if (a == "--no-gather") noGather = true;
		else if (a == "--aov") aovPrefix = next();
		else if (a == "--aov-samples") aovSamples = std::strtoul(next(), nullptr, 10);
		else if (a == "--denoise") denoisePrefix = next();
		else if (a == "--vertices") verticesFile = next();
		else if (a == "--smooth-normals") smoothNormals = true;
		else if (a == "--rig") rigFile = next();
		else if (a == "--pose") poseFile = next();
		else if (a == "--temporal") temporalPrefix = next();
		else if (a == "--infill") infill = true;
		else if (a == "--builder") { builder = next(); if (builder != "sbvh" && builder != "lbvh") { std::fprintf(stderr, "--builder takes sbvh or lbvh\n"); return 2; } }
		else if (a == "--leaf") { char* end = nullptr; const char* v = next(); leaf = std::strtoul(v, &end, 10); if (end == v || *end || leaf < 1 || leaf > 64) { std::fprintf(stderr, "--leaf takes a number in 1..64\n"); return 2; } }
		else if (a == "--optimize") { char* end = nullptr; const char* v = next(); optimize = std::strtoul(v, &end, 10); if (end == v || *end || optimize > 8) { std::fprintf(stderr, "--optimize takes a number of passes in 0..8\n"); return 2; } }
		else if (a == "--dump-tree") dumpTree = next();
		else if (a == "--tree-cost") treeCost = true;
		else if (a == "--until-error") { char* end = nullptr; const char* v = next(); untilThreshold = std::strtof(v, &end); untilError = true; if (end == v || *end || untilThreshold != untilThreshold || untilThreshold < 0.f) { std::fprintf(stderr, "--until-error takes a threshold >= 0\n"); return 2; } }
		else if (a == "--check-every") { char* end = nullptr; const char* v = next(); checkEvery = std::strtoul(v, &end, 10); checkEveryGiven = true; if (end == v || *end || checkEvery < 1) { std::fprintf(stderr, "--check-every takes a number of frames >= 1\n"); return 2; } }
		else if (a == "--allow-pixels") { char* end = nullptr; const char* v = next(); allowPixels = std::strtoul(v, &end, 10); allowPixelsGiven = true; if (end == v || *end) { std::fprintf(stderr, "--allow-pixels takes a number of pixels\n"); return 2; } }
		else if (a == "--error-map") errorMap = next();
		else if (a == "--adaptive") adaptive = true;
		else if (a == "--max-repeat") { char* end = nullptr; const char* v = next(); maxRepeat = std::strtoul(v, &end, 10); maxRepeatGiven = true; if (end == v || *end || maxRepeat < 1 || maxRepeat > 64) { std::fprintf(stderr, "--max-repeat takes a number in 1..64\n"); return 2; } }
		else if (a == "--uniform-every") { char* end = nullptr; const char* v = next(); uniformEvery = std::strtoul(v, &end, 10); uniformEveryGiven = true; if (end == v || *end) { std::fprintf(stderr, "--uniform-every takes a number of paths (0 = off)\n"); return 2; } }
		else if (a == "--aperture") { char* end = nullptr; const char* v = next(); aperture = std::strtof(v, &end); apertureGiven = true; if (end == v || *end || !(aperture > 0.f) || aperture > std::numeric_limits<float>::max()) { std::fprintf(stderr, "--aperture takes a finite radius > 0\n"); return 2; } }
		else if (a == "--focus") { char* end = nullptr; const char* v = next(); focus = std::strtof(v, &end); focusGiven = true; if (end == v || *end || !(focus > 0.f) || focus > std::numeric_limits<float>::max()) { std::fprintf(stderr, "--focus takes a finite distance > 0\n"); return 2; } }
		else if (a == "--focus-at") { if (std::sscanf(next(), "%f,%f", &focusX, &focusY) != 2) { std::fprintf(stderr, "--focus-at takes a pixel X,Y\n"); return 2; } focusAtGiven = true; }
		else if (a == "--lens-guides") lensGuides = true;
		else if (a == "--projection") {
			const std::string v = next(); char* end = nullptr; projectionGiven = true;
			if (v == "equirect") projection.kind = GMUPT_PROJ_EQUIRECT;
			else if (v.compare(0, 6, "ortho:") == 0) {
				projection.kind = GMUPT_PROJ_ORTHOGRAPHIC; projection.extent = std::strtof(v.c_str() + 6, &end);
				if (end == v.c_str() + 6 || *end || !(projection.extent > 0.f) || projection.extent > std::numeric_limits<float>::max()) { std::fprintf(stderr, "--projection ortho:H takes a finite height H > 0\n"); return 2; }
			}
			else if (v.compare(0, 8, "fisheye:") == 0) {
				const float deg = std::strtof(v.c_str() + 8, &end);
				if (end == v.c_str() + 8 || *end || !(deg > 0.f) || deg > 360.f) { std::fprintf(stderr, "--projection fisheye:DEG takes a field of view in (0, 360] degrees\n"); return 2; }
				projection.kind = GMUPT_PROJ_FISHEYE; projection.fov = deg >= 360.f ? 6.28318548f : deg * 0.0174532925f;
			}
			else { std::fprintf(stderr, "--projection takes ortho:H, fisheye:DEG or equirect\n"); return 2; }
		}
		else if (a == "--shutter-to") {
			const char* v = next(); char tail = 0; shutterGiven = true;
			bool ok = std::sscanf(v, "%f,%f,%f,%f,%f%c", &shutterTo[0], &shutterTo[1], &shutterTo[2], &shutterTo[3], &shutterTo[4], &tail) == 5;
			for (float c : shutterTo) ok = ok && c - c == 0.f;
			if (!ok) { std::fprintf(stderr, "--shutter-to takes a finite pose X,Y,Z,PITCH,YAW\n"); return 2; }
		}
		else if (a == "--pick") { if (std::sscanf(next(), "%f,%f", &pickX, &pickY) != 2) return 2; doPick = true; }
		else if (a == "--help" || a == "-h") {
			std::printf("gmupt_render --scene cornell|file.gmesh|file.gltf|file.glb --size WxH --frames N --pool P --live L [--capture] [--dump out.f32] [--pfm out.pfm]\n"
			            "             [--build-only] [--dump-mesh out.gmesh] [--models-root DIR] [--list-scenes] [--params FILE]\n"
			            "             [--ranks N --rank R --rendezvous FILE [--device D] [--no-gather]] [--print-bands H N]\n"
			            "             [--pick X,Y]   after the frames: triangle / material / light sphere under whole-frame pixel (X, Y), one JSON line\n"
			            "             [--aov PREFIX [--aov-samples S]]   after the frames: the AOV buffers of the camera, S = 1..8 samples per axis (default 1):\n"
			            "                            PREFIX_albedo.pfm, PREFIX_normal.pfm (PF), PREFIX_depth.pfm (Pf), PREFIX.aov (64-byte gmupt_aov records); not with --ranks\n"
			            "             [--temporal PREFIX] the temporal preview after the frames (PREFIX.pfm); with --vertices the frames are rendered on the loaded pose first,\n"
			            "                                 then on the moved one, and the preview keeps its history across the refit (Renderer::denoiseTemporalMotion)\n"
			            "             [--vertices FILE]   before the frames: moved positions of all vertices (raw float32 xyz), refitted on the GPU; not with --ranks\n"
			            "             [--smooth-normals]  with --vertices: smooth vertex normals recomputed on the GPU from the moved vertices before the refit\n"
			            "             [--rig FILE --pose FILE]   before the frames: the mesh posed on the GPU from a .grig rig and a pose (raw float32: 12 per joint, then one\n"
			            "                                 weight per morph target), then refitted; --smooth-normals and --temporal as with --vertices; not with --vertices or --ranks\n"
			            "             [--tree-cost]       the surface-area cost of the bound tree, measured on the GPU, after bind and again after --vertices is applied:\n"
			            "                                 one JSON line each, the doubles as hex bit patterns; not with --ranks\n"
			            "             [--until-error T [--check-every N] [--allow-pixels M] [--error-map FILE.pfm]]   the frames run until the image is done: every N frames\n"
			            "                                 (default 8) the per-pixel standard error of the tone-mapped luminance mean is estimated; ends when all but M pixels\n"
			            "                                 (default 0) are at or below T, or after --frames; one JSON line with the last check's info and the iterations run,\n"
			            "                                 floats as hex bit patterns; FILE.pfm (Pf): the error per pixel, -1 = unknown; not with --ranks\n"
			            "             [--aperture R --focus D | --focus-at X,Y]   depth of field: a thin lens of radius R > 0 (scene units) focused at distance D along the\n"
			            "                                 forward axis, or on what whole-frame pixel (X, Y) sees after one camera update; one JSON line with the lens;\n"
			            "                                 picks, AOVs and previews stay on the pinhole centre ray; not with --ranks\n"
			            "             [--lens-guides]     with --aperture: --denoise and --aov use the lens-filtered AOV records (S*S rays per pixel through the lens),\n"
			            "                                 so that the guides are blurred where the frame is; not with --infill\n"
			            "             [--projection ortho:H | fisheye:DEG | equirect]   another camera: orthographic with a view H scene units high, equidistant fisheye with\n"
			            "                                 DEG degrees across the image circle, or the 360-degree equirectangular panorama; --pick, --aov and --denoise\n"
			            "                                 follow it (S*S stratified rays per pixel); one JSON line with the projection; not with --aperture, --temporal,\n"
			            "                                 --infill or --ranks\n"
			            "             [--shutter-to X,Y,Z,PITCH,YAW]   camera motion blur: the scene's camera is the pose at shutter open, a camera at (X, Y, Z) with\n"
			            "                                 PITCH and YAW in degrees the pose at shutter close; every camera path leaves a camera between the two; usable\n"
			            "                                 with --aperture or --projection; picks, AOVs and previews stay at shutter open; one JSON line; not with --ranks\n"
			            "             [--until-error T --adaptive [--max-repeat N] [--uniform-every N]]   adaptive sampling: after every check that does not end the loop\n"
			            "                                 the new camera paths go to the pixels still above T, up to N (default 1, at most 64) list entries each,\n"
			            "                                 every N-th path (default 0 = none) to the pixel it would have gone to anyway; T must be > 0; the JSON line\n"
			            "                                 gains active, entries, max_rep and skipped_nonfinite of the last plan and paths_generated\n"
			            "             [--builder sbvh|lbvh [--leaf L]]   lbvh: the tree rebuilt on the GPU before the frames (linear BVH, leaves of at most L triangles,\n"
			            "                                 default 4), one JSON line with the build info; not with --ranks.  With --build-only: the host reference of that build\n"
			            "             [--optimize N]      with --builder lbvh: N = 1..8 passes of the treelet optimiser on the new tree before it is bound (0, the\n"
			            "                                 default: none), one more JSON line with its info.  With --build-only: the host reference of the optimiser\n"
			            "             [--dump-tree FILE]  with --build-only: the flattened tree, raw (48-byte nodes, then 16-byte triangle records)\n"
			            "             [--infill]          with --denoise / --temporal: pixels without a sample are filled from the sampled pixels of their surface\n"
			            "                                 before the filter (Renderer::preview); filled colour never enters the history\n"
			            "             [--denoise PREFIX [--aov-samples S]]   after the frames: the frame through the a-trous denoiser guided by the AOV buffers\n"
			            "                            (S samples per axis): PREFIX.pfm (PF) and PREFIX.png (8-bit, truncated like --capture); not with --ranks\n");
			return 0;
		}
		else if (a == "--print-bands") { // H N: the row bands of an H-row frame over N ranks, as JSON (the CPU tests compare them with tiles.py)
			const unsigned H = std::strtoul(next(), nullptr, 10), N = std::strtoul(next(), nullptr, 10);
			std::printf("[");
			for (unsigned r = 0; r < N; r++) { const auto b = gmupt::rowBand(H, N, r); std::printf("%s[%u, %u]", r ? ", " : "", b.first, b.second); }
			std::printf("]\n");
			return 0;
		}
		else { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
	}
	try
	{
		if (!paramsOnly.empty()) { // SceneParams: the per-scene CSV of the reference (Source/Scene.cpp:34-62)
			const auto e = SceneParams::load(paramsOnly);
			std::printf("{\"camera\": [%.9g, %.9g, %.9g, %.9g, %.9g], \"lights\": [", e.camera.position[0], e.camera.position[1], e.camera.position[2], e.camera.pitch, e.camera.yaw);
			for (size_t i = 0; i < e.lights.size(); i++) {
				const Light& l = e.lights[i];
				std::printf("%s[%.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g]", i ? ", " : "", l.position[0], l.position[1], l.position[2], l.falloff, l.emission[0], l.emission[1], l.emission[2], l.radius);
			}
			std::printf("]}\n");
			return 0;
		}
		if (listScenes) { // the registry: name, camera, number of lights per scene below the models directory
			SceneParams& reg = SceneParams::instance;
			reg.contains("");
			std::printf("[");
			for (size_t i = 0; i < reg.pathNames.size(); i++) {
				const auto& c = reg.cameraParams[i];
				std::printf("%s{\"name\": \"%s\", \"index\": %zu, \"camera\": [%.9g, %.9g, %.9g, %.9g, %.9g], \"lights\": %zu}", i ? ", " : "", reg.pathsReference[i], reg.getSceneIndex(reg.pathNames[i]),
				            c.position[0], c.position[1], c.position[2], c.pitch, c.yaw, reg.lights[i].size());
			}
			std::printf("]\n");
			return 0;
		}
		if (buildOnly) { // host-only leg (BASELINE config 1): scene load + SBVH build + flatten, no GPU
			const bool gltf = (scene.size() > 5 && scene.compare(scene.size() - 5, 5, ".gltf") == 0) || (scene.size() > 4 && scene.compare(scene.size() - 4, 4, ".glb") == 0);
			{ // like Scene::Scene: a scene below the models directory must be one the registry knows (Source/Scene.cpp:75-80,95)
				SceneParams& reg = SceneParams::instance;
				if (!reg.modelsRoot.empty() && scene.compare(0, reg.modelsRoot.size(), reg.modelsRoot) == 0) reg.getSceneIndex(scene.substr(reg.modelsRoot.size()));
			}
			MeshData mesh = (scene == "cornell") ? MeshData::cornell() : gltf ? MeshData::loadGltf(scene) : MeshData::load(scene);
			if (!dumpMesh.empty()) mesh.save(dumpMesh);
			// texture ingestion without the upload: layers, common size and checksum per texture type (Scene.cpp:209-244,268-285)
			std::string texInfo = "[";
			for (int t = 0; t < 3; t++) {
				gmupt::TextureSet set;
				if (!mesh.textureFiles[t].empty()) set = gmupt::loadSpecificTexture(mesh.textureFiles[t], mesh.materials, t);
				unsigned long long sum = 0; for (const auto& layer : set.layers) for (uint8_t v : layer) sum = sum * 31ull + v;
				char buf[128]; std::snprintf(buf, sizeof(buf), "%s{\"layers\": %zu, \"size\": %u, \"checksum\": %llu}", t ? ", " : "", set.layers.size(), set.dimension, sum);
				texInfo += buf;
			}
			texInfo += "], \"texture_indices\": [";
			for (size_t i = 0; i < mesh.materials.size(); i++) { char buf[96]; std::snprintf(buf, sizeof(buf), "%s[%d, %d, %d]", i ? ", " : "", mesh.materials[i].textureIndices[0], mesh.materials[i].textureIndices[1], mesh.materials[i].textureIndices[2]); texInfo += buf; }
			texInfo += "]";
			const auto t0 = std::chrono::steady_clock::now();
			BVHWrapper bvh(mesh, builder == "lbvh" ? BVHWrapper::Builder::LBVH : BVHWrapper::Builder::SBVH, leaf, optimize);
			const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
			float lo[3] = { 1e30f, 1e30f, 1e30f }, hi[3] = { -1e30f, -1e30f, -1e30f };
			for (size_t i = 0; i < mesh.numVertices(); i++) for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], mesh.vertices[3 * i + k]); hi[k] = std::max(hi[k], mesh.vertices[3 * i + k]); }
			size_t glass = 0; for (const auto& m : mesh.materials) glass += m.materialType == GMUPT_MATERIAL_GLASS;
			if (!dumpTree.empty()) {
				std::FILE* f = std::fopen(dumpTree.c_str(), "wb");
				if (!f || std::fwrite(bvh.tree().data(), sizeof(gmupt_bvh_node), bvh.tree().size(), f) != bvh.tree().size() ||
				    std::fwrite(bvh.indices().data(), sizeof(gmupt_triangle), bvh.indices().size(), f) != bvh.indices().size()) throw std::runtime_error("cannot write " + dumpTree);
				std::fclose(f);
			}
			std::printf("{\"triangles\": %zu, \"vertices\": %zu, \"materials\": %zu, \"glass_materials\": %zu, \"nodes\": %zu, \"references\": %zu, \"sah\": %.6f, \"build_s\": %.4f, \"bbox\": [%.6f, %.6f, %.6f, %.6f, %.6f, %.6f], \"textures\": %s}\n",
			            mesh.numTriangles(), mesh.numVertices(), mesh.materials.size(), glass, bvh.tree().size(), bvh.indices().size(), bvh.sah(), s, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], texInfo.c_str());
			return 0;
		}
		if (!aovPrefix.empty() && ranks > 1)
			throw std::invalid_argument("--aov renders the AOV buffers of a single process: it cannot be combined with --ranks N > 1 (there is no multi-rank AOV gather)");
		if (infill && denoisePrefix.empty() && temporalPrefix.empty())
			throw std::invalid_argument("--infill fills the pixels of a preview: it needs --denoise PREFIX or --temporal PREFIX");
		if (!temporalPrefix.empty() && ranks > 1)
			throw std::invalid_argument("--temporal previews the frame of a single process: it cannot be combined with --ranks N > 1");
		if (!denoisePrefix.empty() && ranks > 1)
			throw std::invalid_argument("--denoise filters the frame of a single process: it cannot be combined with --ranks N > 1 (there is no multi-rank AOV gather)");
		if (!verticesFile.empty() && ranks > 1)
			throw std::invalid_argument("--vertices moves the geometry of a single process: it cannot be combined with --ranks N > 1");
		if (!poseFile.empty() && rigFile.empty())
			throw std::invalid_argument("--pose holds the matrices and weights of a rig: it needs --rig FILE");
		if (!rigFile.empty() && poseFile.empty())
			throw std::invalid_argument("--rig loads a rig to pose: it needs --pose FILE");
		if (!poseFile.empty() && !verticesFile.empty())
			throw std::invalid_argument("--pose computes the vertices on the GPU, --vertices uploads them: give one of the two");
		if (!poseFile.empty() && ranks > 1)
			throw std::invalid_argument("--pose moves the geometry of a single process: it cannot be combined with --ranks N > 1");
		if (smoothNormals && verticesFile.empty() && poseFile.empty())
			throw std::invalid_argument("--smooth-normals recomputes the normals of moved vertices: it needs --vertices FILE or --rig FILE --pose FILE");
		if (!untilError && (checkEveryGiven || allowPixelsGiven || !errorMap.empty()))
			throw std::invalid_argument("--check-every, --allow-pixels and --error-map belong to the convergence loop: they need --until-error T");
		if (!adaptive && (maxRepeatGiven || uniformEveryGiven))
			throw std::invalid_argument("--max-repeat and --uniform-every belong to adaptive sampling: they need --adaptive");
		if (adaptive && (!untilError || !(untilThreshold > 0.f) || untilThreshold > std::numeric_limits<float>::max()))
			throw std::invalid_argument("--adaptive plans from the convergence loop: it needs --until-error T with a finite T > 0");
		if (apertureGiven ? (focusGiven == focusAtGiven) : (focusGiven || focusAtGiven))
			throw std::invalid_argument("--aperture R opens a lens focused by exactly one of --focus D and --focus-at X,Y, which need it");
		if (lensGuides && !apertureGiven)
			throw std::invalid_argument("--lens-guides filters the guide records through the lens: it needs --aperture R");
		if (lensGuides && infill)
			throw std::invalid_argument("--lens-guides guides --denoise and --aov: it cannot be combined with --infill");
		if (projectionGiven && apertureGiven)
			throw std::invalid_argument("--projection and --aperture do not combine: the focal plane of a lens has no meaning behind the camera");
		if (projectionGiven && !temporalPrefix.empty())
			throw std::invalid_argument("--projection cannot be combined with --temporal: the temporal projection inverts a pinhole");
		if (projectionGiven && infill)
			throw std::invalid_argument("--projection guides --denoise by its own records: it cannot be combined with --infill");
		if (projectionGiven && ranks > 1)
			throw std::invalid_argument("--projection sets the camera of a single process: it cannot be combined with --ranks N > 1");
		if (apertureGiven && ranks > 1)
			throw std::invalid_argument("--aperture sets the lens of a single process: it cannot be combined with --ranks N > 1");
		if (shutterGiven && ranks > 1)
			throw std::invalid_argument("--shutter-to sets the shutter of a single process: it cannot be combined with --ranks N > 1");
		if (untilError && ranks > 1)
			throw std::invalid_argument("--until-error judges the frame of a single process: it cannot be combined with --ranks N > 1");
		if (treeCost && ranks > 1)
			throw std::invalid_argument("--tree-cost measures the tree of a single process: it cannot be combined with --ranks N > 1");
		if (optimize && builder != "lbvh")
			throw std::invalid_argument("--optimize restructures the tree of --builder lbvh: it needs that option");
		if (builder == "lbvh" && ranks > 1)
			throw std::invalid_argument("--builder lbvh rebuilds the tree of a single process: it cannot be combined with --ranks N > 1");
		if (ranks > 1 || !rendezvous.empty())
		{
			// one process per GPU: row band `rank` of `ranks`, the camera of the whole frame; the bands meet on rank 0 (RCCL send / receive)
			if (ranks == 0 || rank >= ranks) throw std::invalid_argument("--rank must be below --ranks");
			if (rendezvous.empty() && !noGather) throw std::invalid_argument("--ranks needs --rendezvous FILE (or --no-gather)");
			if (device < 0) device = static_cast<int>(rank);
			const auto band = gmupt::rowBand(h, ranks, rank);
			if (band.second == 0) throw std::invalid_argument("more ranks than rows");
			std::unique_ptr<gmupt::TileGather> gather;
			if (!noGather) gather.reset(new gmupt::TileGather(rank, ranks, device, rendezvous));   // first: every rank reaches the rendezvous before the long part
			Renderer renderer(nullptr, { w, h }, scene, device, pool, live, Renderer::RowBand{ band.first, band.second });
			for (unsigned f = 0; f < frames; f++) { renderer.update(0.f); renderer.draw(); }
			if (noGather) { if (!dump.empty()) writeFloats(dump, renderer.readFramebuffer()); }
			else
			{
				void* bandBuffer = nullptr;
				const size_t bytes = static_cast<size_t>(w) * band.second * 4 * sizeof(float);
				if (hipSetDevice(device) != hipSuccess || hipMalloc(&bandBuffer, bytes) != hipSuccess) throw std::runtime_error("cannot allocate the band buffer");
				renderer.copyFramebufferToDevice(bandBuffer);
				const std::vector<float> frame = gather->gatherToRoot(bandBuffer, w, h);
				(void)hipFree(bandBuffer);
				if (rank == 0) { if (!dump.empty()) writeFloats(dump, frame); if (!pfm.empty()) writePfmFile(pfm, frame, w, h); }
			}
			std::printf("rank %u of %u: rendered %llu iterations of rows %u..%u of %ux%u\n", rank, ranks, renderer.iterations(), band.first, band.first + band.second, w, h);
			return 0;
		}
		Renderer renderer(nullptr, { w, h }, scene, 0, pool, live);
		if (treeCost) printTreeCost("bind", renderer.treeCost());
		if ((!verticesFile.empty() || !poseFile.empty()) && !temporalPrefix.empty()) {   // the history of the loaded pose, which the preview after the refit follows
			for (unsigned f = 0; f < frames; f++) { renderer.update(0.f); renderer.draw(); }
			renderer.denoiseTemporalMotion(aovSamples);
		}
		if (!verticesFile.empty()) {
			renderer.scene().setVertices(readFloats(verticesFile));
			const gmupt_refit_info info = renderer.refitScene(!temporalPrefix.empty(), smoothNormals);
			std::printf("{\"refit\": {\"rebuilt\": %u, \"reason\": %u, \"levels\": %u, \"opened_nodes\": %u, \"ms\": %.6g}}\n", info.rebuilt, info.reason, info.levels, info.opened_nodes, info.ms);
			if (treeCost) printTreeCost("vertices", renderer.treeCost());
		}
		if (!poseFile.empty()) {
			renderer.scene().loadRig(rigFile);
			std::vector<float> pose = readFloats(poseFile);
			const Scene::Rig& rig = *renderer.scene().rig();
			const size_t matFloats = 12 * static_cast<size_t>(rig.numJoints);
			if (pose.size() != matFloats + rig.numTargets)
				throw std::runtime_error(poseFile + " holds " + std::to_string(pose.size()) + " floats, the rig needs " + std::to_string(matFloats) + " + " + std::to_string(rig.numTargets));
			const std::vector<float> targetWeights(pose.begin() + static_cast<std::ptrdiff_t>(matFloats), pose.end());
			pose.resize(matFloats);
			const gmupt_refit_info info = renderer.poseScene(pose, targetWeights, !temporalPrefix.empty(), smoothNormals);
			std::printf("{\"refit\": {\"rebuilt\": %u, \"reason\": %u, \"levels\": %u, \"opened_nodes\": %u, \"ms\": %.6g}}\n", info.rebuilt, info.reason, info.levels, info.opened_nodes, info.ms);
			if (treeCost) printTreeCost("pose", renderer.treeCost());
		}
		if (builder == "lbvh") {
			gmupt_treeopt_info oinfo{};
			const gmupt_lbvh_info info = renderer.rebuildScene(leaf, nullptr, optimize, &oinfo);
			std::printf("{\"lbvh\": {\"num_nodes\": %u, \"num_leaves\": %u, \"depth\": %u, \"num_tris\": %u, \"ms\": %.6g}}\n", info.num_nodes, info.num_leaves, info.depth, info.num_tris, info.ms);
			if (optimize)
				std::printf("{\"optimize\": {\"passes\": %u, \"num_nodes\": %u, \"depth_before\": %u, \"depth_after\": %u, \"treelets_rewritten\": %u, \"cost_before\": %.17g, \"cost_after\": %.17g, \"ms\": %.6g}}\n",
				            optimize, oinfo.num_nodes, oinfo.depth_before, oinfo.depth_after, oinfo.treelets_rewritten, oinfo.cost_before, oinfo.cost_after, oinfo.ms);
		}
		if (apertureGiven) {   // after whatever moved or rebuilt the geometry: --focus-at picks in the scene the frames will see
			gmupt_lens lens{ aperture, focus };
			if (focusAtGiven) { renderer.update(0.f); lens = renderer.focusAt(focusX, focusY, aperture); }
			else renderer.setLens(aperture, focus);
			unsigned ab, fb; std::memcpy(&ab, &lens.aperture_radius, 4); std::memcpy(&fb, &lens.focus_distance, 4);
			std::printf("{\"lens\": {\"aperture_radius\": %.9g, \"focus_distance\": %.9g, \"aperture_bits\": \"%08x\", \"focus_bits\": \"%08x\"}}\n", lens.aperture_radius, lens.focus_distance, ab, fb);
		}
		if (projectionGiven) {
			renderer.setProjection(projection);
			unsigned fb, eb; std::memcpy(&fb, &projection.fov, 4); std::memcpy(&eb, &projection.extent, 4);
			std::printf("{\"projection\": {\"kind\": %u, \"fov\": %.9g, \"extent\": %.9g, \"fov_bits\": \"%08x\", \"extent_bits\": \"%08x\"}}\n", projection.kind, projection.fov, projection.extent, fb, eb);
		}
		if (shutterGiven) {   // the close pose from the same Camera code as the open one
			Camera close(w, h);
			close.setPosition(shutterTo[0], shutterTo[1], shutterTo[2]); close.setRotation(shutterTo[3], shutterTo[4]); close.update(0.f);
			renderer.setShutter(close);
			const gmupt_camera_buffer* cb = close.getBuffer();
			std::printf("{\"shutter\": {\"position\": [%.9g, %.9g, %.9g], \"upper_left_corner\": [%.9g, %.9g, %.9g], \"horizontal\": [%.9g, %.9g, %.9g], \"vertical\": [%.9g, %.9g, %.9g]}}\n",
			            cb->position[0], cb->position[1], cb->position[2], cb->upperLeftCorner[0], cb->upperLeftCorner[1], cb->upperLeftCorner[2],
			            cb->horizontal[0], cb->horizontal[1], cb->horizontal[2], cb->vertical[0], cb->vertical[1], cb->vertical[2]);
		}
		if (untilError) {
			gmupt_converge_params cp; gmupt_converge_default_params(&cp);
			cp.threshold = untilThreshold; cp.allow_pixels = allowPixels;
			const size_t pixels = static_cast<size_t>(w) * h;
			struct DeviceFree { void operator()(float* p) const { (void)hipFree(p); } };
			std::unique_ptr<float, DeviceFree> deviceError;   // the error plane on the device, freed on every way out
			if (!errorMap.empty() || adaptive) {
				void* mem = nullptr;
				if (hipMalloc(&mem, pixels * sizeof(float)) != hipSuccess) throw std::runtime_error("cannot allocate the error plane");
				deviceError.reset(static_cast<float*>(mem));
			}
			unsigned ran = 0;
			gmupt_converge_info ci{};
			if (adaptive) {
				gmupt_adaptive_params ap; gmupt_adaptive_default_params(&ap);
				ap.max_repeat = maxRepeat; ap.uniform_every = uniformEvery;   // threshold 0: the monitor's
				const Renderer::AdaptiveRun run = renderer.renderAdaptive(&cp, &ap, checkEvery, frames, deviceError.get());
				ran = run.iterations; ci = run.converge;
				printConverge(ran, ci, &run.plan, run.pathsGenerated);
			} else {
				ci = renderer.renderUntil(&cp, checkEvery, frames, deviceError.get(), &ran);
				printConverge(ran, ci);
			}
			if (!errorMap.empty()) {
				std::vector<float> plane(pixels, -1.0f);   // no check ran: every pixel unknown
				if (ci.pixels && hipMemcpy(plane.data(), deviceError.get(), pixels * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("cannot read the error plane");
				writePlanePfm(errorMap, plane, w, h);
			}
		}
		else for (unsigned f = 0; f < frames; f++) { renderer.update(0.f); renderer.draw(); }
		if (capture) { renderer.requestCapture(); renderer.update(0.f); std::printf("capture %s\n", renderer.lastCapturePath().c_str()); }
		if (doPick) {
			const Renderer::Pick pk = projectionGiven ? renderer.pickProjected(pickX, pickY) : renderer.pick(pickX, pickY);
			const bool found = pk.hit.triangle >= 0 || pk.hit.light > 0;
			float pt[3] = { 0.f, 0.f, 0.f };
			for (int k = 0; k < 3; k++) pt[k] = pk.ray.origin[k] + pk.ray.direction[k] * pk.hit.t;
			std::printf("{\"pick\": [%.9g, %.9g], \"triangle\": %d, \"material\": %u, \"light\": %u, \"t\": %.9g, \"u\": %.9g, \"v\": %.9g, \"origin\": [%.9g, %.9g, %.9g], \"direction\": [%.9g, %.9g, %.9g]",
			            pickX, pickY, pk.hit.triangle, pk.hit.material, pk.hit.light, pk.hit.t, pk.hit.u, pk.hit.v, pk.ray.origin[0], pk.ray.origin[1], pk.ray.origin[2],
			            pk.ray.direction[0], pk.ray.direction[1], pk.ray.direction[2]);
			if (found) std::printf(", \"point\": [%.9g, %.9g, %.9g]}\n", pt[0], pt[1], pt[2]); else std::printf(", \"point\": null}\n");
		}
		if (!aovPrefix.empty()) {
			const std::vector<gmupt_aov> aov = projectionGiven ? renderer.renderAovsProjected(aovSamples) : lensGuides ? renderer.renderAovsLens(aovSamples) : renderer.renderAovs(aovSamples);
			writeAovPfm(aovPrefix + "_albedo.pfm", aov, w, h, offsetof(gmupt_aov, albedo), 3);
			writeAovPfm(aovPrefix + "_normal.pfm", aov, w, h, offsetof(gmupt_aov, normal), 3);
			writeAovPfm(aovPrefix + "_depth.pfm", aov, w, h, offsetof(gmupt_aov, depth), 1);
			std::FILE* f = std::fopen((aovPrefix + ".aov").c_str(), "wb");
			if (!f || std::fwrite(aov.data(), sizeof(gmupt_aov), aov.size(), f) != aov.size()) throw std::runtime_error("cannot write " + aovPrefix + ".aov");
			std::fclose(f);
			std::printf("aov %s: %ux%u, %u samples\n", aovPrefix.c_str(), w, h, aovSamples);
		}
		if (!denoisePrefix.empty()) {
			gmupt_infill_params ip; gmupt_infill_default_params(&ip);
			const std::vector<float> img = infill ? renderer.preview(false, false, aovSamples, nullptr, &ip) : projectionGiven ? renderer.denoiseProjected(aovSamples) : lensGuides ? renderer.denoiseLens(aovSamples) : renderer.denoise(aovSamples);
			writePfmFile(denoisePrefix + ".pfm", img, w, h);
			std::vector<unsigned char> png(img.size());
			for (size_t i = 0; i < img.size(); i += 4) // Renderer::captureScreen's conversion: float * 255 truncated, alpha 255
			{
				png[i] = static_cast<unsigned char>(img[i] * 255);
				png[i + 1] = static_cast<unsigned char>(img[i + 1] * 255);
				png[i + 2] = static_cast<unsigned char>(img[i + 2] * 255);
				png[i + 3] = 255;
			}
			if (!gmupt::writePngRGBA8(denoisePrefix + ".png", png.data(), w, h)) throw std::runtime_error("Failed to write " + denoisePrefix + ".png");
			std::printf("denoise %s: %ux%u, %u aov samples\n", denoisePrefix.c_str(), w, h, aovSamples);
		}
		if (!temporalPrefix.empty()) {
			gmupt_infill_params ip; gmupt_infill_default_params(&ip);
			const std::vector<float> img = infill ? renderer.preview(true, true, aovSamples, nullptr, &ip) : renderer.denoiseTemporalMotion(aovSamples);
			writePfmFile(temporalPrefix + ".pfm", img, w, h);
			std::printf("temporal %s: %ux%u, %u aov samples\n", temporalPrefix.c_str(), w, h, aovSamples);
		}
		if (!pfm.empty()) renderer.writePfm(pfm);
		if (!dump.empty()) {
			const auto fb = renderer.readFramebuffer();
			FILE* f = std::fopen(dump.c_str(), "wb");
			if (!f || std::fwrite(fb.data(), 4, fb.size(), f) != fb.size()) throw std::runtime_error("cannot write " + dump);
			std::fclose(f);
		}
		std::printf("rendered %llu iterations of %ux%u\n", renderer.iterations(), w, h);
	}
	catch (const std::exception& e) // main.cpp:19-23
	{
		std::fprintf(stderr, "error: %s\n", e.what());
		return -1;
	}
	return 0;
}
