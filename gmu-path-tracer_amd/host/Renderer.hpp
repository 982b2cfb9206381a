// Same public surface as the reference's Renderer (Include/Renderer.hpp:9-68): Renderer(HWND, Resolution), update(dt),
// draw().  The D3D11 device / swap chain / UAVs are replaced by C-ABI handles (include/gmupt.h); HWND becomes an opaque,
// nullable window handle (this build is headless).  render() = update(dt); draw(); is the alias BASELINE.json names.
#pragma once
#include <memory>
#include <string>
#include <utility>
#include <vector>
#include "Scene.hpp"
#include "../../include/gmupt_adaptive.h"
#include "../../include/gmupt_lens.h"
#include "../../include/gmupt_lens_aov.h"
#include "../../include/gmupt_projection.h"
#include "../../include/gmupt_shutter.h"

class Renderer
{
	using Resolution = std::pair<unsigned, unsigned>;
public:
	// multi-GPU extension (one process per GPU, TileGather.hpp): this renderer generates paths for the rows [y0, y0 + rows) of the frame only
	// and accumulates into a target of that size; `resolution` and the camera stay those of the whole frame.  rows == 0: the whole frame.
	struct RowBand { unsigned y0, rows; };

	Renderer(void* hwnd, Resolution resolution, const std::string& scene = "cornell", int hipDevice = 0,
	         unsigned poolPaths = PATHCOUNT, unsigned livePaths = REFERENCE_LIVE_PATHS, RowBand band = RowBand{ 0, 0 });
	~Renderer();

	void update(float dt);
	void draw();
	void render(float dt = 0.f) { update(dt); draw(); }

	// requests the reference takes from keyboard / window events (Source/Renderer.cpp:146-156)
	void requestResize(const Resolution& resolution) { mPendingResize = resolution; mHasResize = true; }
	void requestCapture() { mCaptureRequested = true; }
	void initScene(const std::string& name);

	// headless extras
	std::vector<float> readFramebuffer();            // RGBA32F, a = sample count bits (the row band when one was given)
	void copyFramebufferToDevice(void* deviceDst);   // the same texels into caller-owned device memory (the tile gather's source), synchronised
	Resolution targetSize() const { return { mResolution.first, mBand.rows ? mBand.rows : mResolution.second }; }
	void writePfm(const std::string& path);          // raw RGB float export ("PF", little-endian, bottom row first) for image comparisons
	std::string lastCapturePath() const { return mLastCapture; }
	Scene& scene() { return mScene; }
	unsigned long long iterations() const { return mIterations; }

	// ray queries on the bound scene (gmupt_trace_rays): rays and outputs are caller-owned device memory; synchronous, the frame is untouched
	gmupt_trace_info traceRays(const gmupt_ray* closest, uint32_t nClosest, gmupt_hit* hits, const gmupt_ray* any, uint32_t nAny, uint32_t* occluded,
	                           uint32_t lightCount);
	// picking for the GUI's editors (Source/GUI.cpp:110-221): the un-jittered primary ray through whole-frame pixel (x, y) of the current camera
	// and what it hits first, light spheres up to the camera's lightCount included
	struct Pick { gmupt_ray ray; gmupt_hit hit; };
	Pick pick(float x, float y);
	// depth of field (include/gmupt_lens.h): a thin lens of radius `apertureRadius` focused at `focusDistance` along the camera's forward axis,
	// attached to the renderer; apertureRadius == 0 detaches it.  focusAt focuses on what whole-frame pixel (x, y) of the current camera sees
	// (gmupt_lens_focus_at; throws when it sees nothing) and returns the lens it attached.  Both restart the accumulation like a camera move;
	// pick, the AOV planes and the temporal projection stay on the pinhole centre ray.
	void setLens(float apertureRadius, float focusDistance);
	gmupt_lens focusAt(float x, float y, float apertureRadius);
	// camera projections (include/gmupt_projection.h): an orthographic, fisheye or equirectangular camera attached to the renderer; kind
	// GMUPT_PROJ_PINHOLE detaches it.  Restarts the accumulation like a camera move.  Throws while a lens with an aperture is attached (and
	// setLens with one throws while a projection is): the two do not combine.  pickProjected is pick() on the attached projection's ray;
	// renderAovsProjected / denoiseProjected are renderAovsLens / denoiseLens under it (gmupt_render_aovs_projected, gmupt_render_denoised_projected):
	// samples * samples stratified rays per pixel, no centre ray.  The temporal previews stay a pinhole's and must not be used with a projection.
	void setProjection(const gmupt_projection& projection);
	// camera motion blur (include/gmupt_shutter.h): the renderer's camera is the pose at shutter open, `close` (after its update()) the pose
	// at shutter close; every fresh camera path leaves a camera interpolated between the two, under the attached lens or projection.  Both
	// restart the accumulation like a camera move; pick, the AOV planes and the temporal projection stay at shutter open.  A resize detaches.
	void setShutter(const Camera& close);
	void clearShutter();
	Pick pickProjected(float x, float y);
	gmupt_trace_info renderAovsProjected(gmupt_aov* deviceOut, size_t bytes, unsigned samples = 1);
	std::vector<gmupt_aov> renderAovsProjected(unsigned samples = 1);
	gmupt_trace_info denoiseProjected(float* deviceOut, size_t bytes, unsigned aovSamples = 1, const gmupt_denoise_params* params = nullptr);
	std::vector<float> denoiseProjected(unsigned aovSamples = 1, const gmupt_denoise_params* params = nullptr);
	// AOV buffers of the current camera (gmupt_render_aovs): one gmupt_aov per pixel of targetSize(), row-major -- albedo / normal guide images
	// for a denoiser, depth, position, ids.  samples 1..8: s*s stratified rays per pixel for the albedo and normal planes when > 1.
	// The first form writes caller-owned device memory (16-byte aligned, bytes >= pixels * 64); the second returns the records on the host.
	gmupt_trace_info renderAovs(gmupt_aov* deviceOut, size_t bytes, unsigned samples = 1);
	std::vector<gmupt_aov> renderAovs(unsigned samples = 1);
	// the same records seen through the attached lens (gmupt_render_aovs_lens, include/gmupt_lens_aov.h): samples * samples rays per pixel,
	// each pixel-filter cell through its own lens stratum, so that the planes are blurred where the beauty is; without a lens, a pinhole's.
	// denoiseLens is denoise() guided by these records (gmupt_render_denoised_lens).  The forms as renderAovs() and denoise().
	gmupt_trace_info renderAovsLens(gmupt_aov* deviceOut, size_t bytes, unsigned samples = 1);
	std::vector<gmupt_aov> renderAovsLens(unsigned samples = 1);
	gmupt_trace_info denoiseLens(float* deviceOut, size_t bytes, unsigned aovSamples = 1, const gmupt_denoise_params* params = nullptr);
	std::vector<float> denoiseLens(unsigned aovSamples = 1, const gmupt_denoise_params* params = nullptr);
	// the a-trous denoiser on the current frame (gmupt_render_denoised): AOVs of the current camera at aovSamples, then the filter over
	// targetSize(); RGBA32F, rgb denoised, a = the frame's sample-count bits.  params == nullptr: gmupt_denoise_default_params.
	// The first form writes caller-owned device memory (16-byte aligned, bytes >= pixels * 16); the second returns the texels on the host.
	gmupt_trace_info denoise(float* deviceOut, size_t bytes, unsigned aovSamples = 1, const gmupt_denoise_params* params = nullptr);
	std::vector<float> denoise(unsigned aovSamples = 1, const gmupt_denoise_params* params = nullptr);
	// the denoiser with temporal reuse (gmupt_render_denoised_temporal) through this renderer's own history handle, created on first use:
	// the frame integrated with the reprojected history of earlier accumulations, then filtered; a = the effective sample-count bits.
	// params == nullptr: gmupt_temporal_default_params.  The two forms as denoise().  resetHistory() drops the history (gmupt_temporal_reset),
	// e.g. after a light edit, which makes the old history wrong.
	gmupt_trace_info denoiseTemporal(float* deviceOut, size_t bytes, unsigned aovSamples = 1, const gmupt_temporal_params* params = nullptr);
	std::vector<float> denoiseTemporal(unsigned aovSamples = 1, const gmupt_temporal_params* params = nullptr);
	// denoiseTemporal for geometry that moves (gmupt_render_denoised_temporal_motion): the handle keeps the vertex pose of its record sets,
	// and after refitScene(true) the history is looked up where each surface point was.  Without a refit in between it is denoiseTemporal.
	gmupt_trace_info denoiseTemporalMotion(float* deviceOut, size_t bytes, unsigned aovSamples = 1, const gmupt_temporal_params* params = nullptr);
	std::vector<float> denoiseTemporalMotion(unsigned aovSamples = 1, const gmupt_temporal_params* params = nullptr);
	// the preview in one call (gmupt_render_preview): AOVs -> the integration with this renderer's history (temporal; with motion the
	// history follows refitted vertices) -> the guided infill (infill != nullptr: surface pixels without a sample take a colour from the
	// sampled pixels of their surface; filled colour never enters the history) -> the filter.  Without a history only params->spatial
	// is read.  infill == nullptr: denoise(), denoiseTemporal() or denoiseTemporalMotion() bit for bit.  The two forms as denoise().
	gmupt_trace_info preview(float* deviceOut, size_t bytes, bool temporal, bool motion, unsigned aovSamples = 1,
	                         const gmupt_temporal_params* params = nullptr, const gmupt_infill_params* infill = nullptr);
	std::vector<float> preview(bool temporal, bool motion, unsigned aovSamples = 1, const gmupt_temporal_params* params = nullptr,
	                           const gmupt_infill_params* infill = nullptr);
	void resetHistory();
	// after Scene::setVertices: the tree's boxes and this renderer's traversal tables recomputed on the GPU for the moved vertices
	// (gmupt_renderer_refit; the topology of the tree stays), the accumulation restarted, the temporal history dropped -- or kept
	// (keepHistory) for denoiseTemporalMotion, which follows the moved surface.  smoothNormals: before the refit, area-weighted vertex normals
	// are recomputed on the GPU from the moved vertices and written into the property buffer (gmupt_normals_update, include/gmupt.h
	// "normals") through this renderer's own handle, built on first use from the scene's index list and dropped by rebuildScene / initScene.
	// Throws like the other wrappers.
	gmupt_refit_info refitScene(bool keepHistory = false, bool smoothNormals = false);
	// after Scene::loadRig: the mesh posed on the GPU (gmupt_pose_update, include/gmupt.h "Pose") from jointMats (12 floats per joint of the
	// rig) and targetWeights (one per morph target) straight into the vertex buffer, then refitScene(keepHistory, smoothNormals).  The handle
	// is this renderer's own, built on first use from the scene's rig and dropped by initScene.  The posed vertices are never read back:
	// MeshData::vertices keeps the last host-given positions.  Throws std::runtime_error without a rig or on a wrong count.
	gmupt_refit_info poseScene(const std::vector<float>& jointMats, const std::vector<float>& targetWeights, bool keepHistory = false, bool smoothNormals = false);
	// the surface-area cost of the bound tree, measured on the GPU on the renderer's stream (gmupt_renderer_tree_cost, include/gmupt.h
	// "Tree cost"): after a refitScene it tells how far the refitted tree has degraded against its value at bind time, i.e. when
	// rebuildScene pays.  Binds the scene on first use; touches neither the frame nor the accumulation.
	gmupt_tree_cost_info treeCost();
	// frames until the image is done (include/gmupt.h "Convergence"): update(0); draw(); as Window::loop does, and after every checkEvery
	// frames the convergence monitor of this renderer (gmupt_converge_update through its own handle, created on first use) estimates the
	// standard error of every pixel's tone-mapped luminance mean.  Ends at the first check that reports converged, or after maxIterations
	// frames.  params == nullptr: gmupt_converge_default_params (reports only: runs to maxIterations).  deviceErrorOrNull: targetSize()
	// floats of caller-owned device memory that every check fills with the per-pixel error (-1: unknown); it holds the last check's.
	// *iterations = frames run by this call.  Returns the last check's info, all zero when no check ran.  checkEvery == 0 throws.
	gmupt_converge_info renderUntil(const gmupt_converge_params* params, unsigned checkEvery, unsigned maxIterations, float* deviceErrorOrNull = nullptr,
	                                unsigned* iterations = nullptr);
	// renderUntil with adaptive sampling (include/gmupt_adaptive.h): after every check that does not end the loop the monitor's error plane
	// becomes a sampling plan of this renderer (gmupt_adaptive_select through its own handle, created on first use), attached for the next
	// frames: their new camera paths go to the pixels still above the threshold.  aparams->threshold == 0 means cparams' threshold.  The plan
	// is detached before a frame that clears the target and before returning.  deviceError: targetSize() floats of caller-owned device
	// memory, required here (the plan is made from it); it holds the last check's plane.  plan = the last selection's summary (all zero
	// when none ran), pathsGenerated = gmupt_stats::paths_generated of the renderer after the last frame.  checkEvery == 0 throws.
	struct AdaptiveRun { gmupt_converge_info converge; gmupt_adaptive_info plan; unsigned iterations; unsigned long long pathsGenerated; };
	AdaptiveRun renderAdaptive(const gmupt_converge_params* cparams, const gmupt_adaptive_params* aparams, unsigned checkEvery, unsigned maxIterations,
	                           float* deviceError);
	// geometry a refit does not cover (after Scene::setVertices with vertices that moved far, or with another triangle list): a new tree
	// from the GPU LBVH builder (Scene::rebuildOnDevice) bound in place of the old one, the accumulation restarted and the temporal history
	// dropped -- a new binding is a new geometry.  The host pass of the bind (the traversal tables) runs as for any bind.
	// optimizePasses > 0: the treelet optimiser runs on the new tree before it is bound (Scene::rebuildOnDevice has the details).
	gmupt_lbvh_info rebuildScene(unsigned maxLeafSize = 4, const std::vector<int32_t>* indices = nullptr, unsigned optimizePasses = 0,
	                             gmupt_treeopt_info* optimizeInfo = nullptr);

private:
	void createDevice(int hipDevice);
	void createBuffers(Resolution res);
	void captureScreen();
	void resize(const Resolution& resolution);
	void bindScene();
	void ensureCamera();   // bindScene(), and before the first frame the camera as it stands: what every query on the current camera starts with
	size_t targetPixels() const { return static_cast<size_t>(targetSize().first) * targetSize().second; }
	template <class T, class Call> std::vector<T> readBack(size_t count, const char* name, Call&& call);   // the host forms: call(deviceOut, bytes), read back

	struct DeviceDeleter { void operator()(gmupt_device* d) const { gmupt_device_destroy(d); } };
	struct RendererDeleter { void operator()(gmupt_renderer* r) const { gmupt_renderer_destroy(r); } };
	struct TemporalDeleter { void operator()(gmupt_temporal* t) const { gmupt_temporal_destroy(t); } };
	struct NormalsDeleter { void operator()(gmupt_normals* n) const { gmupt_normals_destroy(n); } };
	struct PoseDeleter { void operator()(gmupt_pose* p) const { gmupt_pose_destroy(p); } };
	struct ConvergeDeleter { void operator()(gmupt_converge* c) const { gmupt_converge_destroy(c); } };
	struct AdaptiveDeleter { void operator()(gmupt_adaptive* a) const { gmupt_adaptive_destroy(a); } };

	void* mHwnd;
	std::unique_ptr<gmupt_device, DeviceDeleter> mDevice;
	std::unique_ptr<gmupt_renderer, RendererDeleter> mRenderer; // path state, queues, counters, accumulation target
	std::unique_ptr<gmupt_temporal, TemporalDeleter> mTemporal; // history of denoiseTemporal (declared after mRenderer: destroyed before it)
	std::unique_ptr<gmupt_normals, NormalsDeleter> mNormals;    // adjacency of refitScene(.., smoothNormals) (declared after mRenderer: destroyed before it)
	std::unique_ptr<gmupt_pose, PoseDeleter> mPose;             // the rig of poseScene on the device (declared after mRenderer: destroyed before it)
	std::unique_ptr<gmupt_converge, ConvergeDeleter> mConverge; // the monitor of renderUntil (declared after mRenderer: destroyed before it)
	std::unique_ptr<gmupt_adaptive, AdaptiveDeleter> mAdaptive; // the sampling plan of renderAdaptive (declared after mRenderer: destroyed before it)
	Scene mScene;
	Resolution mResolution;
	RowBand mBand;
	unsigned mPoolPaths, mLivePaths;
	int mHipDevice = 0;
	bool mSceneBound = false, mCameraSet = false;
	bool mHasResize = false, mCaptureRequested = false;
	Resolution mPendingResize{};
	std::string mLastCapture;
	unsigned long long mIterations = 0;
};
