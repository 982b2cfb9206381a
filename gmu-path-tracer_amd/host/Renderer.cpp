#include <cstdio>
#include "Renderer.hpp"
#include "png_writer.hpp"
#include <hip/hip_runtime_api.h>
#include <cstdlib>
#include <filesystem>
#include <stdexcept>
#include <type_traits>

namespace fs = std::filesystem;

namespace {
void check(int rc) { if (rc != GMUPT_OK) throw std::runtime_error(gmupt_last_error()); }
}

Renderer::Renderer(void* hwnd, Resolution resolution, const std::string& scene, int hipDevice, unsigned poolPaths, unsigned livePaths, RowBand band)
	: mHwnd(hwnd)
	, mResolution(resolution)
	, mBand(band)
	, mPoolPaths(poolPaths)
	, mLivePaths(livePaths)
{
	mHipDevice = hipDevice;
	createDevice(hipDevice);
	createBuffers(resolution);
	initScene(scene);
	mScene.mCamera.updateResolution(resolution.first, resolution.second);
}

Renderer::~Renderer() = default;

void Renderer::createDevice(int hipDevice)
{
	gmupt_device* d = nullptr;
	check(gmupt_device_create(hipDevice, &d));
	mDevice.reset(d);
}

void Renderer::createBuffers(Resolution res)
{
	gmupt_renderer_desc desc{};
	desc.width = res.first; desc.height = res.second;
	if (mBand.rows)
	{
		if (mBand.y0 + mBand.rows > res.second) throw std::invalid_argument("Renderer: row band outside the frame");
		desc.height = mBand.rows; desc.tile_enabled = 1; desc.tile_x0 = 0; desc.tile_y0 = mBand.y0; // the camera stays the whole frame's
	}
	desc.pool_paths = mPoolPaths; desc.live_paths = mLivePaths;
	gmupt_renderer* r = nullptr;
	check(gmupt_renderer_create(mDevice.get(), &desc, &r));
	mRenderer.reset(r);
}

void Renderer::initScene(const std::string& name)
{
	mNormals.reset();
	mPose.reset();
	mScene = Scene(mDevice.get(), name); // old resources die with the temporary (Source/Renderer.cpp:55)
	mScene.mHipDevice = mHipDevice;
	mScene.mCamera.getBuffer()->lightCount = static_cast<uint32_t>(mScene.lightCount() < 2 ? 2 : mScene.lightCount()); // Camera.hpp:20: never below the default 2
	mSceneBound = false;
}

void Renderer::update(float dt)
{
	if (mHasResize) { resize(mPendingResize); mHasResize = false; }
	if (mCaptureRequested) { captureScreen(); mCaptureRequested = false; }

	mScene.update(dt);
	check(gmupt_set_camera(mRenderer.get(), mScene.mCamera.getBuffer())); // UpdateSubresource(mCameraBuffer), Renderer.cpp:161
	mCameraSet = true;
}

void Renderer::draw()
{
	bindScene();
	check(gmupt_iterate(mRenderer.get())); // logic, newPath, materialUE4, materialGlass, extensionRay, shadowRay (Renderer.cpp:195-211)
	mIterations++;
}

void Renderer::ensureCamera()
{
	bindScene();
	if (!mCameraSet) { check(gmupt_set_camera(mRenderer.get(), mScene.mCamera.getBuffer())); mCameraSet = true; }   // before the first frame: the camera as it stands
}

// The host form of a query: device memory for `count` elements, `call` on it, the copy back.  `name`: the public method, for the message
// of what fails here
template <class T, class Call> std::vector<T> Renderer::readBack(size_t count, const char* name, Call&& call)
{
	std::vector<T> out(count);
	const size_t bytes = out.size() * sizeof(T);
	void* d = nullptr;
	if (hipMalloc(&d, bytes) != hipSuccess) throw std::runtime_error(std::string(name) + ": cannot allocate " + std::to_string(bytes) + " bytes of device memory");
	try { call(static_cast<T*>(d), bytes); }
	catch (...) { (void)hipFree(d); throw; }
	const bool copied = hipMemcpy(out.data(), d, bytes, hipMemcpyDeviceToHost) == hipSuccess;
	(void)hipFree(d);
	if (!copied) throw std::runtime_error(std::string(name) + (std::is_same<T, gmupt_aov>::value ? ": cannot read the records back" : ": cannot read the image back"));
	return out;
}

gmupt_trace_info Renderer::traceRays(const gmupt_ray* closest, uint32_t nClosest, gmupt_hit* hits, const gmupt_ray* any, uint32_t nAny, uint32_t* occluded,
                                     uint32_t lightCount)
{
	bindScene();
	gmupt_trace_info info{};
	check(gmupt_trace_rays(mRenderer.get(), closest, nClosest, hits, any, nAny, occluded, lightCount, &info));
	return info;
}

Renderer::Pick Renderer::pick(float x, float y)
{
	ensureCamera();
	Pick p{};
	check(gmupt_pick(mRenderer.get(), x, y, mScene.mCamera.getBuffer()->lightCount, &p.ray, &p.hit));
	return p;
}

void Renderer::setLens(float apertureRadius, float focusDistance)
{
	const gmupt_lens lens{ apertureRadius, focusDistance };
	check(gmupt_renderer_set_lens(mRenderer.get(), &lens));
	mScene.mCamera.getBuffer()->iterationCounter = -1; // the samples so far were made with the old lens
}

gmupt_lens Renderer::focusAt(float x, float y, float apertureRadius)
{
	ensureCamera();
	gmupt_lens lens{ apertureRadius, 1.f };
	check(gmupt_lens_focus_at(mRenderer.get(), x, y, mScene.mCamera.getBuffer()->lightCount, &lens));
	setLens(lens.aperture_radius, lens.focus_distance);
	return lens;
}

void Renderer::setProjection(const gmupt_projection& projection)
{
	check(gmupt_renderer_set_projection(mRenderer.get(), &projection));
	mScene.mCamera.getBuffer()->iterationCounter = -1; // the samples so far were made with the old projection
}

void Renderer::setShutter(const Camera& close)
{
	gmupt_shutter shutter;
	check(gmupt_shutter_from_camera(close.getBuffer(), &shutter));
	check(gmupt_renderer_set_shutter(mRenderer.get(), &shutter));
	mScene.mCamera.getBuffer()->iterationCounter = -1; // the samples so far were made with the old shutter
}

void Renderer::clearShutter()
{
	check(gmupt_renderer_set_shutter(mRenderer.get(), nullptr));
	mScene.mCamera.getBuffer()->iterationCounter = -1;
}

Renderer::Pick Renderer::pickProjected(float x, float y)
{
	ensureCamera();
	Pick p{};
	check(gmupt_pick_projected(mRenderer.get(), x, y, mScene.mCamera.getBuffer()->lightCount, &p.ray, &p.hit));
	return p;
}

gmupt_trace_info Renderer::renderAovsProjected(gmupt_aov* deviceOut, size_t bytes, unsigned samples)
{
	ensureCamera();
	gmupt_trace_info info{};
	check(gmupt_render_aovs_projected(mRenderer.get(), nullptr, samples, deviceOut, bytes, &info));
	return info;
}

std::vector<gmupt_aov> Renderer::renderAovsProjected(unsigned samples)
{
	return readBack<gmupt_aov>(targetPixels(), "renderAovsProjected", [&](gmupt_aov* d, size_t bytes) { renderAovsProjected(d, bytes, samples); });
}

gmupt_trace_info Renderer::denoiseProjected(float* deviceOut, size_t bytes, unsigned aovSamples, const gmupt_denoise_params* params)
{
	ensureCamera();
	gmupt_trace_info info{};
	check(gmupt_render_denoised_projected(mRenderer.get(), nullptr, aovSamples, params, deviceOut, bytes, &info));
	return info;
}

std::vector<float> Renderer::denoiseProjected(unsigned aovSamples, const gmupt_denoise_params* params)
{
	return readBack<float>(4 * targetPixels(), "denoiseProjected", [&](float* d, size_t bytes) { denoiseProjected(d, bytes, aovSamples, params); });
}

gmupt_trace_info Renderer::renderAovs(gmupt_aov* deviceOut, size_t bytes, unsigned samples)
{
	ensureCamera();
	gmupt_trace_info info{};
	check(gmupt_render_aovs(mRenderer.get(), samples, deviceOut, bytes, &info));
	return info;
}

std::vector<gmupt_aov> Renderer::renderAovs(unsigned samples)
{
	return readBack<gmupt_aov>(targetPixels(), "renderAovs", [&](gmupt_aov* d, size_t bytes) { renderAovs(d, bytes, samples); });
}

gmupt_trace_info Renderer::renderAovsLens(gmupt_aov* deviceOut, size_t bytes, unsigned samples)
{
	ensureCamera();
	gmupt_trace_info info{};
	check(gmupt_render_aovs_lens(mRenderer.get(), nullptr, samples, deviceOut, bytes, &info));
	return info;
}

std::vector<gmupt_aov> Renderer::renderAovsLens(unsigned samples)
{
	return readBack<gmupt_aov>(targetPixels(), "renderAovsLens", [&](gmupt_aov* d, size_t bytes) { renderAovsLens(d, bytes, samples); });
}

gmupt_trace_info Renderer::denoiseLens(float* deviceOut, size_t bytes, unsigned aovSamples, const gmupt_denoise_params* params)
{
	ensureCamera();
	gmupt_trace_info info{};
	check(gmupt_render_denoised_lens(mRenderer.get(), nullptr, aovSamples, params, deviceOut, bytes, &info));
	return info;
}

std::vector<float> Renderer::denoiseLens(unsigned aovSamples, const gmupt_denoise_params* params)
{
	return readBack<float>(4 * targetPixels(), "denoiseLens", [&](float* d, size_t bytes) { denoiseLens(d, bytes, aovSamples, params); });
}

gmupt_trace_info Renderer::denoise(float* deviceOut, size_t bytes, unsigned aovSamples, const gmupt_denoise_params* params)
{
	ensureCamera();
	gmupt_trace_info info{};
	check(gmupt_render_denoised(mRenderer.get(), aovSamples, params, deviceOut, bytes, &info));
	return info;
}

std::vector<float> Renderer::denoise(unsigned aovSamples, const gmupt_denoise_params* params)
{
	return readBack<float>(4 * targetPixels(), "denoise", [&](float* d, size_t bytes) { denoise(d, bytes, aovSamples, params); });
}

gmupt_trace_info Renderer::denoiseTemporal(float* deviceOut, size_t bytes, unsigned aovSamples, const gmupt_temporal_params* params)
{
	ensureCamera();
	if (!mTemporal) { gmupt_temporal* t = nullptr; check(gmupt_temporal_create(mRenderer.get(), &t)); mTemporal.reset(t); }
	gmupt_trace_info info{};
	check(gmupt_render_denoised_temporal(mRenderer.get(), mTemporal.get(), aovSamples, params, deviceOut, bytes, &info));
	return info;
}

gmupt_trace_info Renderer::denoiseTemporalMotion(float* deviceOut, size_t bytes, unsigned aovSamples, const gmupt_temporal_params* params)
{
	ensureCamera();
	if (!mTemporal) { gmupt_temporal* t = nullptr; check(gmupt_temporal_create(mRenderer.get(), &t)); mTemporal.reset(t); }
	gmupt_trace_info info{};
	check(gmupt_render_denoised_temporal_motion(mRenderer.get(), mTemporal.get(), aovSamples, params, deviceOut, bytes, &info));
	return info;
}

std::vector<float> Renderer::denoiseTemporalMotion(unsigned aovSamples, const gmupt_temporal_params* params)
{
	return readBack<float>(4 * targetPixels(), "denoiseTemporalMotion", [&](float* d, size_t bytes) { denoiseTemporalMotion(d, bytes, aovSamples, params); });
}

std::vector<float> Renderer::denoiseTemporal(unsigned aovSamples, const gmupt_temporal_params* params)
{
	return readBack<float>(4 * targetPixels(), "denoiseTemporal", [&](float* d, size_t bytes) { denoiseTemporal(d, bytes, aovSamples, params); });
}

gmupt_trace_info Renderer::preview(float* deviceOut, size_t bytes, bool temporal, bool motion, unsigned aovSamples, const gmupt_temporal_params* params,
                                   const gmupt_infill_params* infill)
{
	ensureCamera();
	if (temporal && !mTemporal) { gmupt_temporal* t = nullptr; check(gmupt_temporal_create(mRenderer.get(), &t)); mTemporal.reset(t); }
	gmupt_trace_info info{};
	check(gmupt_render_preview(mRenderer.get(), temporal ? mTemporal.get() : nullptr, temporal && motion ? GMUPT_PREVIEW_MOTION : 0u, aovSamples, params, infill,
	                           deviceOut, bytes, &info));
	return info;
}

std::vector<float> Renderer::preview(bool temporal, bool motion, unsigned aovSamples, const gmupt_temporal_params* params, const gmupt_infill_params* infill)
{
	return readBack<float>(4 * targetPixels(), "preview", [&](float* d, size_t bytes) { preview(d, bytes, temporal, motion, aovSamples, params, infill); });
}

gmupt_refit_info Renderer::refitScene(bool keepHistory, bool smoothNormals)
{
	gmupt_refit_info info{};
	bindScene(); // (the scene is bound on first use: a refit before the first frame starts from the loaded tree)
	if (smoothNormals)
	{
		if (!mNormals)
		{
			const std::vector<int32_t>& list = mScene.mScene.indices;
			void* d = nullptr;
			if (hipSetDevice(mHipDevice) != hipSuccess || hipMalloc(&d, list.size() * sizeof(int32_t)) != hipSuccess) throw std::runtime_error("refitScene: cannot allocate the index list on the device");
			DeviceMemory indices(d);
			if (hipMemcpy(d, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("refitScene: cannot upload the index list");
			gmupt_normals* n = nullptr;
			check(gmupt_normals_create(mRenderer.get(), static_cast<const int32_t*>(d), static_cast<uint32_t>(list.size() / 3), &n));
			mNormals.reset(n);
		}
		check(gmupt_normals_update(mNormals.get(), nullptr));
	}
	check(gmupt_renderer_refit(mRenderer.get(), &info));
	mScene.mCamera.getBuffer()->iterationCounter = -1; // paths in flight carry hits of the old geometry
	if (!keepHistory) resetHistory();
	return info;
}

gmupt_refit_info Renderer::poseScene(const std::vector<float>& jointMats, const std::vector<float>& targetWeights, bool keepHistory, bool smoothNormals)
{
	const Scene::Rig* rig = mScene.rig();
	if (!rig) throw std::runtime_error("poseScene: the scene has no rig (Scene::loadRig)");
	if (jointMats.size() != 12 * static_cast<size_t>(rig->numJoints) || targetWeights.size() != rig->numTargets)
		throw std::runtime_error("poseScene: " + std::to_string(jointMats.size()) + " matrix floats and " + std::to_string(targetWeights.size()) + " target weights for a rig of " +
		                         std::to_string(rig->numJoints) + " joints and " + std::to_string(rig->numTargets) + " targets");
	bindScene(); // (the scene is bound on first use, as in refitScene)
	if (!mPose)
	{
		if (hipSetDevice(mHipDevice) != hipSuccess) throw std::runtime_error("poseScene: cannot select the device");
		auto upload = [](const void* src, size_t bytes) {
			void* d = nullptr;
			if (bytes == 0) return DeviceMemory(nullptr);
			if (hipMalloc(&d, bytes) != hipSuccess) throw std::runtime_error("poseScene: cannot allocate the rig on the device");
			DeviceMemory mem(d);
			if (hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("poseScene: cannot upload the rig");
			return mem;
		};
		const DeviceMemory rest = upload(rig->rest.data(), rig->rest.size() * sizeof(float)), joints = upload(rig->joints.data(), rig->joints.size() * sizeof(uint16_t));
		const DeviceMemory weights = upload(rig->weights.data(), rig->weights.size() * sizeof(float)), deltas = upload(rig->deltas.data(), rig->deltas.size() * sizeof(float));
		gmupt_pose* p = nullptr;
		check(gmupt_pose_create(mRenderer.get(), static_cast<const float*>(rest.get()), static_cast<const uint16_t*>(joints.get()), static_cast<const float*>(weights.get()),
		                        rig->influences, rig->numJoints, static_cast<const float*>(deltas.get()), rig->numTargets, &p));
		mPose.reset(p);
	}
	check(gmupt_pose_update(mPose.get(), jointMats.empty() ? nullptr : jointMats.data(), targetWeights.empty() ? nullptr : targetWeights.data(), nullptr));
	return refitScene(keepHistory, smoothNormals);
}

gmupt_tree_cost_info Renderer::treeCost()
{
	gmupt_tree_cost_info info{};
	bindScene(); // (the scene is bound on first use, as in refitScene)
	check(gmupt_renderer_tree_cost(mRenderer.get(), nullptr, &info));
	return info;
}

gmupt_converge_info Renderer::renderUntil(const gmupt_converge_params* params, unsigned checkEvery, unsigned maxIterations, float* deviceErrorOrNull,
                                          unsigned* iterations)
{
	if (checkEvery == 0) throw std::invalid_argument("Renderer::renderUntil: checkEvery == 0");
	if (!mConverge) { gmupt_converge* c = nullptr; check(gmupt_converge_create(mRenderer.get(), &c)); mConverge.reset(c); }
	gmupt_converge_info info{};
	unsigned k = 0;
	while (k < maxIterations)
	{
		update(0.f); draw(); // Window::loop
		k++;
		if (k % checkEvery) continue;
		check(gmupt_converge_update(mConverge.get(), params, deviceErrorOrNull, &info)); // behind the frames on the renderer's stream; synchronises
		check(gmupt_synchronize(mRenderer.get()));                                       // the sticky ray-cast flags
		if (info.converged) break;
	}
	if (iterations) *iterations = k;
	return info;
}

Renderer::AdaptiveRun Renderer::renderAdaptive(const gmupt_converge_params* cparams, const gmupt_adaptive_params* aparams, unsigned checkEvery,
                                               unsigned maxIterations, float* deviceError)
{
	if (checkEvery == 0) throw std::invalid_argument("Renderer::renderAdaptive: checkEvery == 0");
	if (!aparams || !deviceError) throw std::invalid_argument("Renderer::renderAdaptive: null parameters or error plane");
	gmupt_converge_params cp;
	if (cparams) cp = *cparams; else gmupt_converge_default_params(&cp);
	gmupt_adaptive_params ap = *aparams;
	if (ap.threshold == 0.f) ap.threshold = cp.threshold;   // "the monitor's"
	if (!mConverge) { gmupt_converge* c = nullptr; check(gmupt_converge_create(mRenderer.get(), &c)); mConverge.reset(c); }
	if (!mAdaptive) { gmupt_adaptive* a = nullptr; check(gmupt_adaptive_create(mRenderer.get(), &a)); mAdaptive.reset(a); }
	AdaptiveRun run{};
	const Resolution target = targetSize();
	check(gmupt_renderer_set_adaptive(mRenderer.get(), nullptr)); // no error plane of this frame yet
	bool attached = false;
	unsigned k = 0;
	while (k < maxIterations)
	{
		update(0.f);
		if (attached && mScene.mCamera.getBuffer()->iterationCounter == 0) { check(gmupt_renderer_set_adaptive(mRenderer.get(), nullptr)); attached = false; } // a restarted frame
		draw();
		k++;
		if (k % checkEvery) continue;
		check(gmupt_converge_update(mConverge.get(), &cp, deviceError, &run.converge)); // synchronises
		check(gmupt_synchronize(mRenderer.get()));
		if (run.converge.converged) break;
		check(gmupt_adaptive_select(mAdaptive.get(), deviceError, target.first, target.second, &ap, &run.plan));
		check(gmupt_renderer_set_adaptive(mRenderer.get(), mAdaptive.get()));
		attached = true;
	}
	check(gmupt_renderer_set_adaptive(mRenderer.get(), nullptr));
	gmupt_stats st{};
	check(gmupt_get_stats(mRenderer.get(), &st));
	run.iterations = k; run.pathsGenerated = st.paths_generated;
	return run;
}

gmupt_lbvh_info Renderer::rebuildScene(unsigned maxLeafSize, const std::vector<int32_t>* indices, unsigned optimizePasses, gmupt_treeopt_info* optimizeInfo)
{
	const gmupt_lbvh_info info = mScene.rebuildOnDevice(maxLeafSize, indices, optimizePasses, optimizeInfo);
	mNormals.reset();                                  // another triangle list needs another adjacency
	mSceneBound = false;
	bindScene();                                       // waits for the renderer's stream before it lets go of the old tree
	mScene.mRetiredBVHBuffer.reset();
	mScene.mRetiredIndexBuffer.reset();
	mScene.mCamera.getBuffer()->iterationCounter = -1; // paths in flight carry hits of the old tree's records
	resetHistory();
	return info;
}

void Renderer::resetHistory()
{
	if (mTemporal) check(gmupt_temporal_reset(mTemporal.get()));
}

void Renderer::bindScene()
{
	if (!mSceneBound)
	{
		check(gmupt_renderer_bind_scene(mRenderer.get(), mScene.mBVHBuffer.get(), mScene.mIndexBuffer.get(), mScene.mVertexBuffer.get(),
		                                mScene.mLightBuffer.get(), mScene.mTriangleProperties.get(), mScene.mMaterialPropertyBuffer.get()));
		// CSSetShaderResources t5..t7 + sampler s0 (Renderer.cpp:173-175,192)
		check(gmupt_renderer_bind_textures(mRenderer.get(), mScene.mDiffuse.get(), mScene.mMetallicRoughness.get(), mScene.mNormal.get()));
		mSceneBound = true;
	}
}

std::vector<float> Renderer::readFramebuffer()
{
	const Resolution t = targetSize();
	std::vector<float> rgba(static_cast<size_t>(t.first) * t.second * 4);
	check(gmupt_read_framebuffer(mRenderer.get(), rgba.data(), rgba.size() * sizeof(float)));
	return rgba;
}

void Renderer::copyFramebufferToDevice(void* deviceDst)
{
	const Resolution t = targetSize();
	check(gmupt_copy_framebuffer_to_device(mRenderer.get(), deviceDst, static_cast<size_t>(t.first) * t.second * 4 * sizeof(float)));
}

void Renderer::writePfm(const std::string& path)
{
	if (mBand.rows) throw std::runtime_error("writePfm: a row band is written by the rank that gathers the frame");
	const auto rgba = readFramebuffer();
	std::FILE* f = std::fopen(path.c_str(), "wb");
	if (!f) throw std::runtime_error("Failed to write " + path);
	std::fprintf(f, "PF\n%u %u\n-1.0\n", mResolution.first, mResolution.second);
	std::vector<float> row(static_cast<size_t>(mResolution.first) * 3);
	for (unsigned y = mResolution.second; y-- > 0;)
	{
		for (unsigned x = 0; x < mResolution.first; x++)
			for (int c = 0; c < 3; c++) row[static_cast<size_t>(x) * 3 + static_cast<size_t>(c)] = rgba[(static_cast<size_t>(y) * mResolution.first + x) * 4 + static_cast<size_t>(c)];
		std::fwrite(row.data(), sizeof(float), row.size(), f);
	}
	std::fclose(f);
}

void Renderer::captureScreen()
{
	if (mBand.rows) throw std::runtime_error("captureScreen: a row band is captured by the rank that gathers the frame");
	// Source/Renderer.cpp:355-406: uint8 = float * 255 (truncation), alpha 255, next free Captures/potatoN.png
	const auto rgba = readFramebuffer();
	std::vector<unsigned char> image(rgba.size());
	for (size_t i = 0; i < rgba.size(); i += 4)
	{
		image[i] = static_cast<unsigned char>(rgba[i] * 255);
		image[i + 1] = static_cast<unsigned char>(rgba[i + 1] * 255);
		image[i + 2] = static_cast<unsigned char>(rgba[i + 2] * 255);
		image[i + 3] = 255;
	}
	auto counter = -1;
	if (fs::exists(CAPTURE_DIR_NAME))
	{
		for (const auto& entry : fs::directory_iterator(CAPTURE_DIR_NAME))
		{
			const auto stem = entry.path().filename().string();
			if (stem.rfind(CAPTURE_NAME, 0) == 0) counter = std::max(counter, std::atoi(stem.substr(std::string(CAPTURE_NAME).size()).c_str()));
		}
	}
	else
		fs::create_directory(CAPTURE_DIR_NAME);
	mLastCapture = std::string(CAPTURE_DIR_NAME) + "/" + CAPTURE_NAME + std::to_string(counter + 1) + ".png";
	if (!gmupt::writePngRGBA8(mLastCapture, image.data(), mResolution.first, mResolution.second))
		throw std::runtime_error("Failed to write " + mLastCapture);
}

void Renderer::resize(const Resolution& resolution)
{
	if (mBand.rows) throw std::runtime_error("resize: the ranks of a tiled render are recreated with their new bands");
	mScene.mCamera.updateResolution(resolution.first, resolution.second); // Renderer.cpp:410
	check(gmupt_resize(mRenderer.get(), resolution.first, resolution.second)); // createRenderTexture, :412
	mResolution = resolution;
}
