#include "Scene.hpp"
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <thread>
#include <hip/hip_runtime_api.h>

namespace {
void check(int rc) { if (rc != GMUPT_OK) throw std::runtime_error(gmupt_last_error()); }
DeviceMemory upload(const void* src, size_t bytes, const char* what)
{
	void* d = nullptr;
	if (hipMalloc(&d, bytes) != hipSuccess) throw std::runtime_error(std::string("rebuildOnDevice: cannot allocate the ") + what);
	DeviceMemory mem(d);
	if (hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error(std::string("rebuildOnDevice: cannot upload the ") + what);
	return mem;
}
}

void DeviceFree::operator()(void* p) const { (void)hipFree(p); }

Scene::Scene(gmupt_device* device, const std::string& path)
	: mDevice(device)
	, mSceneName(path)
{
	// Scene.cpp:85: the scene's name is its path below the models directory
	SceneParams& registry = SceneParams::instance;
	const bool belowRoot = !registry.modelsRoot.empty() && path.compare(0, registry.modelsRoot.size(), registry.modelsRoot) == 0;
	if (belowRoot) mSceneName = path.substr(registry.modelsRoot.size());

	loadScene(path);

	std::exception_ptr bvhError;                 // as Source/Scene.cpp:89: BVH build + upload on a worker thread
	std::thread worker([&]() { try { createBVH(); } catch (...) { bvhError = std::current_exception(); } });
	try
	{
		loadTextures(); // decodes / resizes / uploads the three texture arrays on three threads, then uploads the material table

		SceneParams::Entry params;
		if (belowRoot)
		{
			const size_t index = registry.getSceneIndex(mSceneName);   // Scene.cpp:95,315; throws "Non existing scene" like the reference
			params.camera = registry.cameraParams[index]; params.lights = registry.lights[index];
		}
		else
		{
			std::string paramsPath = path;
			const auto dot = paramsPath.find_last_of('.');
			paramsPath = (dot == std::string::npos ? paramsPath : paramsPath.substr(0, dot)) + ".params";
			params = SceneParams::load(paramsPath);
		}
		createLights(params.lights);

		mCamera.setPosition(params.camera.position[0], params.camera.position[1], params.camera.position[2]);
		mCamera.setRotation(params.camera.pitch, params.camera.yaw);
	}
	catch (...) { worker.join(); throw; }

	worker.join();
	if (bvhError) std::rethrow_exception(bvhError);
}

void Scene::update(float dt)
{
	mCamera.update(dt);
}

void Scene::loadScene(const std::string& path)
{
	const bool gltf = (path.size() > 5 && path.compare(path.size() - 5, 5, ".gltf") == 0) || (path.size() > 4 && path.compare(path.size() - 4, 4, ".glb") == 0);
	mScene = (path == "cornell") ? MeshData::cornell() : gltf ? MeshData::loadGltf(path) : MeshData::load(path);
	if (mScene.materials.size() > MAX_LIGHTS) throw std::runtime_error("More than 128 materials (logic.hlsl:8)");
}

void Scene::loadTextures()
{
	// Source/Scene.cpp:126-166: one worker per texture type fills its textureIndices column and creates its Texture2DArray
	std::vector<MaterialProperty>& materialProperties = mScene.materials;
	std::string errors[3];
	auto work = [&](int index, Buffer& resource)
	{
		try
		{
			if (mScene.textureFiles[index].empty()) return;
			createTextures(gmupt::loadSpecificTexture(mScene.textureFiles[index], materialProperties, index), resource);
		}
		catch (const std::exception& e) { errors[index] = e.what(); }
	};
	std::thread diffWorker(work, 0, std::ref(mDiffuse));
	std::thread mtrWorker(work, 1, std::ref(mMetallicRoughness));
	std::thread normWorker(work, 2, std::ref(mNormal));
	diffWorker.join();
	mtrWorker.join();
	normWorker.join();
	for (const std::string& e : errors) if (!e.empty()) throw std::runtime_error(e);
	createPropertyBuffer(materialProperties);
}

void Scene::createTextures(gmupt::TextureSet set, Buffer& resource)
{
	if (set.layers.empty()) return; // Scene.cpp:250-251
	std::vector<uint8_t> packed;
	packed.reserve(set.layers.size() * set.layers[0].size());
	for (const auto& layer : set.layers) packed.insert(packed.end(), layer.begin(), layer.end());
	gmupt_buffer* b = nullptr;
	check(gmupt_texture_array_create(mDevice, packed.data(), set.dimension, static_cast<uint32_t>(set.layers.size()), &b));
	resource.reset(b);
}

void Scene::createBVH()
{
	BVHWrapper bvh(mScene);
	gmupt_buffer* b = nullptr;
	check(gmupt_buffer_create(mDevice, GMUPT_BUFFER_BVH_NODES, bvh.mGPUTree.data(), bvh.mGPUTree.size() * sizeof(BVHWrapper::BVHNode), &b)); mBVHBuffer.reset(b);
	check(gmupt_buffer_create(mDevice, GMUPT_BUFFER_TRIANGLES, bvh.mIndices.data(), bvh.mIndices.size() * sizeof(BVHWrapper::Triangle), &b)); mIndexBuffer.reset(b);
	check(gmupt_buffer_create(mDevice, GMUPT_BUFFER_VERTICES, bvh.mVertices.data(), bvh.mVertices.size() * sizeof(float), &b)); mVertexBuffer.reset(b);
	check(gmupt_buffer_create(mDevice, GMUPT_BUFFER_TRI_PROPS, bvh.mTriangleProperties.data(), bvh.mTriangleProperties.size() * sizeof(BVHWrapper::TriangleProperties), &b)); mTriangleProperties.reset(b);
}

void Scene::createPropertyBuffer(const std::vector<MaterialProperty>& data)
{
	gmupt_buffer* b = nullptr;
	check(gmupt_buffer_create(mDevice, GMUPT_BUFFER_MATERIALS, data.data(), data.size() * sizeof(MaterialProperty), &b));
	mMaterialPropertyBuffer.reset(b);
}

void Scene::createLights(const std::vector<Light>& lights)
{
	if (lights.size() > MAX_LIGHTS) throw std::runtime_error("More than 128 lights");
	mLights = {};
	for (size_t i = 0; i < lights.size(); ++i) mLights[i] = lights[i];
	mLightCount = lights.size();
	gmupt_buffer* b = nullptr;
	check(gmupt_buffer_create(mDevice, GMUPT_BUFFER_LIGHTS, mLights.data(), mLights.size() * sizeof(Light), &b));
	mLightBuffer.reset(b);
}

void Scene::setVertices(const std::vector<float>& xyz, const std::vector<float>* normals)
{
	if (xyz.size() != mScene.vertices.size()) throw std::runtime_error("setVertices: " + std::to_string(xyz.size() / 3) + " vertices for a mesh of " + std::to_string(mScene.numVertices()));
	if (normals && normals->size() != xyz.size()) throw std::runtime_error("setVertices: one normal per vertex");
	check(gmupt_buffer_update(mVertexBuffer.get(), xyz.data(), xyz.size() * sizeof(float)));
	mScene.vertices = xyz;
	if (normals)
	{
		std::vector<gmupt_tri_props> props(mScene.numVertices());
		check(gmupt_buffer_read(mTriangleProperties.get(), props.data(), props.size() * sizeof(gmupt_tri_props)));
		for (size_t i = 0; i < props.size(); ++i) for (int k = 0; k < 3; ++k) props[i].normal[k] = (*normals)[3 * i + k];
		check(gmupt_buffer_update(mTriangleProperties.get(), props.data(), props.size() * sizeof(gmupt_tri_props)));
		mScene.normals = *normals;
	}
}

void Scene::loadRig(const std::string& path)
{
	std::FILE* f = std::fopen(path.c_str(), "rb");
	if (!f) throw std::runtime_error("loadRig: cannot read " + path);
	std::unique_ptr<std::FILE, int (*)(std::FILE*)> closer(f, &std::fclose);
	char magic[4]; uint32_t head[5];
	if (std::fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "GRIG", 4) != 0 || std::fread(head, 4, 5, f) != 5) throw std::runtime_error("loadRig: " + path + " is no .grig file");
	if (head[0] != 1) throw std::runtime_error("loadRig: " + path + " has version " + std::to_string(head[0]) + ", this build reads 1");
	std::unique_ptr<Rig> rig(new Rig());
	rig->numVerts = head[1]; rig->influences = head[2]; rig->numJoints = head[3]; rig->numTargets = head[4];
	if (rig->numVerts != mScene.numVertices()) throw std::runtime_error("loadRig: a rig of " + std::to_string(rig->numVerts) + " vertices for a mesh of " + std::to_string(mScene.numVertices()));
	if (rig->numJoints > 65535 || rig->numTargets > 256 || (rig->numJoints == 0 && rig->numTargets == 0) || (rig->numJoints && (rig->influences < 1 || rig->influences > 8)))
		throw std::runtime_error("loadRig: " + std::to_string(rig->numJoints) + " joints, " + std::to_string(rig->influences) + " influences, " + std::to_string(rig->numTargets) + " targets are outside the limits of the pose rule");
	const size_t V = rig->numVerts, VK = rig->numJoints ? V * rig->influences : 0;
	rig->rest.resize(3 * V); rig->joints.resize(VK); rig->weights.resize(VK); rig->deltas.resize(3 * V * rig->numTargets);
	auto take = [&](void* dst, size_t size, size_t count) { if (count && std::fread(dst, size, count, f) != count) throw std::runtime_error("loadRig: " + path + " is shorter than its header says"); };
	take(rig->rest.data(), 4, rig->rest.size()); take(rig->joints.data(), 2, VK); take(rig->weights.data(), 4, VK); take(rig->deltas.data(), 4, rig->deltas.size());
	if (std::fgetc(f) != EOF) throw std::runtime_error("loadRig: " + path + " is longer than its header says");
	for (size_t i = 0; i < VK; i++) // rule 4 of the pose rule, here so that the message names the file
		if (rig->weights[i] != 0.0f && rig->joints[i] >= rig->numJoints)
			throw std::runtime_error("loadRig: " + path + ": influence " + std::to_string(i % rig->influences) + " of vertex " + std::to_string(i / rig->influences) + " has a weight that is not zero and names joint " +
			                         std::to_string(rig->joints[i]) + " of " + std::to_string(rig->numJoints));
	mRig = std::move(rig);
}

gmupt_lbvh_info Scene::rebuildOnDevice(unsigned maxLeafSize, const std::vector<int32_t>* indices, unsigned optimizePasses, gmupt_treeopt_info* optimizeInfo)
{
	const std::vector<int32_t>& list = indices ? *indices : mScene.indices;
	if (list.empty() || list.size() % 3 != 0) throw std::runtime_error("rebuildOnDevice: " + std::to_string(list.size()) + " indices are no triangle list");
	if (mHipDevice >= 0 && hipSetDevice(mHipDevice) != hipSuccess) throw std::runtime_error("rebuildOnDevice: cannot select device " + std::to_string(mHipDevice));
	if (!mLBVH) { gmupt_lbvh* h = nullptr; check(gmupt_lbvh_create(mDevice, &h)); mLBVH.reset(h); }
	if (!mDeviceVertexMaterial) mDeviceVertexMaterial = upload(mScene.vertexMaterial.data(), mScene.vertexMaterial.size() * sizeof(uint32_t), "vertex materials");
	if (list.size() > mDeviceIndexCapacity)
	{
		mDeviceIndices = upload(list.data(), list.size() * sizeof(int32_t), "indices");
		mDeviceIndexCapacity = list.size();
	}
	else if (hipMemcpy(mDeviceIndices.get(), list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)
		throw std::runtime_error("rebuildOnDevice: cannot upload the indices");

	gmupt_lbvh_params params;
	gmupt_lbvh_default_params(&params);
	params.max_leaf_size = maxLeafSize;
	gmupt_lbvh_info info{};
	gmupt_buffer *nodes = nullptr, *tris = nullptr;
	check(gmupt_lbvh_build(mLBVH.get(), mVertexBuffer.get(), static_cast<const int32_t*>(mDeviceIndices.get()), static_cast<uint32_t>(list.size() / 3),
	                       static_cast<const uint32_t*>(mDeviceVertexMaterial.get()), &params, &nodes, &tris, nullptr, &info));
	if (optimizePasses)
	{
		Buffer plain(nodes), records(tris);                 // released below; destroyed when the optimiser throws
		if (!mTreeopt) { gmupt_treeopt* h = nullptr; check(gmupt_treeopt_create(mDevice, &h)); mTreeopt.reset(h); }
		gmupt_treeopt_info oinfo{};
		nodes = BVHWrapper::optimizeOnDevice(mTreeopt.get(), plain.get(), optimizePasses, &oinfo);
		tris = records.release();
		info.depth = oinfo.depth_after;
		if (optimizeInfo) *optimizeInfo = oinfo;
	}
	if (!mRetiredBVHBuffer) { mRetiredBVHBuffer = std::move(mBVHBuffer); mRetiredIndexBuffer = std::move(mIndexBuffer); }   // (else: never bound, dropped below)
	mBVHBuffer.reset(nodes);
	mIndexBuffer.reset(tris);
	if (indices) mScene.indices = *indices;
	return info;
}

void Scene::setLights(const std::vector<Light>& lights)
{
	if (lights.size() > MAX_LIGHTS) throw std::runtime_error("More than 128 lights");
	mLights = {};
	for (size_t i = 0; i < lights.size(); ++i) mLights[i] = lights[i];
	mLightCount = lights.size();
	check(gmupt_buffer_update(mLightBuffer.get(), mLights.data(), mLights.size() * sizeof(Light)));
	mCamera.getBuffer()->lightCount = static_cast<uint32_t>(lights.size());
	mCamera.getBuffer()->iterationCounter = -1; // GUI.cpp: light edits reset the accumulation
}
