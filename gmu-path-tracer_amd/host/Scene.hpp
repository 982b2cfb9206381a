// Same public surface as the reference's Scene / SceneParams / Light / MaterialProperty (Include/Scene.hpp:13-120), with the
// ID3D11Device replaced by the C-ABI device handle and uni::Buffer members by gmupt_buffer handles (move-only RAII).
#pragma once
#include <array>
#include <memory>
#include <string>
#include <vector>
#include "Camera.hpp"
#include "BVHWrapper.hpp"
#include "Constants.hpp"
#include "TextureLoader.hpp"

using Light = gmupt_light;                   // Include/Scene.hpp:13-19
using MaterialProperty = gmupt_material;     // Include/Scene.hpp:43-68

// The reference's registry of scenes (Include/Scene.hpp:21-41, Source/Scene.cpp:22-80): every *.gltf below the models directory with the
// camera pose and lights of its sibling .params file (or the defaults).  Differences: the models directory is a settable path (the
// reference hard-codes "Assets\\Models\\" relative to the working directory), names use the platform's separator, .glb files are listed
// too, and the registry is filled on first use instead of during static initialisation.
struct SceneParams
{
	struct CameraParam { float position[3]; float pitch; float yaw; };
	struct Entry { std::vector<Light> lights; CameraParam camera; };

	void loadScenes();                                   // scans modelsRoot recursively (Scene.cpp:22-73); replaces the current lists
	void loadScenes(const std::string& root);            // the same after modelsRoot = root
	size_t getSceneIndex(const std::string& name);       // name relative to modelsRoot; throws std::runtime_error("Non existing scene <name>") (Scene.cpp:75-80)
	bool contains(const std::string& name);

	std::vector<std::string> pathNames;                  // scene names relative to modelsRoot, in directory-walk order
	std::vector<const char*> pathsReference;             // the same as C strings (GUI.cpp:72 hands them to its combo box)
	std::vector<std::vector<Light>> lights;
	std::vector<CameraParam> cameraParams;
	std::string modelsRoot = "Assets/Models/";

	static SceneParams instance;

	// row 0 = camera (x,y,z,pitch,yaw), rows 1.. = lights (x,y,z,falloff,r,g,b,radius); defaults if the file is missing
	// (Source/Scene.cpp:34-62)
	static Entry load(const std::string& paramsPath);

private:
	bool mLoaded = false;
};

struct BufferDeleter { void operator()(gmupt_buffer* b) const { gmupt_buffer_destroy(b); } };
using Buffer = std::unique_ptr<gmupt_buffer, BufferDeleter>;
struct LbvhDeleter { void operator()(gmupt_lbvh* h) const { gmupt_lbvh_destroy(h); } };
struct TreeoptDeleter { void operator()(gmupt_treeopt* h) const { gmupt_treeopt_destroy(h); } };
struct DeviceFree { void operator()(void* p) const; };   // hipFree
using DeviceMemory = std::unique_ptr<void, DeviceFree>;

class Scene
{
public:
	Scene() = default;
	// path: a .gltf / .glb file.  Below SceneParams::instance.modelsRoot its camera / lights come from the registry, as in the reference
	// (Scene.cpp:95,315); elsewhere (and for a ".gmesh" dump or the built-in "cornell") from the sibling "<name>.params" or the defaults.
	Scene(gmupt_device* device, const std::string& path);

	Scene(Scene&) = delete;
	Scene& operator=(const Scene&) = delete;
	Scene(Scene&& scene) = default;
	Scene& operator=(Scene&& scene) = default;

	void update(float dt);
	size_t lightCount() const { return mLightCount; }
	void setLights(const std::vector<Light>& lights); // GUI light editor: re-upload (Source/GUI.cpp:125-130)
	// moved geometry (an extension; the reference has none): new positions for ALL vertices (3 floats each, the count of the loaded mesh) and,
	// optionally, new normals -- into the mesh data, the vertex buffer and the normals inside the property buffer.  The tree keeps its
	// topology: call Renderer::refitScene() afterwards.  Throws std::runtime_error on a wrong count or a failed upload.
	// With Renderer::refitScene(.., smoothNormals = true) the normals are recomputed on the device and never read back: MeshData::normals
	// then holds the last host-given normals (those of the loader, or of the last call with `normals`), not the device's.
	void setVertices(const std::vector<float>& xyz, const std::vector<float>* normals = nullptr);
	// geometry beyond a refit (vertices that moved far, another triangle list): a new tree from the GPU LBVH builder (gmupt_lbvh_build,
	// include/gmupt.h "LBVH") over the device-resident vertex buffer.  indices: 3 per triangle into the loaded vertices, replacing the mesh's
	// list; nullptr keeps it.  The builder handle and the device copy of the indices / vertex materials are created on first use and kept.
	// The node and triangle buffers are replaced; the renderer still reads the old ones until it binds again, so call this through
	// Renderer::rebuildScene(), which does.  Throws std::runtime_error (a bad index, a non-finite used vertex, ...) and then keeps the tree, the buffers and the mesh's
	// triangle list as they were (only the internal device copy of the index list may hold the refused one; the next call uploads again).
	// optimizePasses > 0: the new tree goes through that many passes of the treelet optimiser on the device before it takes the place of the
	// old one (BVHWrapper::optimizeOnDevice, include/gmupt.h "Tree optimisation"; the optimiser handle is created on first use and kept);
	// *optimizeInfo (may be nullptr) then holds its info.  An optimiser error is thrown like a builder error: everything stays as it was.
	gmupt_lbvh_info rebuildOnDevice(unsigned maxLeafSize = 4, const std::vector<int32_t>* indices = nullptr, unsigned optimizePasses = 0,
	                                gmupt_treeopt_info* optimizeInfo = nullptr);
	// the rig of the loaded mesh (an extension; include/gmupt.h "Pose"): a ".grig" file -- "GRIG", then version (1), num_verts, influences,
	// num_joints, num_targets as little-endian uint32, then the arrays in the order of gmupt_pose_create: rest (3 floats per vertex), joints
	// (uint16) and weights (float), `influences` per vertex each and absent when num_joints is 0, deltas (3 floats per vertex and target).
	// Throws std::runtime_error on a file that is not one, a vertex count other than the mesh's, counts outside the rule's limits, a
	// length that does not match or a joint number outside the rig's joints behind a weight that is not zero.  Renderer::poseScene poses with it.
	struct Rig
	{
		uint32_t numVerts = 0, influences = 0, numJoints = 0, numTargets = 0;
		std::vector<float> rest, weights, deltas;
		std::vector<uint16_t> joints;
	};
	void loadRig(const std::string& path);
	const Rig* rig() const { return mRig.get(); }

private:
	void loadScene(const std::string& path);
	void createBVH();
	void loadTextures();
	void createTextures(struct gmupt::TextureSet set, Buffer& resource);
	void createPropertyBuffer(const std::vector<MaterialProperty>& data);
	void createLights(const std::vector<Light>& lights);

	gmupt_device* mDevice = nullptr;
	Camera mCamera;
	MeshData mScene;
	std::string mSceneName;

	Buffer mBVHBuffer;
	Buffer mIndexBuffer;
	Buffer mVertexBuffer;
	Buffer mTriangleProperties;
	Buffer mLightBuffer;
	Buffer mMaterialPropertyBuffer;
	Buffer mDiffuse, mMetallicRoughness, mNormal; // Texture2DArray t5..t7 (Include/Scene.hpp:108-110); null when the scene has none

	// rebuildOnDevice: the builder, its inputs on the device, and the tree the renderer is still bound to until Renderer::rebuildScene rebinds
	std::unique_ptr<gmupt_lbvh, LbvhDeleter> mLBVH;
	std::unique_ptr<gmupt_treeopt, TreeoptDeleter> mTreeopt;
	DeviceMemory mDeviceIndices, mDeviceVertexMaterial;
	size_t mDeviceIndexCapacity = 0;
	int mHipDevice = -1;                          // set by the Renderer that owns the scene: the device of rebuildOnDevice's own allocations
	Buffer mRetiredBVHBuffer, mRetiredIndexBuffer;
	std::unique_ptr<Rig> mRig;                    // loadRig

	std::array<Light, MAX_LIGHTS> mLights{};
	size_t mLightCount = 0;

	friend class Renderer;
};
