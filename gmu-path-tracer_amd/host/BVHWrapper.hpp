// Same role and nested PODs as the reference's BVHWrapper (Include/BVHWrapper.hpp:10-51): turns the imported meshes into the
// flattened SBVH buffers the ray-cast kernels consume.  The aiScene input becomes MeshData; the vendored Nvidia-SBVH classes
// are replaced by gmupt::SbvhBuilder.
#pragma once
#include <vector>
#include "MeshData.hpp"

class BVHWrapper
{
public:
	using BVHNode = gmupt_bvh_node;                 // 48 B, Include/BVHWrapper.hpp:13-21
	using Triangle = gmupt_triangle;                // 16 B, :23-27
	using TriangleProperties = gmupt_tri_props;     // 32 B per vertex, :29-34

	// SBVH: the reference's builder (the default, and the one for offline builds).  LBVH: the linear BVH of include/gmupt.h "LBVH", here
	// through its host reference gmupt_lbvh_build_host -- the arrays Scene::rebuildOnDevice gets from the GPU, bit for bit.
	enum class Builder { SBVH, LBVH };

	// optimizePasses > 0 (LBVH only): that many passes of the treelet optimiser's host reference (gmupt_tree_optimize_host, include/gmupt.h
	// "Tree optimisation") on the built tree -- the nodes optimizeOnDevice gets from the GPU, bit for bit.  Throws std::runtime_error.
	BVHWrapper() = default;
	explicit BVHWrapper(const MeshData& scene, Builder builder = Builder::SBVH, unsigned maxLeafSize = 4, unsigned optimizePasses = 0);

	// The treelet optimiser on the device (gmupt_treeopt_run) for a node buffer that lives there, e.g. the one gmupt_lbvh_build returned:
	// a new node buffer of the same leaves, which the caller owns; `nodes` stays as it is and the triangle buffer stays valid.  Throws
	// std::runtime_error with gmupt_last_error (a tree deeper than 64 levels after a pass, ...) and then creates nothing.
	static gmupt_buffer* optimizeOnDevice(gmupt_treeopt* optimizer, const gmupt_buffer* nodes, unsigned passes, gmupt_treeopt_info* info = nullptr);
	const gmupt_treeopt_info& optimizeInfo() const { return mOptimizeInfo; } // of the constructor's passes; zeros without

	const std::vector<BVHNode>& tree() const { return mGPUTree; }
	const std::vector<Triangle>& indices() const { return mIndices; }
	const std::vector<TriangleProperties>& triangleProperties() const { return mTriangleProperties; }
	const std::vector<float>& vertices() const { return mVertices; }
	float sah() const { return mSAH; }                            // of the SBVH build; 0 after buildLBVH, which computes none
	const gmupt_lbvh_info& lbvhInfo() const { return mLBVHInfo; } // of buildLBVH; zeros after buildSBVH

private:
	void fillProperties(const MeshData& scene);
	void buildSBVH(const MeshData& scene);
	void buildLBVH(const MeshData& scene, unsigned maxLeafSize); // throws std::runtime_error with gmupt_last_error (rule 9 of the header)

	std::vector<BVHNode> mGPUTree;
	std::vector<Triangle> mIndices;
	std::vector<TriangleProperties> mTriangleProperties;
	std::vector<float> mVertices;
	float mSAH = 0.f;
	gmupt_lbvh_info mLBVHInfo{};
	gmupt_treeopt_info mOptimizeInfo{};

	friend class Scene;
};
