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

	BVHWrapper() = default;
	explicit BVHWrapper(const MeshData& scene, Builder builder = Builder::SBVH, unsigned maxLeafSize = 4);

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

	friend class Scene;
};
