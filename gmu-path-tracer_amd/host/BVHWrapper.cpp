#include "BVHWrapper.hpp"
#include "sbvh_builder.hpp"
#include <cstring>
#include <stdexcept>

BVHWrapper::BVHWrapper(const MeshData& scene, Builder builder, unsigned maxLeafSize, unsigned optimizePasses)
{
	if (optimizePasses && builder != Builder::LBVH) throw std::runtime_error("BVHWrapper: the treelet optimiser goes with the LBVH builder");
	if (builder == Builder::LBVH) buildLBVH(scene, maxLeafSize); else buildSBVH(scene);
	if (optimizePasses)
	{
		gmupt_treeopt_params params;
		gmupt_treeopt_default_params(&params);
		params.passes = optimizePasses;
		std::vector<BVHNode> better(mGPUTree.size());
		if (gmupt_tree_optimize_host(mGPUTree.data(), static_cast<uint32_t>(mGPUTree.size()), &params, better.data(), &mOptimizeInfo) != GMUPT_OK)
			throw std::runtime_error(gmupt_last_error());
		mGPUTree.swap(better);
	}
}

gmupt_buffer* BVHWrapper::optimizeOnDevice(gmupt_treeopt* optimizer, const gmupt_buffer* nodes, unsigned passes, gmupt_treeopt_info* info)
{
	gmupt_treeopt_params params;
	gmupt_treeopt_default_params(&params);
	params.passes = passes;
	gmupt_buffer* better = nullptr;
	if (gmupt_treeopt_run(optimizer, nodes, &params, &better, info) != GMUPT_OK) throw std::runtime_error(gmupt_last_error());
	return better;
}

void BVHWrapper::fillProperties(const MeshData& scene)
{
	mVertices = scene.vertices;

	// one TriangleProperties per vertex (Source/BVHWrapper.cpp:30-37)
	mTriangleProperties.resize(scene.numVertices());
	for (size_t n = 0; n < scene.numVertices(); n++)
	{
		auto& p = mTriangleProperties[n];
		std::memset(&p, 0, sizeof(p));
		for (int k = 0; k < 3; k++) p.normal[k] = scene.normals[3 * n + k];
		if (!scene.texCoords.empty()) { p.uv[0] = scene.texCoords[2 * n]; p.uv[1] = scene.texCoords[2 * n + 1]; }
		p.materialID = scene.vertexMaterial[n];
	}
}

void BVHWrapper::buildSBVH(const MeshData& scene)
{
	fillProperties(scene);

	gmupt_sbvh_params params;
	gmupt_sbvh_default_params(&params); // default Platform / BuildParams of Source/BVHWrapper.cpp:52-54
	gmupt::SbvhBuilder builder(mVertices.data(), static_cast<uint32_t>(scene.numVertices()), scene.indices.data(),
	                           static_cast<uint32_t>(scene.numTriangles()), params);
	builder.build();
	mSAH = builder.sah();

	mGPUTree.resize(builder.numNodes());
	mIndices.resize(builder.numReferences());
	builder.flatten(scene.vertexMaterial.data(), mGPUTree.data(), mIndices.data(), nullptr);
}

void BVHWrapper::buildLBVH(const MeshData& scene, unsigned maxLeafSize)
{
	fillProperties(scene);

	gmupt_lbvh_params params;
	gmupt_lbvh_default_params(&params);
	params.max_leaf_size = maxLeafSize;
	const size_t n = scene.numTriangles();
	mGPUTree.assign(n ? 2 * n - 1 : 0, BVHNode{});
	mIndices.assign(n, Triangle{});
	if (gmupt_lbvh_build_host(mVertices.data(), static_cast<uint32_t>(scene.numVertices()), scene.indices.data(), static_cast<uint32_t>(n),
	                          scene.vertexMaterial.data(), &params, mGPUTree.data(), mIndices.data(), nullptr, &mLBVHInfo) != GMUPT_OK)
		throw std::runtime_error(gmupt_last_error());
	mGPUTree.resize(mLBVHInfo.num_nodes);
	mSAH = 0.f;
}
