// Renderer.h -- the reference's mesh-extractor interface (453-skeleton/Renderer.h:10-55) and the walk that drives it
// (renderOctree, 453-skeleton/main.cpp:95-208): kept so that code written against them compiles.  MarchingCubesRenderer's
// triangles also feed the leaf-triangle ray path.  These are the CPU forms; RayTracerBVH::extractMesh makes the same lists on the
// GPU (rto_extract_mesh).  The reference's third renderer, AdaptiveDualContouringRenderer, is in
// DualContouring.h (RayTracerBVH::dualContour on the GPU).
#pragma once

#include <vector>

#include "Camera.h"
#include "OctreeVoxel.h"

class Renderer {
public:
    virtual std::vector<MCTriangle> render(const OctreeNode* node, const VoxelGrid& grid, int x0, int y0, int z0, int size) = 0;
    virtual ~Renderer() = default;
};

// localMC on every leaf below `node`, children in index order (453-skeleton/Renderer.cpp:14-36)
class MarchingCubesRenderer : public Renderer {
public:
    std::vector<MCTriangle> render(const OctreeNode* node, const VoxelGrid& grid, int x0, int y0, int z0, int size) override;
};

// A cube per solid leaf below `node`, children in index order; only the faces whose centre looks at an EMPTY voxel, or out of the
// grid, are emitted: +X, -X, +Y, -Y, +Z, -Z, two triangles each (453-skeleton/Renderer.cpp:40-168).
class VoxelCubeRenderer : public Renderer {
public:
    std::vector<MCTriangle> render(const OctreeNode* node, const VoxelGrid& grid, int x0, int y0, int z0, int size) override;

private:
    void addBlockFaces(const VoxelGrid& grid, int x0, int y0, int z0, int size, std::vector<MCTriangle>& out);
};

// The reference's walk without its dual-contouring cache parameters: depth first, a subtree is dropped when its box fails
// Frustum(perspective(radians(45), aspect, 0.01, 5000) * camera.getView()).testAABB(min, max, extraMargin); `renderer` runs on
// every leaf that is reached.
std::vector<MCTriangle> renderOctree(const OctreeNode* root, const VoxelGrid& grid, Renderer& renderer, const Camera& camera, float aspect,
                                     float extraMargin = 50.0f);
// addition: the same walk over caller-supplied planes (LEFT .. FAR as nx, ny, nz, d; normalised); planes == nullptr: nothing is culled
std::vector<MCTriangle> renderOctreePlanes(const OctreeNode* root, const VoxelGrid& grid, Renderer& renderer, const float* planes,
                                           float extraMargin);
