// DualContouring.h -- the reference's second surface extractor on the CPU (include/rto_hip.h, rto_extract_dual_contour; DESIGN.md
// section 32).  HermitePoint, QEFSolver and AdaptiveDualContouringRenderer carry the reference's names and signatures
// (453-skeleton/AdaptiveDualContouringRenderer.h:19-58, 61-102) for its deterministic pair: the per-voxel vertex rule
// (gatherHermiteData with size 1, calculateIntersection, generateDualVertex, QEFSolver) and the triangulation buildTrianglesCPU.
// render()'s top-level call runs that pair on the CPU.  There is no GL, no thread pool and no cache here; the adaptive
// createTriangles path and the shipped GLSL are out of scope, so a call of render() below the top level returns no triangle.
//
// dualContourVolume / dualVertexVolume are the CPU forms of the whole rule with its two options (the area rule and the clip box of
// cells), tri_cell and the summary; they call the arithmetic the kernels call (DualVertex.h).  float32, one IEEE operation per
// operator: the library is built with -ffp-contract=off.
#pragma once

#include <cstdint>
#include <vector>

#include "OctreeVoxel.h"
#include "Renderer.h"
#include "rto_hip.h"

namespace rtmath {
struct vec4 {
    float x = 0.f, y = 0.f, z = 0.f, w = 0.f;
    vec4() = default;
    vec4(float x_, float y_, float z_, float w_) : x(x_), y(y_), z(z_), w(w_) {}
};
}  // namespace rtmath

struct HermitePoint {
    rtmath::vec3 position;
    rtmath::vec3 normal;
};

class QEFSolver {
public:
    QEFSolver();
    void addPoint(const rtmath::vec3& point, const rtmath::vec3& normal);
    void clear();
    rtmath::vec3 solve(const rtmath::vec3& cellCenter, float cellSize);
    rtmath::vec3 solveConstrained(const rtmath::vec3& minBound, const rtmath::vec3& maxBound);

private:
    float ata[3][3];               // column, row: glm's indexing
    rtmath::vec3 atb;
    rtmath::vec3 pointSum;
    int numPoints;
};

class AdaptiveDualContouringRenderer : public Renderer {
public:
    // x0 = y0 = z0 = 0 and size == grid.dimX: one vertex per voxel, then buildTrianglesCPU.  Anything else: an empty list.
    std::vector<MCTriangle> render(const OctreeNode* node, const VoxelGrid& grid, int x0, int y0, int z0, int size) override;

    // allVerts: one per voxel, x fastest; w is not read.
    std::vector<MCTriangle> buildTrianglesCPU(const VoxelGrid& grid, const std::vector<rtmath::vec4>& allVerts);
    rtmath::vec3 gridToWorld(const VoxelGrid& grid, int x, int y, int z);
    std::vector<HermitePoint> gatherHermiteData(const VoxelGrid& grid, int x0, int y0, int z0, int size);
    rtmath::vec3 generateDualVertex(const std::vector<HermitePoint>& hermiteData, const rtmath::vec3& cellCenter, float cellSize);
    // grid-aligned neighbours with a sign change between them (what gatherHermiteData passes)
    HermitePoint calculateIntersection(const VoxelGrid& grid, int x1, int y1, int z1, int x2, int y2, int z2);
    // addition: the vertex of every voxel by the three functions above (w: the number of Hermite points)
    std::vector<rtmath::vec4> dualVertices(const VoxelGrid& grid);
};

// voxels: dimZ x dimY x dimX bytes, x fastest; a voxel is solid when it is FILLED (1).  The checks are the C ABI's (RTO_E_INVALID for
// an unknown area rule, reserved words or a bad clip box; RTO_E_UNSUPPORTED for more than 2^31 - 1 voxels: an empty list and *rc,
// when given, set to the code).  triCell and summary may be null.
std::vector<MCTriangle> dualContourVolume(const uint8_t* voxels, int dimX, int dimY, int dimZ, const rtmath::vec3& gridMin, float voxelSize,
                                          const rto_dc_params& params, std::vector<int32_t>* triCell = nullptr,
                                          rto_dc_summary* summary = nullptr, int* rc = nullptr);
// The vertex of every voxel, x fastest.
std::vector<rto_dual_vertex> dualVertexVolume(const uint8_t* voxels, int dimX, int dimY, int dimZ, const rtmath::vec3& gridMin, float voxelSize);
