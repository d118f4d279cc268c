// Renderer.cpp -- MarchingCubesRenderer::render and VoxelCubeRenderer::render, behaviour of 453-skeleton/Renderer.cpp:14-168, and
// renderOctree, behaviour of the walk at 453-skeleton/main.cpp:123-189.
#include "Renderer.h"

#include "Frustum.h"

using rtmath::vec3;

std::vector<MCTriangle> MarchingCubesRenderer::render(const OctreeNode* node, const VoxelGrid& grid, int x0, int y0, int z0, int size) {
    std::vector<MCTriangle> out;
    if (!node) return out;
    if (node->isLeaf) return localMC(grid, x0, y0, z0, size);
    const int half = size / 2;
    for (int i = 0; i < 8; i++) {
        const std::vector<MCTriangle> sub = render(node->children[i], grid, x0 + ((i & 1) ? half : 0), y0 + ((i & 2) ? half : 0),
                                                   z0 + ((i & 4) ? half : 0), half);
        out.insert(out.end(), sub.begin(), sub.end());
    }
    return out;
}

std::vector<MCTriangle> VoxelCubeRenderer::render(const OctreeNode* node, const VoxelGrid& grid, int x0, int y0, int z0, int size) {
    std::vector<MCTriangle> out;
    if (!node) return out;
    if (node->isLeaf) {
        if (node->isSolid) addBlockFaces(grid, x0, y0, z0, size, out);
        return out;
    }
    const int half = size / 2;
    for (int i = 0; i < 8; i++) {
        const std::vector<MCTriangle> sub = render(node->children[i], grid, x0 + ((i & 1) ? half : 0), y0 + ((i & 2) ? half : 0),
                                                   z0 + ((i & 4) ? half : 0), half);
        out.insert(out.end(), sub.begin(), sub.end());
    }
    return out;
}

namespace {
// The four corners of a face in the reference's order (Renderer.cpp:100-153), bit a = the max corner's coordinate on axis a.
const int kFaceCorners[6][4] = { { 1, 3, 7, 5 }, { 0, 4, 6, 2 }, { 2, 6, 7, 3 }, { 0, 1, 5, 4 }, { 4, 6, 7, 5 }, { 0, 1, 3, 2 } };
const float kFaceNormals[6][3] = { { 1, 0, 0 }, { -1, 0, 0 }, { 0, 1, 0 }, { 0, -1, 0 }, { 0, 0, 1 }, { 0, 0, -1 } };

MCTriangle triangle_of(const vec3& a, const vec3& b, const vec3& c, const vec3& n) {
    MCTriangle t;
    t.v[0] = a; t.v[1] = b; t.v[2] = c;
    t.normal[0] = t.normal[1] = t.normal[2] = n;
    return t;
}
}  // namespace

// The centre-only exposure test is the reference's (Renderer.cpp:75-97): one voxel per face, x0 + size (or x0 - 1) on the face's
// axis and + size / 2 on the other two.
void VoxelCubeRenderer::addBlockFaces(const VoxelGrid& grid, int x0, int y0, int z0, int size, std::vector<MCTriangle>& out) {
    const float vs = grid.voxelSize;
    const vec3 lo(grid.minX + x0 * vs, grid.minY + y0 * vs, grid.minZ + z0 * vs);
    const vec3 hi = lo + vec3(size * vs);
    const int h = size / 2;
    const int tests[6][3] = { { x0 + size, y0 + h, z0 + h }, { x0 - 1, y0 + h, z0 + h }, { x0 + h, y0 + size, z0 + h },
                              { x0 + h, y0 - 1, z0 + h },    { x0 + h, y0 + h, z0 + size }, { x0 + h, y0 + h, z0 - 1 } };
    for (int f = 0; f < 6; f++) {
        const int tx = tests[f][0], ty = tests[f][1], tz = tests[f][2];
        const bool outside = tx < 0 || ty < 0 || tz < 0 || tx >= grid.dimX || ty >= grid.dimY || tz >= grid.dimZ;
        if (!outside && grid.data[(size_t)grid.index(tx, ty, tz)] != VoxelState::EMPTY) continue;
        vec3 v[4];
        for (int k = 0; k < 4; k++) {
            const int c = kFaceCorners[f][k];
            v[k] = vec3((c & 1) ? hi.x : lo.x, (c & 2) ? hi.y : lo.y, (c & 4) ? hi.z : lo.z);
        }
        const vec3 n(kFaceNormals[f][0], kFaceNormals[f][1], kFaceNormals[f][2]);
        out.push_back(triangle_of(v[0], v[1], v[3], n));
        out.push_back(triangle_of(v[3], v[1], v[2], n));
    }
}

namespace {
void walk(const OctreeNode* node, const VoxelGrid& grid, Renderer& renderer, const Frustum* frustum, float margin, std::vector<MCTriangle>& out) {
    if (!node) return;
    if (frustum) {
        const float vs = grid.voxelSize;
        const vec3 lo(grid.minX + node->x * vs, grid.minY + node->y * vs, grid.minZ + node->z * vs);
        const vec3 hi = lo + vec3(node->size * vs);
        if (frustum->testAABB(lo, hi, margin) == -1) return;
    }
    if (node->isLeaf) {
        const std::vector<MCTriangle> tris = renderer.render(node, grid, node->x, node->y, node->z, node->size);
        out.insert(out.end(), tris.begin(), tris.end());
        return;
    }
    for (const OctreeNode* child : node->children) walk(child, grid, renderer, frustum, margin, out);
}
}  // namespace

std::vector<MCTriangle> renderOctreePlanes(const OctreeNode* root, const VoxelGrid& grid, Renderer& renderer, const float* planes,
                                           float extraMargin) {
    std::vector<MCTriangle> out;
    if (planes) {
        const Frustum frustum = Frustum::fromPlanes(planes);
        walk(root, grid, renderer, &frustum, extraMargin, out);
    } else walk(root, grid, renderer, nullptr, extraMargin, out);
    return out;
}

std::vector<MCTriangle> renderOctree(const OctreeNode* root, const VoxelGrid& grid, Renderer& renderer, const Camera& camera, float aspect,
                                     float extraMargin) {
    const rtmath::mat4 proj = rtmath::perspective(rtmath::radians(45.f), aspect, 0.01f, 5000.f);
    const Frustum frustum(proj * camera.getView());
    std::vector<MCTriangle> out;
    walk(root, grid, renderer, &frustum, extraMargin, out);
    return out;
}
