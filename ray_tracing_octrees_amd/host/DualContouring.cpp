// DualContouring.cpp -- see DualContouring.h.  Two forms of one rule:
//   * the reference's own shape: the Hermite points of a voxel stored in a vector, QEFSolver as a class, buildTrianglesCPU over a
//     vertex per voxel.  It keeps the branches no input can take (|det| < 1e-10, a bad entry of the inverse);
//   * dualContourVolume / dualVertexVolume: the arithmetic the kernels run (DualVertex.h), which walks the points twice instead of
//     storing them, with the area rule, the clip box, tri_cell and the summary.
// tests/test_dual_contour.py and tools/dc_selftest.cpp hold the two against each other, byte for byte.
#include "DualContouring.h"

#include <algorithm>
#include <cmath>

#include "DualVertex.h"

using rtmath::vec3;
using rtmath::vec4;

namespace {

inline bool solidAt(const VoxelGrid& grid, int x, int y, int z) {
    if (x < 0 || y < 0 || z < 0 || x >= grid.dimX || y >= grid.dimY || z >= grid.dimZ) return false;
    return grid.data[(size_t)x + (size_t)y * (size_t)grid.dimX + (size_t)z * ((size_t)grid.dimX * (size_t)grid.dimY)] == VoxelState::FILLED;
}
inline vec3 divide(const vec3& v, float s) { return vec3(v.x / s, v.y / s, v.z / s); }
inline float minf(float x, float y) { return y < x ? y : x; }
inline float maxf(float x, float y) { return x < y ? y : x; }
inline vec3 clampv(const vec3& v, const vec3& lo, const vec3& hi) {
    return vec3(minf(maxf(v.x, lo.x), hi.x), minf(maxf(v.y, lo.y), hi.y), minf(maxf(v.z, lo.z), hi.z));
}
inline vec3 mixv(const vec3& x, const vec3& y, float a) { return x * (1.0f - a) + y * a; }

}  // namespace

// ---------------------------------------------------------------- QEFSolver
QEFSolver::QEFSolver() { clear(); }

void QEFSolver::clear() {
    for (auto& col : ata) for (float& v : col) v = 0.0f;
    atb = vec3(0.0f, 0.0f, 0.0f);
    pointSum = vec3(0.0f, 0.0f, 0.0f);
    numPoints = 0;
}

void QEFSolver::addPoint(const vec3& point, const vec3& normal) {
    const vec3 n = rtmath::normalize(normal);
    for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) ata[c][r] += n[c] * n[r];
    const float d = -rtmath::dot(n, point);
    atb.x += n.x * d; atb.y += n.y * d; atb.z += n.z * d;
    pointSum += point;
    numPoints++;
}

vec3 QEFSolver::solve(const vec3& cellCenter, float cellSize) {
    const vec3 masspoint = numPoints > 0 ? divide(pointSum, static_cast<float>(numPoints)) : cellCenter;
    if (numPoints <= 2) return masspoint;
    float m[3][3];
    for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) m[c][r] = ata[c][r];
    m[0][0] += 0.3f; m[1][1] += 0.3f; m[2][2] += 0.3f;
    const float det = m[0][0] * (m[1][1] * m[2][2] - m[2][1] * m[1][2]) - m[1][0] * (m[0][1] * m[2][2] - m[2][1] * m[0][2]) +
                      m[2][0] * (m[0][1] * m[1][2] - m[1][1] * m[0][2]);
    bool invertible = true;
    float inv[3][3] = {};
    if (std::abs(det) < 1e-10) invertible = false;      // cannot be taken: AtA + 0.3 I has determinant >= 0.027
    else {
        const float ood = 1.0f / det;                   // glm::inverse forms the same determinant again
        inv[0][0] = (m[1][1] * m[2][2] - m[2][1] * m[1][2]) * ood;
        inv[1][0] = -(m[1][0] * m[2][2] - m[2][0] * m[1][2]) * ood;
        inv[2][0] = (m[1][0] * m[2][1] - m[2][0] * m[1][1]) * ood;
        inv[0][1] = -(m[0][1] * m[2][2] - m[2][1] * m[0][2]) * ood;
        inv[1][1] = (m[0][0] * m[2][2] - m[2][0] * m[0][2]) * ood;
        inv[2][1] = -(m[0][0] * m[2][1] - m[2][0] * m[0][1]) * ood;
        inv[0][2] = (m[0][1] * m[1][2] - m[1][1] * m[0][2]) * ood;
        inv[1][2] = -(m[0][0] * m[1][2] - m[1][0] * m[0][2]) * ood;
        inv[2][2] = (m[0][0] * m[1][1] - m[1][0] * m[0][1]) * ood;
        for (int i = 0; i < 3 && invertible; i++)
            for (int j = 0; j < 3 && invertible; j++)
                if (std::isnan(inv[i][j]) || std::isinf(inv[i][j]) || std::abs(inv[i][j]) > 1e6) invertible = false;      // nor this
    }
    if (invertible) {
        vec3 solution(inv[0][0] * atb.x + inv[1][0] * atb.y + inv[2][0] * atb.z, inv[0][1] * atb.x + inv[1][1] * atb.y + inv[2][1] * atb.z,
                      inv[0][2] * atb.x + inv[1][2] * atb.y + inv[2][2] * atb.z);
        solution = masspoint + 0.7f * (solution - masspoint);
        if (!std::isnan(solution.x) && !std::isnan(solution.y) && !std::isnan(solution.z)) {
            const vec3 d = masspoint - solution;
            if (rtmath::dot(d, d) < cellSize * cellSize) return mixv(solution, masspoint, 0.2f);
        }
    }
    return masspoint;
}

vec3 QEFSolver::solveConstrained(const vec3& minBound, const vec3& maxBound) {
    const vec3 cellCenter = (minBound + maxBound) * 0.5f;
    const float cellSize = maxBound.x - minBound.x;
    return clampv(solve(cellCenter, cellSize), minBound, maxBound);
}

// ---------------------------------------------------------------- AdaptiveDualContouringRenderer
vec3 AdaptiveDualContouringRenderer::gridToWorld(const VoxelGrid& grid, int x, int y, int z) {
    return vec3(grid.minX + (float)x * grid.voxelSize, grid.minY + (float)y * grid.voxelSize, grid.minZ + (float)z * grid.voxelSize);
}

HermitePoint AdaptiveDualContouringRenderer::calculateIntersection(const VoxelGrid& grid, int x1, int y1, int z1, int x2, int y2, int z2) {
    const bool filled2 = solidAt(grid, x2, y2, z2);
    const vec3 p1 = gridToWorld(grid, x1, y1, z1), p2 = gridToWorld(grid, x2, y2, z2);
    HermitePoint hp;
    hp.position = p1 + 0.5f * (p2 - p1);                 // t = v1 / (v1 - v2) with v = +-1
    const int dx = x2 - x1, dy = y2 - y1, dz = z2 - z1;
    auto scalar = [&](int x, int y, int z) { return solidAt(grid, x, y, z) ? -1.0f : 1.0f; };
    vec3 normal;
    if (dx != 0) normal = vec3(0.0f, scalar(x1, y1 + 1, z1) - scalar(x1, y1 - 1, z1), scalar(x1, y1, z1 + 1) - scalar(x1, y1, z1 - 1));
    else if (dy != 0) normal = vec3(scalar(x1 + 1, y1, z1) - scalar(x1 - 1, y1, z1), 0.0f, scalar(x1, y1, z1 + 1) - scalar(x1, y1, z1 - 1));
    else normal = vec3(scalar(x1 + 1, y1, z1) - scalar(x1 - 1, y1, z1), scalar(x1, y1 + 1, z1) - scalar(x1, y1 - 1, z1), 0.0f);
    if (rtmath::dot(normal, normal) < 1e-10) normal = vec3((float)dx, (float)dy, (float)dz);
    else normal = rtmath::normalize(normal);
    const float along = normal.x * (float)dx + normal.y * (float)dy + normal.z * (float)dz;
    if ((along > 0) == filled2) normal = -normal;
    hp.normal = normal;
    return hp;
}

std::vector<HermitePoint> AdaptiveDualContouringRenderer::gatherHermiteData(const VoxelGrid& grid, int x0, int y0, int z0, int size) {
    const int maxX = std::min(x0 + size, grid.dimX - 1), maxY = std::min(y0 + size, grid.dimY - 1), maxZ = std::min(z0 + size, grid.dimZ - 1);
    const int minX = std::max(x0, 0), minY = std::max(y0, 0), minZ = std::max(z0, 0);
    const int stride = size > 8 ? 2 : 1;
    std::vector<HermitePoint> points;
    for (int z = minZ; z <= maxZ; z += stride)
        for (int y = minY; y <= maxY; y += stride)
            for (int x = minX; x <= maxX; x += stride) {
                const bool cur = solidAt(grid, x, y, z);
                for (int d = 0; d < 3; d++) {
                    const int nx = x + (d == 0), ny = y + (d == 1), nz = z + (d == 2);
                    if (nx >= grid.dimX || ny >= grid.dimY || nz >= grid.dimZ) continue;
                    if (cur != solidAt(grid, nx, ny, nz)) points.push_back(calculateIntersection(grid, x, y, z, nx, ny, nz));
                }
            }
    return points;
}

vec3 AdaptiveDualContouringRenderer::generateDualVertex(const std::vector<HermitePoint>& hermiteData, const vec3& cellCenter, float cellSize) {
    if (hermiteData.empty()) return cellCenter;
    const float half = cellSize * 0.5f, inset = cellSize * 0.001f;
    vec3 minBound = cellCenter - vec3(half, half, half), maxBound = cellCenter + vec3(half, half, half);
    minBound += vec3(inset, inset, inset);
    maxBound -= vec3(inset, inset, inset);
    vec3 massPoint;
    for (const HermitePoint& hp : hermiteData) massPoint += hp.position;
    massPoint = divide(massPoint, float(hermiteData.size()));
    vec3 avgNormal;
    for (const HermitePoint& hp : hermiteData) avgNormal += hp.normal;
    if (rtmath::length(avgNormal) > 0.0001f) {
        avgNormal = rtmath::normalize(avgNormal);
        const vec3 a(std::fabs(avgNormal.x), std::fabs(avgNormal.y), std::fabs(avgNormal.z));
        const float maxComp = std::max(std::max(a.x, a.y), a.z);
        if (maxComp > 0.85f) {
            if (a.x == maxComp) avgNormal = vec3(avgNormal.x > 0 ? 1.0f : -1.0f, 0.0f, 0.0f);
            else if (a.y == maxComp) avgNormal = vec3(0.0f, avgNormal.y > 0 ? 1.0f : -1.0f, 0.0f);
            else avgNormal = vec3(0.0f, 0.0f, avgNormal.z > 0 ? 1.0f : -1.0f);
            vec3 planePoint;
            int planePointCount = 0;
            for (const HermitePoint& hp : hermiteData)
                if (rtmath::dot(rtmath::normalize(hp.normal), avgNormal) > 0.7f) {
                    planePoint += hp.position;
                    planePointCount++;
                }
            if (planePointCount > 0) {
                planePoint = divide(planePoint, float(planePointCount));
                const float d = -rtmath::dot(avgNormal, planePoint);
                const float t = -(rtmath::dot(avgNormal, cellCenter) + d);
                return clampv(cellCenter + t * avgNormal, minBound, maxBound);
            }
        }
    }
    QEFSolver qef;
    for (const HermitePoint& hp : hermiteData) qef.addPoint(hp.position, hp.normal);
    return mixv(qef.solveConstrained(minBound, maxBound), massPoint, 0.1f);
}

std::vector<vec4> AdaptiveDualContouringRenderer::dualVertices(const VoxelGrid& grid) {
    std::vector<vec4> verts((size_t)grid.dimX * (size_t)grid.dimY * (size_t)grid.dimZ);
    size_t i = 0;
    for (int z = 0; z < grid.dimZ; z++)
        for (int y = 0; y < grid.dimY; y++)
            for (int x = 0; x < grid.dimX; x++, i++) {
                const std::vector<HermitePoint> points = gatherHermiteData(grid, x, y, z, 1);
                const vec3 corner = gridToWorld(grid, x, y, z);
                const float h = 0.5f * grid.voxelSize;
                const vec3 v = generateDualVertex(points, vec3(corner.x + h, corner.y + h, corner.z + h), grid.voxelSize);
                verts[i] = vec4(v.x, v.y, v.z, (float)points.size());
            }
    return verts;
}

std::vector<MCTriangle> AdaptiveDualContouringRenderer::buildTrianglesCPU(const VoxelGrid& grid, const std::vector<vec4>& allVerts) {
    std::vector<MCTriangle> out;
    auto vertex = [&](int x, int y, int z) {
        const vec4& v = allVerts[(size_t)x + (size_t)y * (size_t)grid.dimX + (size_t)z * ((size_t)grid.dimX * (size_t)grid.dimY)];
        return vec3(v.x, v.y, v.z);
    };
    auto addTri = [&](const vec3& a, const vec3& b, const vec3& c, bool invert) {
        const vec3 cr = rtmath::cross(b - a, c - a);
        vec3 n = rtmath::normalize(cr);
        if (invert) n = -n;
        if (0.5f * rtmath::length(cr) > 1e-6) {
            MCTriangle t;
            t.v[0] = a; t.v[1] = b; t.v[2] = c;
            t.normal[0] = t.normal[1] = t.normal[2] = n;
            out.push_back(t);
        }
    };
    auto addQuad = [&](const vec3& V00, const vec3& V01, const vec3& V11, const vec3& V10, bool invert) {
        addTri(V00, V01, V11, invert);
        addTri(V00, V11, V10, invert);
    };
    for (int z = 0; z < grid.dimZ - 1; z++)
        for (int y = 0; y < grid.dimY - 1; y++)
            for (int x = 0; x < grid.dimX - 1; x++) {
                const bool c = solidAt(grid, x, y, z);
                if (c != solidAt(grid, x + 1, y, z)) addQuad(vertex(x, y, z), vertex(x, y + 1, z), vertex(x + 1, y + 1, z), vertex(x + 1, y, z), c);
                if (c != solidAt(grid, x, y + 1, z)) addQuad(vertex(x, y, z), vertex(x + 1, y, z), vertex(x + 1, y + 1, z), vertex(x, y + 1, z), c);
                if (c != solidAt(grid, x, y, z + 1)) addQuad(vertex(x, y, z), vertex(x, y + 1, z), vertex(x, y + 1, z + 1), vertex(x, y, z + 1), c);
            }
    return out;
}

std::vector<MCTriangle> AdaptiveDualContouringRenderer::render(const OctreeNode*, const VoxelGrid& grid, int x0, int y0, int z0, int size) {
    if (x0 != 0 || y0 != 0 || z0 != 0 || size != grid.dimX) return {};
    return buildTrianglesCPU(grid, dualVertices(grid));
}

// ---------------------------------------------------------------- the CPU form of the whole rule
namespace {

struct SolidBytes {
    const uint8_t* v;
    int dx, dy, dz;
    bool operator()(int x, int y, int z) const {
        if (x < 0 || y < 0 || z < 0 || x >= dx || y >= dy || z >= dz) return false;
        return v[((size_t)z * (size_t)dy + (size_t)y) * (size_t)dx + (size_t)x] == 1;
    }
};

int checkParams(const rto_dc_params& p, int dimX, int dimY, int dimZ) {
    if (p.area_rule != RTO_DC_AREA_REFERENCE && p.area_rule != RTO_DC_AREA_NONE) return RTO_E_INVALID;
    for (int r : p.reserved) if (r != 0) return RTO_E_INVALID;
    if (dimX <= 0 || dimY <= 0 || dimZ <= 0) return RTO_E_INVALID;
    if ((int64_t)dimX * dimY * dimZ > 0x7fffffffll) return RTO_E_UNSUPPORTED;
    if (p.clip) {
        const int dim[3] = { dimX, dimY, dimZ };
        for (int a = 0; a < 3; a++)
            if (p.clip_lo[a] < 0 || p.clip_hi[a] > dim[a] || p.clip_lo[a] >= p.clip_hi[a]) return RTO_E_INVALID;
    }
    return RTO_OK;
}

}  // namespace

std::vector<rto_dual_vertex> dualVertexVolume(const uint8_t* voxels, int dimX, int dimY, int dimZ, const vec3& gridMin, float voxelSize) {
    const SolidBytes solid{ voxels, dimX, dimY, dimZ };
    const rto_dc::Grid g{ dimX, dimY, dimZ, gridMin.x, gridMin.y, gridMin.z, voxelSize };
    std::vector<rto_dual_vertex> out((size_t)dimX * (size_t)dimY * (size_t)dimZ);
    size_t i = 0;
    for (int z = 0; z < dimZ; z++)
        for (int y = 0; y < dimY; y++)
            for (int x = 0; x < dimX; x++, i++) {
                rto_dc::V3 v;
                out[i].points = rto_dc::vertex(solid, g, x, y, z, &v);
                out[i].p[0] = v.x; out[i].p[1] = v.y; out[i].p[2] = v.z;
            }
    return out;
}

std::vector<MCTriangle> dualContourVolume(const uint8_t* voxels, int dimX, int dimY, int dimZ, const vec3& gridMin, float voxelSize,
                                          const rto_dc_params& params, std::vector<int32_t>* triCell, rto_dc_summary* summary, int* rc) {
    std::vector<MCTriangle> out;
    if (triCell) triCell->clear();
    if (summary) *summary = rto_dc_summary{};
    const int code = checkParams(params, dimX, dimY, dimZ);
    if (rc) *rc = code;
    if (code != RTO_OK) return out;
    const SolidBytes solid{ voxels, dimX, dimY, dimZ };
    const rto_dc::Grid g{ dimX, dimY, dimZ, gridMin.x, gridMin.y, gridMin.z, voxelSize };
    const int dim[3] = { dimX, dimY, dimZ };
    int lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
        lo[a] = params.clip ? params.clip_lo[a] : 0;
        hi[a] = std::min(params.clip ? params.clip_hi[a] : dim[a], dim[a] - 1);
    }
    int64_t faces = 0, dropped = 0, degenerate = 0, withPoints = 0;
    std::vector<bool> seen;                              // voxels whose vertex a face has read
    if (summary) seen.assign((size_t)dimX * (size_t)dimY * (size_t)dimZ, false);
    for (int z = lo[2]; z < hi[2]; z++)
        for (int y = lo[1]; y < hi[1]; y++)
            for (int x = lo[0]; x < hi[0]; x++) {
                const bool c = solid(x, y, z);
                for (int axis = 0; axis < 3; axis++) {
                    if (c == solid(x + (axis == 0), y + (axis == 1), z + (axis == 2))) continue;
                    faces++;
                    rto_dc::V3 q[4];
                    for (int k = 0; k < 4; k++) {
                        const int o = rto_dc::face_corner(axis, k);
                        const int vx = x + (o & 1), vy = y + ((o >> 1) & 1), vz = z + ((o >> 2) & 1);
                        const int points = rto_dc::vertex(solid, g, vx, vy, vz, &q[k]);
                        if (summary) {
                            const size_t i = ((size_t)vz * (size_t)dimY + (size_t)vy) * (size_t)dimX + (size_t)vx;
                            if (!seen[i]) { seen[i] = true; withPoints += points > 0 ? 1 : 0; }
                        }
                    }
                    for (int t = 0; t < 2; t++) {
                        const rto_dc::V3 a = q[0], b = q[1 + t], d = q[2 + t];
                        rto_dc::V3 n;
                        float l2;
                        const bool fine = rto_dc::triangle_normal(a, b, d, c, &n, &l2);
                        if (params.area_rule == RTO_DC_AREA_REFERENCE && !rto_dc::area_kept(l2)) { dropped++; continue; }
                        if (!fine) degenerate++;
                        MCTriangle tri;
                        tri.v[0] = vec3(a.x, a.y, a.z); tri.v[1] = vec3(b.x, b.y, b.z); tri.v[2] = vec3(d.x, d.y, d.z);
                        tri.normal[0] = tri.normal[1] = tri.normal[2] = vec3(n.x, n.y, n.z);
                        out.push_back(tri);
                        if (triCell) triCell->push_back((z * dimY + y) * dimX + x);
                    }
                }
            }
    if (summary) {
        summary->faces = faces; summary->triangles = (int64_t)out.size(); summary->dropped = dropped;
        summary->degenerate = degenerate; summary->vertex_voxels = withPoints; summary->reserved = 0;
    }
    return out;
}
