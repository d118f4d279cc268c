// MarchingCubes.cpp -- marchingCubesVolume with the semantics of 453-skeleton/MarchingCubes.cpp:544-689 (vertexInterp,
// marchingCubesCell, marchingCubesVolume), and isoSurfaceVolume, the field isosurface rule of DESIGN.md section 30 on the CPU.
#include "MarchingCubes.h"

#include <cmath>

#include "mc_cases.inc"

using rtmath::vec3;

namespace {

const int kCorner[8][3] = { { 0, 0, 0 }, { 1, 0, 0 }, { 1, 1, 0 }, { 0, 1, 0 }, { 0, 0, 1 }, { 1, 0, 1 }, { 1, 1, 1 }, { 0, 1, 1 } };

inline vec3 vertexInterp(float iso, const vec3& p1, const vec3& p2, float v1, float v2) {
    if (std::fabs(iso - v1) < 1e-6f) return p1;
    if (std::fabs(iso - v2) < 1e-6f) return p2;
    if (std::fabs(v1 - v2) < 1e-6f) return p1;
    const float mu = (iso - v1) / (v2 - v1);
    return p1 + mu * (p2 - p1);
}

inline int hexval(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

// marchingCubesCell: the triangles of one cell, in the table's order, without normals
template <class Emit>
void cellTriangles(const vec3 pos[8], const float val[8], float iso, Emit emit) {
    int cubeIndex = 0;
    for (int i = 0; i < 8; i++)
        if (val[i] < iso) cubeIndex |= 1 << i;
    for (const char* e = kMcCaseEdges[cubeIndex]; *e != 'f'; e += 3) {
        MCTriangle tri;
        for (int v = 0; v < 3; v++) {
            const int id = hexval(e[v]);
            const int a = edgeToCorner[id][0], b = edgeToCorner[id][1];
            tri.v[v] = vertexInterp(iso, pos[a], pos[b], val[a], val[b]);
        }
        emit(tri);
    }
}

}  // namespace

std::vector<MCTriangle> marchingCubesVolume(const float* scalarField, int dimX, int dimY, int dimZ, const vec3& origin, float spacing, float isoValue) {
    std::vector<MCTriangle> triangles;
    for (int z = 0; z < dimZ - 1; z++)
        for (int y = 0; y < dimY - 1; y++)
            for (int x = 0; x < dimX - 1; x++) {
                vec3 pos[8];
                float val[8];
                for (int i = 0; i < 8; i++) {
                    const int cx = x + kCorner[i][0], cy = y + kCorner[i][1], cz = z + kCorner[i][2];
                    pos[i] = origin + vec3((float)cx, (float)cy, (float)cz) * spacing;
                    val[i] = scalarField[(size_t)cx + (size_t)cy * dimX + (size_t)cz * dimX * dimY];
                }
                cellTriangles(pos, val, isoValue, [&](MCTriangle& t) {
                    t.normal[0] = t.normal[1] = t.normal[2] = vec3(0.0f, 1.0f, 0.0f);      // the reference's placeholder
                    triangles.push_back(t);
                });
            }
    return triangles;
}

std::vector<MCTriangle> isoSurfaceVolume(const int32_t* volume, int dimX, int dimY, int dimZ, const vec3& gridMin, float voxelSize,
                                         const rto_iso_params& p, std::vector<int32_t>* triCell, rto_iso_summary* summary, int* rc) {
    std::vector<MCTriangle> triangles;
    if (triCell) triCell->clear();
    if (summary) *summary = rto_iso_summary{ 0, 0, 0, 0 };
    const int dim[3] = { dimX, dimY, dimZ };
    bool ok = volume && dimX > 0 && dimY > 0 && dimZ > 0 && p.valid_lo <= p.valid_hi && p.valid_lo > RTO_FIELD_PIXEL_NONE &&
              std::isfinite(p.level) && std::isfinite(p.outside) && (p.pad == 0 || p.pad == 1) &&
              ((int64_t)dimX + 1) * ((int64_t)dimY + 1) * ((int64_t)dimZ + 1) < 0x80000000ll;
    for (int r : p.reserved) ok = ok && r == 0;
    int lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
        lo[a] = p.clip ? p.clip_lo[a] : 0;
        hi[a] = p.clip ? p.clip_hi[a] : dim[a];
        ok = ok && lo[a] >= 0 && hi[a] <= dim[a] && lo[a] < hi[a];
    }
    if (rc) *rc = ok ? RTO_OK : RTO_E_INVALID;
    if (!ok) return triangles;

    const vec3 origin(gridMin.x + 0.5f * voxelSize, gridMin.y + 0.5f * voxelSize, gridMin.z + 0.5f * voxelSize);
    auto sample = [&](int x, int y, int z) -> float {
        if (x < lo[0] || x >= hi[0] || y < lo[1] || y >= hi[1] || z < lo[2] || z >= hi[2]) return p.outside;
        const int32_t v = volume[(size_t)x + (size_t)y * dimX + (size_t)z * dimX * dimY];
        return v >= p.valid_lo && v <= p.valid_hi ? (float)v : p.outside;
    };
    int64_t active = 0, degenerate = 0;
    for (int z = lo[2] - p.pad; z < hi[2] - 1 + p.pad; z++)
        for (int y = lo[1] - p.pad; y < hi[1] - 1 + p.pad; y++)
            for (int x = lo[0] - p.pad; x < hi[0] - 1 + p.pad; x++) {
                vec3 pos[8];
                float val[8];
                for (int i = 0; i < 8; i++) {
                    const int cx = x + kCorner[i][0], cy = y + kCorner[i][1], cz = z + kCorner[i][2];
                    pos[i] = origin + vec3((float)cx, (float)cy, (float)cz) * voxelSize;
                    val[i] = sample(cx, cy, cz);
                }
                const size_t before = triangles.size();
                cellTriangles(pos, val, p.level, [&](MCTriangle& t) {
                    const vec3 n = rtmath::cross(t.v[1] - t.v[0], t.v[2] - t.v[0]);
                    const float l2 = rtmath::dot(n, n);
                    vec3 unit(0.0f, 0.0f, 0.0f);
                    if (l2 > 0.0f && std::isfinite(l2)) unit = n * rtmath::inversesqrt(l2);
                    else degenerate++;
                    t.normal[0] = t.normal[1] = t.normal[2] = unit;
                    triangles.push_back(t);
                    if (triCell) triCell->push_back((int32_t)(((int64_t)(z + 1) * (dimY + 1) + (y + 1)) * (dimX + 1) + (x + 1)));
                });
                if (triangles.size() != before) active++;
            }
    if (summary) *summary = rto_iso_summary{ (int64_t)triangles.size(), active, degenerate, 0 };
    return triangles;
}
