// dc_selftest.cpp -- a stand-alone check of the CPU form of dual contouring (host/DualContouring.h) under the
// sanitizers.  Build and run from the repository root:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iray_tracing_octrees_amd/host tools/dc_selftest.cpp ray_tracing_octrees_amd/host/DualContouring.cpp -o dc_selftest
//   ./dc_selftest [grids, default 300]
//
// On a few hundred random grids (every dimension 1 .. 9, any density, both area rules, with and without a clip box of cells) it holds
// dualContourVolume -- records, tri_cell and summary -- against a plain loop of its own that restates the triangulation over a
// vertex per voxel made by the shared vertex function (DualVertex.h), and AdaptiveDualContouringRenderer::render, the reference's
// own shape with its points stored, against both.  Prints "ok" and returns 0, or says what differs and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "DualContouring.h"
#include "DualVertex.h"

namespace {

struct Solid {
    const std::vector<uint8_t>& v;
    int dx, dy, dz;
    bool operator()(int x, int y, int z) const {
        if (x < 0 || y < 0 || z < 0 || x >= dx || y >= dy || z >= dz) return false;
        return v[((size_t)z * dy + y) * dx + x] == 1;
    }
};

struct Expect {
    std::vector<float> rec;              // 12 per triangle
    std::vector<int32_t> cell;
    rto_dc_summary s{};
};

// The triangulation, restated: cells z slowest, faces +X +Y +Z, V00 V01 V11 V10, two triangles, the area rule.
Expect plainLoop(const std::vector<uint8_t>& vox, int dx, int dy, int dz, const float gmin[3], float vs, const rto_dc_params& p) {
    const Solid solid{ vox, dx, dy, dz };
    const rto_dc::Grid g{ dx, dy, dz, gmin[0], gmin[1], gmin[2], vs };
    std::vector<rto_dc::V3> vert((size_t)dx * dy * dz);
    std::vector<int> points(vert.size());
    for (int z = 0; z < dz; z++)
        for (int y = 0; y < dy; y++)
            for (int x = 0; x < dx; x++) points[((size_t)z * dy + y) * dx + x] = rto_dc::vertex(solid, g, x, y, z, &vert[((size_t)z * dy + y) * dx + x]);
    std::vector<char> seen(vert.size(), 0);
    Expect e;
    const int dim[3] = { dx, dy, dz };
    int lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
        lo[a] = p.clip ? p.clip_lo[a] : 0;
        hi[a] = p.clip ? p.clip_hi[a] : dim[a];
        if (hi[a] > dim[a] - 1) hi[a] = dim[a] - 1;
    }
    static const int corner[3][4][3] = { { { 0, 0, 0 }, { 0, 1, 0 }, { 1, 1, 0 }, { 1, 0, 0 } },
                                         { { 0, 0, 0 }, { 1, 0, 0 }, { 1, 1, 0 }, { 0, 1, 0 } },
                                         { { 0, 0, 0 }, { 0, 1, 0 }, { 0, 1, 1 }, { 0, 0, 1 } } };
    for (int z = lo[2]; z < hi[2]; z++)
        for (int y = lo[1]; y < hi[1]; y++)
            for (int x = lo[0]; x < hi[0]; x++)
                for (int axis = 0; axis < 3; axis++) {
                    const bool c = solid(x, y, z);
                    if (c == solid(x + (axis == 0), y + (axis == 1), z + (axis == 2))) continue;
                    e.s.faces++;
                    rto_dc::V3 q[4];
                    for (int k = 0; k < 4; k++) {
                        const size_t i = ((size_t)(z + corner[axis][k][2]) * dy + (y + corner[axis][k][1])) * dx + (x + corner[axis][k][0]);
                        q[k] = vert[i];
                        if (!seen[i]) { seen[i] = 1; e.s.vertex_voxels += points[i] > 0; }
                    }
                    const int order[2][3] = { { 0, 1, 2 }, { 0, 2, 3 } };
                    for (const auto& t : order) {
                        rto_dc::V3 n;
                        float l2;
                        const bool fine = rto_dc::triangle_normal(q[t[0]], q[t[1]], q[t[2]], c, &n, &l2);
                        if (p.area_rule == RTO_DC_AREA_REFERENCE && !((double)(0.5f * sqrtf(l2)) > 1e-6)) { e.s.dropped++; continue; }
                        e.s.degenerate += fine ? 0 : 1;
                        for (int k = 0; k < 3; k++) { e.rec.push_back(q[t[k]].x); e.rec.push_back(q[t[k]].y); e.rec.push_back(q[t[k]].z); }
                        e.rec.push_back(n.x); e.rec.push_back(n.y); e.rec.push_back(n.z);
                        e.cell.push_back((z * dy + y) * dx + x);
                    }
                }
    e.s.triangles = (int64_t)e.cell.size();
    return e;
}

std::vector<float> records(const std::vector<MCTriangle>& tris) {
    std::vector<float> r;
    for (const MCTriangle& t : tris) {
        for (int v = 0; v < 3; v++) { r.push_back(t.v[v].x); r.push_back(t.v[v].y); r.push_back(t.v[v].z); }
        r.push_back(t.normal[0].x); r.push_back(t.normal[0].y); r.push_back(t.normal[0].z);
    }
    return r;
}

bool sameBytes(const std::vector<float>& a, const std::vector<float>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}

}  // namespace

int main(int argc, char** argv) {
    const int grids = argc > 1 ? std::atoi(argv[1]) : 300;
    std::mt19937 rng(20240);
    long long triangles = 0, vertices = 0;
    for (int it = 0; it < grids; it++) {
        const int dx = 1 + (int)(rng() % 9), dy = 1 + (int)(rng() % 9), dz = 1 + (int)(rng() % 9);
        const unsigned density = rng() % 101;
        std::vector<uint8_t> vox((size_t)dx * dy * dz);
        for (uint8_t& v : vox) v = rng() % 100 < density ? 1 : 0;
        const float gmin[3] = { -0.5f + (float)(rng() % 7), -3.25f, 100.0f * (float)(rng() % 3) };
        const float sizes[4] = { 1.0f, 1.0f / 16, 1.0f / 512, 10.0f };
        const float vs = sizes[rng() % 4];
        rto_dc_params p;
        std::memset(&p, 0, sizeof p);
        p.area_rule = (int)(rng() % 2);
        p.clip = (int)(rng() % 2);
        const int dim[3] = { dx, dy, dz };
        for (int a = 0; a < 3; a++) {
            p.clip_lo[a] = (int)(rng() % (unsigned)dim[a]);
            p.clip_hi[a] = p.clip_lo[a] + 1 + (int)(rng() % (unsigned)(dim[a] - p.clip_lo[a]));
        }
        std::vector<int32_t> cell;
        rto_dc_summary s;
        int rc = -1;
        const std::vector<MCTriangle> got = dualContourVolume(vox.data(), dx, dy, dz, rtmath::vec3(gmin[0], gmin[1], gmin[2]), vs, p, &cell, &s, &rc);
        const Expect want = plainLoop(vox, dx, dy, dz, gmin, vs, p);
        if (rc != RTO_OK || !sameBytes(records(got), want.rec) || cell != want.cell || std::memcmp(&s, &want.s, sizeof s) != 0) {
            std::printf("grid %d (%d x %d x %d, rule %d, clip %d): dualContourVolume differs from the plain loop\n", it, dx, dy, dz, p.area_rule, p.clip);
            return 1;
        }
        if (s.triangles + s.dropped != 2 * s.faces) { std::printf("grid %d: kept + dropped != 2 faces\n", it); return 1; }
        triangles += s.triangles;
        // the reference's own shape: vertices, and the whole list under its rule without a box
        VoxelGrid grid;
        grid.dimX = dx; grid.dimY = dy; grid.dimZ = dz;
        grid.minX = gmin[0]; grid.minY = gmin[1]; grid.minZ = gmin[2];
        grid.voxelSize = vs;
        grid.data.resize(vox.size());
        for (size_t i = 0; i < vox.size(); i++) grid.data[i] = vox[i] ? VoxelState::FILLED : VoxelState::EMPTY;
        AdaptiveDualContouringRenderer r;
        const std::vector<rtmath::vec4> a = r.dualVertices(grid);
        const std::vector<rto_dual_vertex> b = dualVertexVolume(vox.data(), dx, dy, dz, rtmath::vec3(gmin[0], gmin[1], gmin[2]), vs);
        for (size_t i = 0; i < a.size(); i++)
            if (std::memcmp(&a[i].x, b[i].p, 12) != 0 || (int)a[i].w != b[i].points) {
                std::printf("grid %d: voxel %zu: the stored-points form and the shared vertex function differ\n", it, i);
                return 1;
            }
        vertices += (long long)a.size();
        if (p.area_rule == RTO_DC_AREA_REFERENCE && !p.clip) {
            const std::vector<MCTriangle> whole = r.render(nullptr, grid, 0, 0, 0, grid.dimX);
            if (!sameBytes(records(whole), want.rec)) { std::printf("grid %d: render() differs\n", it); return 1; }
        }
    }
    // the refusals
    rto_dc_params p;
    std::memset(&p, 0, sizeof p);
    std::vector<uint8_t> vox(8, 1);
    int rc = 0;
    p.area_rule = 2;
    if (!dualContourVolume(vox.data(), 2, 2, 2, rtmath::vec3(0, 0, 0), 1.0f, p, nullptr, nullptr, &rc).empty() || rc != RTO_E_INVALID) return 1;
    p.area_rule = 0; p.clip = 1; p.clip_hi[0] = 3; p.clip_hi[1] = p.clip_hi[2] = 1;
    if (!dualContourVolume(vox.data(), 2, 2, 2, rtmath::vec3(0, 0, 0), 1.0f, p, nullptr, nullptr, &rc).empty() || rc != RTO_E_INVALID) return 1;
    std::printf("ok: %d grids, %lld triangles, %lld vertices\n", grids, triangles, vertices);
    return 0;
}
