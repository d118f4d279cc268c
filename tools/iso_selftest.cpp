// iso_selftest.cpp -- the CPU form of a field isosurface (host/MarchingCubes.cpp: isoSurfaceVolume) against a plain triple loop
// written here: the substituted float samples of the padded, clipped box are written out as a block first, and plain_cells() below
// walks the block's cells with its own statement of the cell -- corner order, case bits, edge corner pairs, the three snaps and the
// interpolation, per component -- and must give the same vertices bit for bit.  What it shares with the code under test is DATA
// only: the rows of the case table (host/mc_cases.inc), which tests/golden/make_golden_iso.py proves equal to the reference's
// tables.  marchingCubesVolume over the same block is compared too; it shares cellTriangles with isoSurfaceVolume, so it checks the
// loop, the substitution and the placeholder normals, not the cell (bit for bit where the block starts at index 0; elsewhere its
// moved origin rounds differently and the positions are compared within a tolerance).  Further: tri_cell names a cell of the box and
// never falls, every vertex lies inside its cell, a zero normal is counted as degenerate, the summary adds up, bad parameters are
// refused.  Host code only; meant to be built and run with sanitizers:
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -Iinclude
//       -Iray_tracing_octrees_amd/host tools/iso_selftest.cpp ray_tracing_octrees_amd/host/MarchingCubes.cpp
//       ray_tracing_octrees_amd/host/OctreeVoxel.cpp -o iso_selftest
//   ./iso_selftest [rounds]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "MarchingCubes.h"
#include "rto_hip.h"
#include "mc_cases.inc"      // the table's rows: data, shared on purpose (see above)

using rtmath::vec3;

static int g_failed = 0;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond)) { if (g_failed++ < 20) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } \
    } while (0)

static bool same_bits(const vec3& a, const vec3& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// The plain form: every cell of a block of samples whose sample (0, 0, 0) has the index `first`, z slowest; 9 floats a triangle.
static std::vector<float> plain_cells(const std::vector<float>& block, const int n[3], const int first[3], const float origin[3], float vs,
                                      float level) {
    static const int cornerXYZ[8][3] = { { 0, 0, 0 }, { 1, 0, 0 }, { 1, 1, 0 }, { 0, 1, 0 }, { 0, 0, 1 }, { 1, 0, 1 }, { 1, 1, 1 }, { 0, 1, 1 } };
    static const int edgeEnds[12][2] = { { 0, 1 }, { 1, 2 }, { 2, 3 }, { 3, 0 }, { 4, 5 }, { 5, 6 }, { 6, 7 }, { 7, 4 }, { 0, 4 }, { 1, 5 }, { 2, 6 }, { 3, 7 } };
    std::vector<float> out;
    for (int z = 0; z + 1 < n[2]; z++)
        for (int y = 0; y + 1 < n[1]; y++)
            for (int x = 0; x + 1 < n[0]; x++) {
                float val[8], pos[8][3];
                int bits = 0;
                for (int i = 0; i < 8; i++) {
                    const int c[3] = { x + cornerXYZ[i][0], y + cornerXYZ[i][1], z + cornerXYZ[i][2] };
                    val[i] = block[(size_t)c[0] + (size_t)c[1] * n[0] + (size_t)c[2] * n[0] * n[1]];
                    for (int a = 0; a < 3; a++) pos[i][a] = origin[a] + (float)(c[a] + first[a]) * vs;
                    if (val[i] < level) bits += 1 << i;
                }
                for (const char* e = kMcCaseEdges[bits]; *e != 'f'; e++) {
                    const int id = *e <= '9' ? *e - '0' : *e - 'a' + 10;
                    const int a = edgeEnds[id][0], b = edgeEnds[id][1];
                    int take = 0;                                        // 1: the first end, 2: the second, 0: between them
                    if (std::fabs(level - val[a]) < 1e-6f) take = 1;
                    else if (std::fabs(level - val[b]) < 1e-6f) take = 2;
                    else if (std::fabs(val[a] - val[b]) < 1e-6f) take = 1;
                    const float mu = take ? 0.0f : (level - val[a]) / (val[b] - val[a]);
                    for (int k = 0; k < 3; k++)
                        out.push_back(take == 1 ? pos[a][k] : take == 2 ? pos[b][k] : pos[a][k] + mu * (pos[b][k] - pos[a][k]));
                }
            }
    return out;
}

static void one_round(std::mt19937& rng, int round) {
    auto pick = [&](int lo, int hi) { return (int)(rng() % (unsigned)(hi - lo + 1)) + lo; };
    const int dim[3] = { pick(1, 37), pick(1, 11), pick(1, 10) };
    std::vector<int32_t> vol((size_t)dim[0] * dim[1] * dim[2]);
    const int span = pick(2, 9), shift = round % 3 == 0 ? (1 << 24) - 3 : pick(-4, 0);
    for (int32_t& v : vol) v = shift + pick(0, span);
    rto_iso_params p;
    std::memset(&p, 0, sizeof p);
    p.source = RTO_FIELD_CALLER;
    p.valid_lo = shift + pick(0, 1); p.valid_hi = shift + span - pick(0, 1);
    if (p.valid_lo <= RTO_FIELD_PIXEL_NONE) p.valid_lo = RTO_FIELD_PIXEL_NONE + 1;
    p.level = (float)shift + (float)pick(0, 2 * span) * 0.5f;            // whole levels too: the snaps
    p.outside = (float)shift + (float)pick(-2, span + 2);
    p.pad = pick(0, 1);
    p.clip = pick(0, 1);
    int lo[3] = { 0, 0, 0 }, hi[3] = { dim[0], dim[1], dim[2] };
    if (p.clip)
        for (int a = 0; a < 3; a++) {
            lo[a] = pick(0, dim[a] - 1); hi[a] = pick(lo[a] + 1, dim[a]);
            p.clip_lo[a] = lo[a]; p.clip_hi[a] = hi[a];
        }
    const vec3 gmin((float)pick(-50, 50) * 0.37f, (float)pick(-50, 50) * 1.3f, (float)pick(-5, 5));
    const float vs = (float)pick(1, 40) * 0.05f;

    std::vector<int32_t> cell;
    rto_iso_summary sum;
    int rc = -99;
    const std::vector<MCTriangle> got = isoSurfaceVolume(vol.data(), dim[0], dim[1], dim[2], gmin, vs, p, &cell, &sum, &rc);
    CHECK(rc == RTO_OK, "round %d: rc %d", round, rc);
    CHECK(cell.size() == got.size() && sum.triangles == (int64_t)got.size() && sum.reserved == 0, "round %d: sizes", round);

    // the plain form: the block of substituted samples, then the reference-named loop over it
    const int first[3] = { lo[0] - p.pad, lo[1] - p.pad, lo[2] - p.pad };
    const int n[3] = { hi[0] - lo[0] + 2 * p.pad, hi[1] - lo[1] + 2 * p.pad, hi[2] - lo[2] + 2 * p.pad };
    std::vector<float> block((size_t)n[0] * n[1] * n[2]);
    for (int z = 0; z < n[2]; z++)
        for (int y = 0; y < n[1]; y++)
            for (int x = 0; x < n[0]; x++) {
                const int gx = x + first[0], gy = y + first[1], gz = z + first[2];
                float f = p.outside;
                if (gx >= lo[0] && gx < hi[0] && gy >= lo[1] && gy < hi[1] && gz >= lo[2] && gz < hi[2]) {
                    const int32_t v = vol[(size_t)gx + (size_t)gy * dim[0] + (size_t)gz * dim[0] * dim[1]];
                    if (v >= p.valid_lo && v <= p.valid_hi) f = (float)v;
                }
                block[(size_t)x + (size_t)y * n[0] + (size_t)z * n[0] * n[1]] = f;
            }
    const vec3 origin(gmin.x + 0.5f * vs, gmin.y + 0.5f * vs, gmin.z + 0.5f * vs);
    const bool atZero = first[0] == 0 && first[1] == 0 && first[2] == 0;
    const vec3 moved = origin + vec3((float)first[0], (float)first[1], (float)first[2]) * vs;
    const std::vector<MCTriangle> want = marchingCubesVolume(block.data(), n[0], n[1], n[2], atZero ? origin : moved, vs, p.level);
    CHECK(want.size() == got.size(), "round %d: %zu triangles against %zu", round, got.size(), want.size());
    if (want.size() != got.size()) return;
    const float org[3] = { origin.x, origin.y, origin.z };
    const std::vector<float> plain = plain_cells(block, n, first, org, vs, p.level);
    CHECK(plain.size() == 9 * got.size(), "round %d: the plain loop gives %zu triangles against %zu", round, plain.size() / 9, got.size());
    if (plain.size() != 9 * got.size()) return;
    for (size_t i = 0; i < got.size(); i++)
        for (int v = 0; v < 3; v++)
            CHECK(std::memcmp(&got[i].v[v], &plain[9 * i + 3 * v], 12) == 0, "round %d: triangle %zu vertex %d differs from the plain loop", round, i, v);

    int64_t degenerate = 0, active = 0;
    int32_t last = -1;
    const float tol = 1e-4f * (std::fabs(gmin.x) + std::fabs(gmin.y) + std::fabs(gmin.z) + 40.0f * vs);
    for (size_t i = 0; i < got.size(); i++) {
        const MCTriangle& t = got[i];
        CHECK(same_bits(want[i].normal[0], vec3(0.0f, 1.0f, 0.0f)), "round %d: the placeholder normal", round);
        for (int v = 0; v < 3; v++) {
            if (atZero) CHECK(same_bits(t.v[v], want[i].v[v]), "round %d: triangle %zu vertex %d differs", round, i, v);
            else CHECK(std::fabs(t.v[v].x - want[i].v[v].x) <= tol && std::fabs(t.v[v].y - want[i].v[v].y) <= tol &&
                       std::fabs(t.v[v].z - want[i].v[v].z) <= tol, "round %d: triangle %zu vertex %d is elsewhere", round, i, v);
        }
        // the owning cell: inside the box, never falling, and the vertices inside it
        const int32_t c = cell[i];
        CHECK(c >= last, "round %d: tri_cell falls at %zu", round, i);
        if (c != last) active++;
        last = c;
        const int ux = c % (dim[0] + 1), uy = (c / (dim[0] + 1)) % (dim[1] + 1), uz = c / ((dim[0] + 1) * (dim[1] + 1));
        const int cx = ux - 1, cy = uy - 1, cz = uz - 1;
        CHECK(cx >= lo[0] - p.pad && cx < hi[0] - 1 + p.pad && cy >= lo[1] - p.pad && cy < hi[1] - 1 + p.pad && cz >= lo[2] - p.pad &&
              cz < hi[2] - 1 + p.pad, "round %d: cell (%d, %d, %d) outside the box", round, cx, cy, cz);
        const vec3 a = origin + vec3((float)cx, (float)cy, (float)cz) * vs, b = origin + vec3((float)(cx + 1), (float)(cy + 1), (float)(cz + 1)) * vs;
        for (int v = 0; v < 3; v++)
            CHECK(t.v[v].x >= a.x - tol && t.v[v].x <= b.x + tol && t.v[v].y >= a.y - tol && t.v[v].y <= b.y + tol && t.v[v].z >= a.z - tol &&
                  t.v[v].z <= b.z + tol, "round %d: triangle %zu leaves its cell", round, i);
        // the normal: unit, or zero and counted
        CHECK(same_bits(t.normal[0], t.normal[1]) && same_bits(t.normal[0], t.normal[2]), "round %d: three normals", round);
        const vec3 nn = t.normal[0];
        const float len = std::sqrt(rtmath::dot(nn, nn));
        if (nn.x == 0.0f && nn.y == 0.0f && nn.z == 0.0f) {
            degenerate++;
            CHECK(!std::signbit(nn.x) && !std::signbit(nn.y) && !std::signbit(nn.z), "round %d: a negative zero", round);
        } else CHECK(std::fabs(len - 1.0f) < 1e-5f, "round %d: a normal of length %g", round, len);
    }
    CHECK(sum.degenerate == degenerate && sum.active_cells == active, "round %d: summary %lld %lld against %lld %lld", round,
          (long long)sum.degenerate, (long long)sum.active_cells, (long long)degenerate, (long long)active);
}

static void refusals() {
    const int32_t vol[8] = { 0, 1, 2, 3, 4, 5, 6, 7 };
    rto_iso_params ok;
    std::memset(&ok, 0, sizeof ok);
    ok.source = RTO_FIELD_CALLER; ok.valid_hi = 0x7ffffffe; ok.level = 3.5f; ok.pad = 1;
    auto rc_of = [&](const rto_iso_params& p, const int32_t* v = nullptr) {
        int rc = -99;
        rto_iso_summary s;
        const size_t n = isoSurfaceVolume(v ? v : vol, 2, 2, 2, vec3(0.0f, 0.0f, 0.0f), 1.0f, p, nullptr, &s, &rc).size();
        if (rc != RTO_OK) CHECK(n == 0 && s.triangles == 0, "a refusal with triangles");
        return rc;
    };
    CHECK(rc_of(ok) == RTO_OK, "the good call");
    rto_iso_params p = ok; p.pad = 2;                       CHECK(rc_of(p) == RTO_E_INVALID, "pad 2");
    p = ok; p.level = NAN;                                  CHECK(rc_of(p) == RTO_E_INVALID, "NaN level");
    p = ok; p.outside = INFINITY;                           CHECK(rc_of(p) == RTO_E_INVALID, "infinite outside");
    p = ok; p.valid_lo = 3; p.valid_hi = 2;                 CHECK(rc_of(p) == RTO_E_INVALID, "window");
    p = ok; p.valid_lo = RTO_FIELD_PIXEL_NONE;              CHECK(rc_of(p) == RTO_E_INVALID, "valid_lo");
    p = ok; p.reserved[1] = 1;                              CHECK(rc_of(p) == RTO_E_INVALID, "reserved");
    p = ok; p.clip = 1; p.clip_hi[0] = p.clip_hi[1] = 2;    CHECK(rc_of(p) == RTO_E_INVALID, "empty clip box");
    p = ok; p.clip = 1; p.clip_hi[0] = p.clip_hi[1] = p.clip_hi[2] = 1; p.pad = 0;
    CHECK(rc_of(p) == RTO_OK, "a box of one sample without pad: an empty list, no error");
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 400;
    std::mt19937 rng(20240530u);
    for (int r = 0; r < rounds; r++) one_round(rng, r);
    refusals();
    if (g_failed) { std::printf("iso_selftest: %d checks FAILED\n", g_failed); return 1; }
    std::printf("iso_selftest: %d rounds ok\n", rounds);
    return 0;
}
