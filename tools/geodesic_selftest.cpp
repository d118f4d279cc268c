// tools/geodesic_selftest.cpp -- the host layer's CPU form of the geodesic rule (host/Geodesic.cpp) as a stand-alone program, so
// that it can run under AddressSanitizer and UBSan with no Python and no GPU (tools/sanitize_geodesic.sh).  Seeded random grids,
// degenerate dims, full and empty media: every medium, connectivity and limit against a Bellman-Ford relaxation to the fixed
// point, the paths' invariants, the flood, the refusals.  Exit code 0 and "geodesic selftest ok" when all hold.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "Geodesic.h"

static int g_fail = 0;
#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); g_fail++; } \
    } while (0)

static VoxelGrid make(int dx, int dy, int dz, unsigned seed, double fill) {
    VoxelGrid g;
    g.dimX = dx; g.dimY = dy; g.dimZ = dz;
    g.data.resize((size_t)dx * dy * dz);
    unsigned s = seed * 2654435761u + 12345u;
    for (auto& v : g.data) {
        s = s * 1664525u + 1013904223u;
        v = (double)(s >> 8) / (double)(1u << 24) < fill ? VoxelState::FILLED : VoxelState::EMPTY;
    }
    return g;
}

// the weight of the move from a to b under the connectivity, 0: not a move
static int moveWeight(const VoxelGrid& g, int64_t a, int64_t b, int connectivity) {
    const int64_t xy = (int64_t)g.dimX * g.dimY;
    const int d[3] = { (int)(b % g.dimX - a % g.dimX), (int)((b / g.dimX) % g.dimY - (a / g.dimX) % g.dimY), (int)(b / xy - a / xy) };
    int changed = 0;
    for (int k = 0; k < 3; k++) {
        if (d[k] < -1 || d[k] > 1) return 0;
        changed += d[k] != 0;
    }
    if (changed == 0 || (connectivity == RTO_CONN_FACE && changed != 1)) return 0;
    return connectivity == RTO_CONN_FACE ? 1 : 2 + changed;
}

static void check_field(const VoxelGrid& g, int medium, int connectivity, const std::vector<int64_t>& seeds, int64_t limit) {
    std::vector<int32_t> f;
    rto_geo_summary sm;
    CHECK(geodesicFieldCPU(g, medium, connectivity, seeds.data(), (int64_t)seeds.size(), limit, f, &sm) == RTO_OK);
    const int64_t n = (int64_t)g.dimX * g.dimY * g.dimZ;
    CHECK((int64_t)f.size() == n);
    if ((int64_t)f.size() != n) return;
    const VoxelState want = medium == RTO_SET_SOLID ? VoxelState::FILLED : VoxelState::EMPTY;
    // Bellman-Ford: sweep all voxels until nothing changes
    std::vector<int64_t> d((size_t)n, RTO_DIST_NONE);
    for (int64_t s : seeds)
        if (g.data[(size_t)s] == want) d[(size_t)s] = 0;
    for (bool again = true; again;) {
        again = false;
        for (int64_t v = 0; v < n; v++) {
            if (g.data[(size_t)v] != want) continue;
            const int x = (int)(v % g.dimX), y = (int)((v / g.dimX) % g.dimY), z = (int)(v / ((int64_t)g.dimX * g.dimY));
            for (int dz = -1; dz <= 1; dz++)
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        const int a = x + dx, b = y + dy, c = z + dz;
                        if (a < 0 || a >= g.dimX || b < 0 || b >= g.dimY || c < 0 || c >= g.dimZ) continue;
                        const int64_t u = a + (int64_t)g.dimX * (b + (int64_t)g.dimY * c);
                        const int w = moveWeight(g, u, v, connectivity);
                        if (!w || d[(size_t)u] == RTO_DIST_NONE) continue;
                        if (d[(size_t)u] + w < d[(size_t)v]) { d[(size_t)v] = d[(size_t)u] + w; again = true; }
                    }
        }
    }
    int64_t reached = 0, best = -1, arg = -1;
    for (int64_t v = 0; v < n; v++) {
        const int64_t m = d[(size_t)v] > limit ? (int64_t)RTO_DIST_NONE : d[(size_t)v];
        CHECK(f[(size_t)v] == m);
        if (m != RTO_DIST_NONE) { reached++; if (m > best) { best = m; arg = v; } }
    }
    CHECK(sm.reached == reached && sm.max_g == best && sm.argmax == arg && sm.reserved == 0);
    // paths: every voxel as a target
    std::vector<int64_t> targets((size_t)n), lens((size_t)n), rows;
    for (int64_t v = 0; v < n; v++) targets[(size_t)v] = v;
    CHECK(geodesicPathsCPU(g, connectivity, f, targets.data(), n, 0, nullptr, lens.data()) == RTO_OK);
    const int64_t maxLen = std::max<int64_t>(1, *std::max_element(lens.begin(), lens.end()));
    rows.assign((size_t)(n * maxLen), -7);
    std::vector<int64_t> lens2((size_t)n);
    CHECK(geodesicPathsCPU(g, connectivity, f, targets.data(), n, maxLen, rows.data(), lens2.data()) == RTO_OK);
    CHECK(lens == lens2);
    for (int64_t v = 0; v < n; v++) {
        const int64_t* row = rows.data() + v * maxLen;
        const int64_t len = lens[(size_t)v];
        if (f[(size_t)v] == RTO_DIST_NONE) { CHECK(len == -1 && row[0] == -1); continue; }
        CHECK(len >= 1 && row[0] == v && f[(size_t)row[len - 1]] == 0);
        int64_t total = 0;
        for (int64_t k = 0; k + 1 < len; k++) {
            const int w = moveWeight(g, row[k], row[k + 1], connectivity);
            CHECK(w > 0 && f[(size_t)row[k]] - f[(size_t)row[k + 1]] == w && g.data[(size_t)row[k + 1]] == want);
            total += w;
        }
        CHECK(total == f[(size_t)v]);
        for (int64_t k = len; k < maxLen; k++) CHECK(row[k] == -1);
    }
    // the flood flips exactly the reached voxels
    VoxelGrid e = g;
    CHECK(floodGeodesicCPU(e, medium, connectivity, seeds.data(), (int64_t)seeds.size(), limit) == reached);
    for (int64_t v = 0; v < n; v++) CHECK((e.data[(size_t)v] != g.data[(size_t)v]) == (f[(size_t)v] != RTO_DIST_NONE));
}

int main() {
    const int shapes[][3] = { { 1, 1, 1 }, { 3, 2, 5 }, { 17, 9, 5 }, { 1, 40, 1 }, { 64, 1, 2 }, { 2, 3, 33 } };
    unsigned seed = 1;
    for (const auto& s : shapes)
        for (double fill : { 0.0, 0.3, 0.6, 1.0 }) {
            const VoxelGrid g = make(s[0], s[1], s[2], seed++, fill);
            const int64_t n = (int64_t)s[0] * s[1] * s[2];
            const std::vector<int64_t> seeds = { 0, n / 2, n - 1, n / 2 };
            for (int medium : { RTO_SET_SOLID, RTO_SET_EMPTY })
                for (int conn : { RTO_CONN_FACE, RTO_CONN_FULL })
                    for (int64_t limit : { (int64_t)0, (int64_t)1, (int64_t)7, (int64_t)0x7fffffff, (int64_t)1 << 40 }) check_field(g, medium, conn, seeds, limit);
        }
    // refusals
    VoxelGrid g = make(5, 4, 3, 9, 0.3);
    const VoxelGrid before = g;
    std::vector<int32_t> f;
    const int64_t ok[1] = { 0 }, low[1] = { -1 }, high[1] = { 60 };
    CHECK(geodesicFieldCPU(g, 2, RTO_CONN_FACE, ok, 1, 5, f, nullptr) == RTO_E_INVALID && f.empty());
    CHECK(geodesicFieldCPU(g, RTO_SET_EMPTY, 18, ok, 1, 5, f, nullptr) == RTO_E_INVALID);
    CHECK(geodesicFieldCPU(g, RTO_SET_EMPTY, RTO_CONN_FACE, ok, 0, 5, f, nullptr) == RTO_E_INVALID);
    CHECK(geodesicFieldCPU(g, RTO_SET_EMPTY, RTO_CONN_FACE, nullptr, 1, 5, f, nullptr) == RTO_E_INVALID);
    CHECK(geodesicFieldCPU(g, RTO_SET_EMPTY, RTO_CONN_FACE, ok, 1, -1, f, nullptr) == RTO_E_INVALID);
    CHECK(geodesicFieldCPU(g, RTO_SET_EMPTY, RTO_CONN_FACE, low, 1, 5, f, nullptr) == RTO_E_INVALID);
    CHECK(geodesicFieldCPU(g, RTO_SET_EMPTY, RTO_CONN_FACE, high, 1, 5, f, nullptr) == RTO_E_INVALID);
    CHECK(floodGeodesicCPU(g, RTO_SET_EMPTY, RTO_CONN_FACE, high, 1, 5) == RTO_E_INVALID && g.data == before.data);
    VoxelGrid none;
    CHECK(geodesicFieldCPU(none, RTO_SET_EMPTY, RTO_CONN_FACE, ok, 1, 5, f, nullptr) == RTO_E_UNSUPPORTED);
    CHECK(geodesicFieldCPU(g, RTO_SET_EMPTY, RTO_CONN_FACE, ok, 1, 5, f, nullptr) == RTO_OK);
    int64_t len = 0, row[2];
    CHECK(geodesicPathsCPU(g, RTO_CONN_FACE, f, ok, 0, 2, row, &len) == RTO_E_INVALID);
    CHECK(geodesicPathsCPU(g, RTO_CONN_FACE, f, high, 1, 2, row, &len) == RTO_E_INVALID);
    CHECK(geodesicPathsCPU(g, RTO_CONN_FACE, f, ok, 1, -1, row, &len) == RTO_E_INVALID);
    CHECK(geodesicPathsCPU(g, RTO_CONN_FACE, f, ok, 1, 2, nullptr, &len) == RTO_E_INVALID);
    CHECK(geodesicPathsCPU(g, RTO_CONN_FACE, std::vector<int32_t>(3), ok, 1, 2, row, &len) == RTO_E_INVALID);
    if (g_fail) { std::fprintf(stderr, "geodesic selftest: %d checks failed\n", g_fail); return 1; }
    std::puts("geodesic selftest ok");
    return 0;
}
