// tools/exposure_selftest.cpp -- the host layer's CPU form of the exposure rule (host/Exposure.cpp) as a stand-alone program, so that
// it can run under AddressSanitizer and UBSan with no Python and no GPU (tools/sanitize_exposure.sh).  The comparator is not the
// template but the rule as it is written: for every start voxel p, direction d and voxel q of a small grid, q is crossed when the
// open half line from p's centre meets q's open cube, decided in doubled integer coordinates by cross-multiplying the ends of the
// three time intervals.  Checked: the template's properties (last entry, length, monotone max-norm), the field and summary on
// seeded random grids, full and empty grids and degenerate dims, both modes, with and without a reach and weights, the closed forms
// of DESIGN.md section 25, and the refusals.  Exit code 0 and "exposure selftest ok" when all hold.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "Exposure.h"

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

// Does the ray from the centre of p along d meet the open cube of q != p?  Per axis with d_a != 0 the times inside q's slab are the
// open interval (lo_a, hi_a) / |d_a|; crossed: every hi_a > 0 and every lo_a / |d_a| < hi_b / |d_b|.
static bool crossed_slow(const int p[3], const int d[3], const int q[3]) {
    if (p[0] == q[0] && p[1] == q[1] && p[2] == q[2]) return false;
    long long lo[3], hi[3], den[3];
    int axes = 0;
    for (int a = 0; a < 3; a++) {
        const long long P = 2LL * p[a] + 1;
        if (d[a] == 0) {
            if (q[a] != p[a]) return false;
            continue;
        }
        lo[axes] = d[a] > 0 ? 2LL * q[a] - P : P - 2LL * q[a] - 2;
        hi[axes] = lo[axes] + 2;
        den[axes] = std::llabs((long long)d[a]);
        axes++;
    }
    for (int a = 0; a < axes; a++) {
        if (hi[a] <= 0) return false;
        for (int b = 0; b < axes; b++)
            if (!(lo[a] * den[b] < hi[b] * den[a])) return false;
    }
    return true;
}

static bool solid(const VoxelGrid& g, int x, int y, int z) { return g.data[((size_t)z * g.dimY + y) * g.dimX + x] == VoxelState::FILLED; }

static void field_slow(const VoxelGrid& g, const std::vector<int32_t>& dirs, const int32_t* weights, int mode, int reach, std::vector<int32_t>& e,
                       rto_expo_summary& s) {
    const int n = (int)dirs.size() / 3;
    long long W = 0;
    for (int i = 0; i < n; i++) W += weights ? weights[i] : 1;
    e.assign(g.data.size(), -1);
    s = rto_expo_summary{ 0, 0, 0, 0 };
    for (int z = 0; z < g.dimZ; z++)
        for (int y = 0; y < g.dimY; y++)
            for (int x = 0; x < g.dimX; x++) {
                if (solid(g, x, y, z)) continue;
                if (mode == RTO_EXPO_SKIN) {
                    bool near = false;
                    const int nb[6][3] = { { -1, 0, 0 }, { 1, 0, 0 }, { 0, -1, 0 }, { 0, 1, 0 }, { 0, 0, -1 }, { 0, 0, 1 } };
                    for (const auto& o : nb) {
                        const int nx = x + o[0], ny = y + o[1], nz = z + o[2];
                        if (nx >= 0 && nx < g.dimX && ny >= 0 && ny < g.dimY && nz >= 0 && nz < g.dimZ && solid(g, nx, ny, nz)) near = true;
                    }
                    if (!near) continue;
                }
                long long sum = 0;
                const int p[3] = { x, y, z };
                for (int i = 0; i < n; i++) {
                    const int d[3] = { dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2] };
                    bool blocked = false;
                    for (int qz = 0; qz < g.dimZ && !blocked; qz++)
                        for (int qy = 0; qy < g.dimY && !blocked; qy++)
                            for (int qx = 0; qx < g.dimX && !blocked; qx++) {
                                const int q[3] = { qx, qy, qz };
                                const int far = std::max(std::max(std::abs(qx - x), std::abs(qy - y)), std::abs(qz - z));
                                if (far <= reach && solid(g, qx, qy, qz) && crossed_slow(p, d, q)) blocked = true;
                            }
                    if (!blocked) sum += weights ? weights[i] : 1;
                }
                e[((size_t)z * g.dimY + y) * g.dimX + x] = (int32_t)sum;
                s.evaluated++;
                s.total += sum;
                s.dark += sum == 0;
                s.open += sum == W;
            }
}

static std::vector<int32_t> direction_set() {
    std::vector<int32_t> d;
    for (int z = -1; z <= 1; z++)
        for (int y = -1; y <= 1; y++)
            for (int x = -1; x <= 1; x++)
                if (x || y || z) d.insert(d.end(), { x, y, z });
    const int more[][3] = { { 1, 2, 3 }, { 3, -1, 2 }, { -2, 5, 0 }, { 7, 1, -1 }, { 5, 3, -4 }, { 0, 0, -3 }, { 9, 7, -8 }, { -6, 4, 2 }, { 2, 2, 0 },
                            { 255, 1, -1 }, { 253, 255, 254 }, { -255, -255, -255 } };
    for (const auto& m : more) d.insert(d.end(), { m[0], m[1], m[2] });
    return d;
}

static bool same(const rto_expo_summary& a, const rto_expo_summary& b) {
    return a.evaluated == b.evaluated && a.total == b.total && a.dark == b.dark && a.open == b.open;
}

// EMPTY voxels of a 21^3 grid with one SOLID voxel at the centre that direction d leaves blocked.
static int64_t centre_blocks(int a, int b, int c, int reach) {
    VoxelGrid g = make(21, 21, 21, 0, 0.0);
    g.data[(size_t)g.index(10, 10, 10)] = VoxelState::FILLED;
    const int32_t d[3] = { a, b, c };
    std::vector<int32_t> e;
    rto_expo_summary s;
    CHECK(exposureFieldCPU(g, d, nullptr, 1, RTO_EXPO_ALL, reach, e, &s) == RTO_OK);
    return s.dark;
}

int main() {
    const std::vector<int32_t> D = direction_set();
    const int n = (int)D.size() / 3;
    // the templates
    for (int i = 0; i < n; i++) {
        std::vector<int32_t> off;
        int32_t prim[3];
        CHECK(exposureTemplate(&D[3 * (size_t)i], off, prim));
        const size_t entries = off.size() / 3;
        CHECK(entries >= 1 && off[3 * entries - 3] == prim[0] && off[3 * entries - 2] == prim[1] && off[3 * entries - 1] == prim[2]);
        std::set<std::pair<long long, long long>> times;              // distinct (2 m + 1) / |a| as reduced fractions
        for (int a = 0; a < 3; a++)
            for (int m = 0; m < std::abs(prim[a]); m++) {
                long long num = 2 * m + 1, den = std::abs(prim[a]), x = num, y = den;
                while (y) { const long long t = x % y; x = y; y = t; }
                times.insert({ num / x, den / x });
            }
        CHECK(times.size() == entries);
        int last = 0;
        for (size_t j = 0; j < entries; j++) {
            const int far = std::max(std::max(std::abs(off[3 * j]), std::abs(off[3 * j + 1])), std::abs(off[3 * j + 2]));
            CHECK(far >= last && far >= 1);
            last = far;
        }
    }
    {
        std::vector<int32_t> off;
        int32_t prim[3];
        const int32_t a[3] = { 1, 1, 1 }, b[3] = { 1, 2, 3 }, zero[3] = { 0, 0, 0 }, big[3] = { 256, 0, 0 };
        CHECK(exposureTemplate(a, off, prim) && off.size() == 3);
        CHECK(exposureTemplate(b, off, prim) && off.size() == 15);
        CHECK(!exposureTemplate(zero, off, prim) && off.empty());
        CHECK(!exposureTemplate(big, off, prim) && off.empty());
    }
    // the field against the definition
    std::vector<int32_t> weights((size_t)n);
    for (int i = 0; i < n; i++) weights[(size_t)i] = 1 + i % 7;
    weights[3] = 0;
    const int dims[][3] = { { 7, 5, 4 }, { 5, 3, 2 }, { 9, 1, 1 }, { 1, 1, 6 }, { 1, 1, 1 }, { 4, 4, 4 } };
    unsigned seed = 1;
    for (const auto& dm : dims)
        for (const double fill : { 0.0, 0.15, 0.4, 1.0 }) {
            const VoxelGrid g = make(dm[0], dm[1], dm[2], seed++, fill);
            for (const int mode : { RTO_EXPO_ALL, RTO_EXPO_SKIN })
                for (const int reach : { 1, 2, RTO_EXPO_NO_LIMIT })
                    for (const int32_t* w : { (const int32_t*)nullptr, (const int32_t*)weights.data() }) {
                        std::vector<int32_t> e, want;
                        rto_expo_summary s, ws;
                        int64_t steps = -1;
                        CHECK(exposureFieldCPU(g, D.data(), w, n, mode, reach, e, &s, &steps) == RTO_OK);
                        field_slow(g, D, w, mode, reach, want, ws);
                        CHECK(e == want);
                        CHECK(same(s, ws));
                        CHECK(steps >= s.evaluated * n);
                        if (fill == 1.0) CHECK(s.evaluated == 0 && s.total == 0 && s.dark == 0 && s.open == 0);
                        if (fill == 0.0) CHECK(mode == RTO_EXPO_SKIN ? s.evaluated == 0 : (s.open == s.evaluated && s.evaluated == (int64_t)g.data.size()));
                    }
        }
    // closed forms: one SOLID voxel at the centre of 21^3
    CHECK(centre_blocks(1, 0, 0, RTO_EXPO_NO_LIMIT) == 10);
    CHECK(centre_blocks(1, 1, 1, RTO_EXPO_NO_LIMIT) == 10);
    CHECK(centre_blocks(1, 2, 3, RTO_EXPO_NO_LIMIT) == 17);
    CHECK(centre_blocks(3, -1, 2, RTO_EXPO_NO_LIMIT) == 17);
    CHECK(centre_blocks(-2, 5, 0, RTO_EXPO_NO_LIMIT) == 14);
    CHECK(centre_blocks(1, 2, 3, 3) == 5);
    CHECK(centre_blocks(2, 2, 0, RTO_EXPO_NO_LIMIT) == centre_blocks(1, 1, 0, RTO_EXPO_NO_LIMIT));
    {   // corner cutting: 2 x 2 x 2 with only (0, 0, 0) and (1, 1, 1) EMPTY
        VoxelGrid g = make(2, 2, 2, 0, 1.0);
        g.data[0] = VoxelState::EMPTY;
        g.data[7] = VoxelState::EMPTY;
        const int32_t four[12] = { 1, 1, 1, 1, 1, 0, 1, 0, 0, 1, 2, 3 };
        const int32_t w[4] = { 1, 2, 4, 8 };
        std::vector<int32_t> e;
        CHECK(exposureFieldCPU(g, four, w, 4, RTO_EXPO_ALL, RTO_EXPO_NO_LIMIT, e, nullptr) == RTO_OK);
        CHECK(e.size() == 8 && e[0] == 1 && e[7] == 15 && e[1] == -1);
    }
    // refusals
    {
        const VoxelGrid g = make(5, 3, 2, 3, 0.3);
        std::vector<int32_t> e;
        const int32_t ok[6] = { 1, 0, 0, 0, 1, 0 }, zero[6] = { 1, 0, 0, 0, 0, 0 }, big[3] = { 0, -256, 1 }, neg[2] = { 1, -1 };
        const int32_t heavy[2] = { 0x7fffffff, 1 }, most[2] = { 0x7ffffffe, 1 };
        std::vector<int32_t> many(3 * (size_t)(RTO_EXPO_MAX_DIRS + 1), 1);
        CHECK(exposureFieldCPU(g, nullptr, nullptr, 2, RTO_EXPO_ALL, 1, e, nullptr) == RTO_E_INVALID && e.empty());
        CHECK(exposureFieldCPU(g, ok, nullptr, 0, RTO_EXPO_ALL, 1, e, nullptr) == RTO_E_INVALID);
        CHECK(exposureFieldCPU(g, many.data(), nullptr, RTO_EXPO_MAX_DIRS + 1, RTO_EXPO_ALL, 1, e, nullptr) == RTO_E_INVALID);
        CHECK(exposureFieldCPU(g, many.data(), nullptr, RTO_EXPO_MAX_DIRS, RTO_EXPO_ALL, 1, e, nullptr) == RTO_OK);
        CHECK(exposureFieldCPU(g, zero, nullptr, 2, RTO_EXPO_ALL, 1, e, nullptr) == RTO_E_INVALID);
        CHECK(exposureFieldCPU(g, big, nullptr, 1, RTO_EXPO_ALL, 1, e, nullptr) == RTO_E_INVALID);
        CHECK(exposureFieldCPU(g, ok, neg, 2, RTO_EXPO_ALL, 1, e, nullptr) == RTO_E_INVALID);
        CHECK(exposureFieldCPU(g, ok, heavy, 2, RTO_EXPO_ALL, 1, e, nullptr) == RTO_E_INVALID);
        CHECK(exposureFieldCPU(g, ok, most, 2, RTO_EXPO_ALL, 1, e, nullptr) == RTO_OK);
        CHECK(exposureFieldCPU(g, ok, nullptr, 2, 2, 1, e, nullptr) == RTO_E_INVALID);
        CHECK(exposureFieldCPU(g, ok, nullptr, 2, -1, 1, e, nullptr) == RTO_E_INVALID);
        CHECK(exposureFieldCPU(g, ok, nullptr, 2, RTO_EXPO_SKIN, 0, e, nullptr) == RTO_E_INVALID && e.empty());
        CHECK(exposureFieldCPU(VoxelGrid(), ok, nullptr, 2, RTO_EXPO_SKIN, 1, e, nullptr) == RTO_E_UNSUPPORTED);
        CHECK(exposureFieldCPU(VoxelGrid(), zero, nullptr, 2, RTO_EXPO_SKIN, 1, e, nullptr) == RTO_E_INVALID);     // the arguments come first
    }
    if (g_fail) {
        std::fprintf(stderr, "exposure selftest: %d checks failed\n", g_fail);
        return 1;
    }
    std::printf("exposure selftest ok\n");
    return 0;
}
