// tools/dose_selftest.cpp -- the host layer's CPU form of the dose rule (host/Dose.cpp) as a stand-alone program, so that it can run
// under AddressSanitizer and UBSan with no Python and no GPU (tools/sanitize_dose.sh).  The comparator is not the walk but the rule
// as it is written: for every evaluated voxel p, source s and voxel q of a small grid, q is crossed when the open segment from p's
// centre to s's meets q's open cube -- decided in doubled integer coordinates by cross-multiplying the ends of the three time
// intervals, from p along d and from s along -d.  Checked: the segments' lengths and ends, the field, coverage and summary on
// seeded random grids, full and empty grids and degenerate dims, both modes and falloffs, with and without a reach, four tables,
// the closed forms of DESIGN.md section 31, and the refusals in their order.  Exit code 0 and "dose selftest ok" when all hold.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "Dose.h"

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
static bool ray_crosses(const int p[3], const int d[3], const int q[3]) {
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

// The segment: crossed from p along d = s - p and from s along -d.
static bool segment_crosses(const int p[3], const int s[3], const int q[3]) {
    const int d[3] = { s[0] - p[0], s[1] - p[1], s[2] - p[2] }, back[3] = { -d[0], -d[1], -d[2] };
    if (!d[0] && !d[1] && !d[2]) return false;
    return ray_crosses(p, d, q) && ray_crosses(s, back, q);
}

static bool solid(const VoxelGrid& g, int x, int y, int z) { return g.data[((size_t)z * g.dimY + y) * g.dimX + x] == VoxelState::FILLED; }

static void field_slow(const VoxelGrid& g, const std::vector<int32_t>& src, const std::vector<uint32_t>& T, int falloff, int mode, int reach,
                       std::vector<int32_t>& e, std::vector<int64_t>& cover, rto_dose_summary& sum) {
    const int n = (int)src.size() / 4, m = (int)T.size();
    const int r = std::min(reach, RTO_DOSE_MAX_REACH);
    e.assign(g.data.size(), -1);
    cover.assign((size_t)n, 0);
    sum = rto_dose_summary{ 0, 0, 0, 0, -1, -1 };
    for (int z = 0; z < g.dimZ; z++)
        for (int y = 0; y < g.dimY; y++)
            for (int x = 0; x < g.dimX; x++) {
                if (solid(g, x, y, z)) continue;
                if (mode == RTO_DOSE_SKIN) {
                    bool near = false;
                    const int nb[6][3] = { { -1, 0, 0 }, { 1, 0, 0 }, { 0, -1, 0 }, { 0, 1, 0 }, { 0, 0, -1 }, { 0, 0, 1 } };
                    for (const auto& o : nb) {
                        const int nx = x + o[0], ny = y + o[1], nz = z + o[2];
                        if (nx >= 0 && nx < g.dimX && ny >= 0 && ny < g.dimY && nz >= 0 && nz < g.dimZ && solid(g, nx, ny, nz)) near = true;
                    }
                    if (!near) continue;
                }
                long long total = 0;
                bool sees = false;
                const int p[3] = { x, y, z };
                for (int i = 0; i < n; i++) {
                    const int s[3] = { src[4 * (size_t)i], src[4 * (size_t)i + 1], src[4 * (size_t)i + 2] };
                    const long long ax = std::abs(s[0] - x), ay = std::abs(s[1] - y), az = std::abs(s[2] - z);
                    if (std::max(ax, std::max(ay, az)) > r) continue;
                    int k = 0;
                    for (int qz = 0; qz < g.dimZ; qz++)
                        for (int qy = 0; qy < g.dimY; qy++)
                            for (int qx = 0; qx < g.dimX; qx++) {
                                const int q[3] = { qx, qy, qz };
                                if (solid(g, qx, qy, qz) && !(qx == s[0] && qy == s[1] && qz == s[2]) && segment_crosses(p, s, q)) k++;
                            }
                    unsigned long long c = ((unsigned long long)src[4 * (size_t)i + 3] * (k < m ? T[(size_t)k] : 0u)) >> 16;
                    if (falloff == RTO_DOSE_FALLOFF_INVERSE_SQUARE) c /= (unsigned long long)std::max(1LL, ax * ax + ay * ay + az * az);
                    total += (long long)c;
                    if (k == 0) { cover[(size_t)i]++; sees = true; }
                }
                const long long v = ((long long)z * g.dimY + y) * g.dimX + x;
                e[(size_t)v] = (int32_t)total;
                sum.evaluated++;
                sum.total += total;
                sum.dark += total == 0;
                sum.seen += sees;
                if (total > sum.peak) { sum.peak = total; sum.peak_voxel = v; }
            }
}

static bool same(const rto_dose_summary& a, const rto_dose_summary& b) {
    return a.evaluated == b.evaluated && a.total == b.total && a.dark == b.dark && a.seen == b.seen && a.peak == b.peak && a.peak_voxel == b.peak_voxel;
}

int main() {
    // the segments: every pair of a 6 x 4 x 3 box against the definition, cell by cell and in a monotone order
    {
        const int dx = 6, dy = 4, dz = 3;
        for (int pv = 0; pv < dx * dy * dz; pv++)
            for (int sv = 0; sv < dx * dy * dz; sv++) {
                const int32_t p[3] = { pv % dx, pv / dx % dy, pv / dx / dy }, s[3] = { sv % dx, sv / dx % dy, sv / dx / dy };
                std::vector<int32_t> cells;
                doseSegment(p, s, cells);
                std::set<int> got;
                int last = 0;
                for (size_t j = 0; j < cells.size() / 3; j++) {
                    const int far = std::max(std::max(std::abs(cells[3 * j] - p[0]), std::abs(cells[3 * j + 1] - p[1])), std::abs(cells[3 * j + 2] - p[2]));
                    CHECK(far >= last && far >= 1);
                    last = far;
                    CHECK(got.insert(cells[3 * j] + dx * (cells[3 * j + 1] + dy * cells[3 * j + 2])).second);
                }
                int want = 0;
                for (int qv = 0; qv < dx * dy * dz; qv++) {
                    const int q[3] = { qv % dx, qv / dx % dy, qv / dx / dy };
                    const int pi[3] = { p[0], p[1], p[2] }, si[3] = { s[0], s[1], s[2] };
                    if (qv != sv && segment_crosses(pi, si, q)) { want++; CHECK(got.count(qv) == 1); }
                }
                CHECK((size_t)want == got.size());
            }
        const int32_t a[3] = { 1023, 1023, 1 }, b[3] = { 1023, 1022, 0 }, o[3] = { 0, 0, 0 };
        std::vector<int32_t> cells;
        doseSegment(a, o, cells);
        CHECK(cells.size() == 3 * 1022);                                 // 1,023 joint x-y steps, the z step at t = 1 / 2 among them, less the arrival
        doseSegment(b, o, cells);
        CHECK(cells.size() == 3 * (1023 + 1022 - 1));
        doseSegment(o, o, cells);
        CHECK(cells.empty());
    }
    // the field against the definition
    const std::vector<std::vector<uint32_t>> tables = { { 65536u }, { 65536u, 32768u, 16384u }, { 65536u, 0u, 65536u }, { 0u, 0u } };
    const int dims[][3] = { { 7, 5, 4 }, { 5, 3, 2 }, { 9, 1, 1 }, { 1, 1, 6 }, { 1, 1, 1 }, { 4, 4, 4 } };
    unsigned seed = 1;
    for (const auto& dm : dims)
        for (const double fill : { 0.0, 0.15, 0.4, 1.0 }) {
            const VoxelGrid g = make(dm[0], dm[1], dm[2], seed++, fill);
            std::vector<int32_t> src = { 0, 0, 0, 1, dm[0] - 1, dm[1] - 1, dm[2] - 1, 1001, dm[0] / 2, dm[1] / 2, dm[2] / 2, 2001, dm[0] - 1, 0, dm[2] / 2, 0,
                                         dm[0] / 2, dm[1] / 2, dm[2] / 2, 4001 };
            const int n = (int)src.size() / 4;
            for (const int mode : { RTO_DOSE_ALL, RTO_DOSE_SKIN })
                for (const int falloff : { RTO_DOSE_FALLOFF_NONE, RTO_DOSE_FALLOFF_INVERSE_SQUARE })
                    for (const int reach : { 1, 2, RTO_DOSE_NO_LIMIT })
                        for (const auto& T : tables) {
                            std::vector<int32_t> e, want;
                            std::vector<int64_t> cover, wcover;
                            rto_dose_summary s, ws;
                            int64_t steps = -1;
                            CHECK(doseFieldCPU(g, src.data(), n, T.data(), (int)T.size(), falloff, mode, reach, e, &cover, &s, &steps) == RTO_OK);
                            field_slow(g, src, T, falloff, mode, reach, want, wcover, ws);
                            CHECK(e == want);
                            CHECK(cover == wcover);
                            CHECK(same(s, ws));
                            CHECK(steps >= 0);
                            if (fill == 1.0) CHECK(s.evaluated == 0 && s.peak == -1 && s.peak_voxel == -1);
                            if (fill == 0.0 && mode == RTO_DOSE_ALL && reach == RTO_DOSE_NO_LIMIT) CHECK(s.seen == s.evaluated && s.evaluated == (int64_t)g.data.size());
                        }
            std::vector<int32_t> e, want;                                // NULL for the table: plain line of sight, m not read
            std::vector<int64_t> cover, wcover;
            rto_dose_summary s, ws;
            CHECK(doseFieldCPU(g, src.data(), n, nullptr, -5, RTO_DOSE_FALLOFF_NONE, RTO_DOSE_ALL, RTO_DOSE_NO_LIMIT, e, &cover, &s) == RTO_OK);
            field_slow(g, src, tables[0], RTO_DOSE_FALLOFF_NONE, RTO_DOSE_ALL, RTO_DOSE_NO_LIMIT, want, wcover, ws);
            CHECK(e == want && cover == wcover && same(s, ws));
        }
    // closed forms
    {   // one SOLID voxel at the centre of 21^3, one corner source: 70 voxels in its shadow
        VoxelGrid g = make(21, 21, 21, 0, 0.0);
        g.data[(size_t)g.index(10, 10, 10)] = VoxelState::FILLED;
        const int32_t src[4] = { 0, 0, 0, 5 };
        std::vector<int32_t> e;
        std::vector<int64_t> cover;
        rto_dose_summary s;
        CHECK(doseFieldCPU(g, src, 1, nullptr, 0, RTO_DOSE_FALLOFF_NONE, RTO_DOSE_ALL, RTO_DOSE_NO_LIMIT, e, &cover, &s) == RTO_OK);
        CHECK(s.dark == 70 && s.seen == 9260 - 70 && cover[0] == 9260 - 70 && s.peak == 5 && s.peak_voxel == 0 && s.total == 5 * (9260 - 70));
    }
    {   // corner cutting: the segment through the shared edge crosses neither voxel it touches
        VoxelGrid g = make(2, 2, 2, 0, 0.0);
        g.data[1] = VoxelState::FILLED;
        g.data[2] = VoxelState::FILLED;
        const int32_t src[4] = { 1, 1, 0, 1000 };
        std::vector<int32_t> e;
        CHECK(doseFieldCPU(g, src, 1, nullptr, 0, RTO_DOSE_FALLOFF_NONE, RTO_DOSE_ALL, RTO_DOSE_NO_LIMIT, e, nullptr, nullptr) == RTO_OK);
        CHECK(e.size() == 8 && e[0] == 1000 && e[1] == -1 && e[3] == 1000);
    }
    {   // the 64-bit product, and k >= m
        VoxelGrid g = make(130, 1, 1, 0, 0.0);
        for (int x = 1; x <= 64; x++) g.data[(size_t)x] = VoxelState::FILLED;
        const int32_t src[4] = { 129, 0, 0, 0x7fffffff };
        std::vector<uint32_t> T(64, 65536u);
        std::vector<int32_t> e;
        CHECK(doseFieldCPU(g, src, 1, T.data(), 64, RTO_DOSE_FALLOFF_NONE, RTO_DOSE_ALL, RTO_DOSE_NO_LIMIT, e, nullptr, nullptr) == RTO_OK);
        CHECK(e[0] == 0 && e[65] == 0x7fffffff && e[129] == 0x7fffffff);
        g.data[64] = VoxelState::EMPTY;
        CHECK(doseFieldCPU(g, src, 1, T.data(), 64, RTO_DOSE_FALLOFF_NONE, RTO_DOSE_ALL, RTO_DOSE_NO_LIMIT, e, nullptr, nullptr) == RTO_OK);
        CHECK(e[0] == 0x7fffffff);
    }
    // refusals, in their order
    {
        const VoxelGrid g = make(5, 3, 2, 3, 0.3);
        std::vector<int32_t> e;
        std::vector<int64_t> cover;
        const int32_t ok[8] = { 0, 0, 0, 1, 4, 2, 1, 2 }, neg[8] = { 0, 0, 0, 1, 4, 2, 1, -1 }, heavy[8] = { 0, 0, 0, 0x7fffffff, 4, 2, 1, 1 };
        const int32_t most[8] = { 0, 0, 0, 0x7ffffffe, 4, 2, 1, 1 }, outside[8] = { 0, 0, 0, 1, 5, 0, 0, 1 }, badneg[8] = { 9, 9, 9, -1, 0, 0, 0, 1 };
        const uint32_t T[3] = { 65536u, 32768u, 16384u }, over[2] = { 65536u, 65537u };
        std::vector<uint32_t> longT(65, 1u);
        std::vector<int32_t> many(4 * (size_t)(RTO_DOSE_MAX_SOURCES + 1), 1);
        int bad = -1;
        const int A = RTO_DOSE_ALL, N = RTO_DOSE_FALLOFF_NONE, R = RTO_DOSE_NO_LIMIT;
        CHECK(doseFieldCPU(g, nullptr, 2, T, 3, N, A, R, e, &cover, nullptr) == RTO_E_INVALID && e.empty() && cover.empty());
        CHECK(doseFieldCPU(g, ok, 0, T, 3, N, A, R, e, nullptr, nullptr) == RTO_E_INVALID);
        CHECK(doseFieldCPU(g, many.data(), RTO_DOSE_MAX_SOURCES + 1, T, 3, N, A, R, e, nullptr, nullptr) == RTO_E_INVALID);
        CHECK(doseFieldCPU(g, many.data(), RTO_DOSE_MAX_SOURCES, T, 3, N, A, R, e, nullptr, nullptr) == RTO_OK);
        CHECK(doseFieldCPU(g, neg, 2, T, 3, N, A, R, e, nullptr, nullptr) == RTO_E_INVALID);
        CHECK(doseFieldCPU(g, heavy, 2, T, 3, N, A, R, e, nullptr, nullptr) == RTO_E_INVALID);
        CHECK(doseFieldCPU(g, most, 2, T, 3, N, A, R, e, nullptr, nullptr) == RTO_OK);
        CHECK(doseFieldCPU(g, ok, 2, T, 0, N, A, R, e, nullptr, nullptr) == RTO_E_INVALID);
        CHECK(doseFieldCPU(g, ok, 2, longT.data(), 65, N, A, R, e, nullptr, nullptr) == RTO_E_INVALID);
        CHECK(doseFieldCPU(g, ok, 2, longT.data(), 64, N, A, R, e, nullptr, nullptr) == RTO_OK);
        CHECK(doseFieldCPU(g, ok, 2, over, 2, N, A, R, e, nullptr, nullptr) == RTO_E_INVALID);
        CHECK(doseFieldCPU(g, ok, 2, T, 3, 2, A, R, e, nullptr, nullptr) == RTO_E_INVALID);
        CHECK(doseFieldCPU(g, ok, 2, T, 3, -1, A, R, e, nullptr, nullptr) == RTO_E_INVALID);
        CHECK(doseFieldCPU(g, ok, 2, T, 3, N, 2, R, e, nullptr, nullptr) == RTO_E_INVALID);
        CHECK(doseFieldCPU(g, ok, 2, T, 3, N, -1, R, e, nullptr, nullptr) == RTO_E_INVALID);
        CHECK(doseFieldCPU(g, ok, 2, T, 3, N, A, 0, e, nullptr, nullptr) == RTO_E_INVALID && e.empty());
        CHECK(doseFieldCPU(g, outside, 2, T, 3, N, A, R, e, nullptr, nullptr, nullptr, &bad) == RTO_E_INVALID && bad == 1);
        CHECK(doseFieldCPU(VoxelGrid(), outside, 2, T, 3, N, A, R, e, nullptr, nullptr) == RTO_E_UNSUPPORTED);        // the grid before the sources' places
        CHECK(doseFieldCPU(VoxelGrid(), badneg, 2, T, 3, N, A, R, e, nullptr, nullptr) == RTO_E_INVALID);             // the arguments before the grid
        bad = -1;
        CHECK(doseFieldCPU(g, badneg, 2, over, 2, 7, 7, 0, e, nullptr, nullptr, nullptr, &bad) == RTO_E_INVALID && bad == -1);
    }
    if (g_fail) {
        std::fprintf(stderr, "dose selftest: %d checks failed\n", g_fail);
        return 1;
    }
    std::printf("dose selftest ok\n");
    return 0;
}
