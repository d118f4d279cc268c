// tools/parts_selftest.cpp -- the host layer's CPU form of the part-segmentation rule (host/Parts.cpp over host/Distance.cpp's
// transform) as a stand-alone program, so that it can run under AddressSanitizer and UBSan with no Python and no GPU
// (tools/sanitize_parts.sh).  Seeded random grids, two touching balls, a full and an empty grid, degenerate dims: every set,
// connectivity and a spread of ratios, the refusals included, with the invariants of the rule checked on every answer.  Exit code 0
// and "parts selftest ok" when all hold.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "Components.h"
#include "Parts.h"

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

static VoxelGrid balls(int dx, int dy, int dz, int r, int gap) {
    VoxelGrid g = make(dx, dy, dz, 0, 0.0);
    const int cx = (dx - gap) / 2;
    for (int z = 0; z < dz; z++)
        for (int y = 0; y < dy; y++)
            for (int x = 0; x < dx; x++)
                for (int c : { cx, cx + gap })
                    if ((x - c) * (x - c) + (y - dy / 2) * (y - dy / 2) + (z - dz / 2) * (z - dz / 2) <= r * r)
                        g.data[(size_t)x + (size_t)dx * ((size_t)y + (size_t)dy * (size_t)z)] = VoxelState::FILLED;
    return g;
}

// Calls f(v, u) for every ordered pair of adjacent voxels.
template <class F> static void adjacent(const VoxelGrid& g, int conn, F f) {
    for (int z = 0; z < g.dimZ; z++)
        for (int y = 0; y < g.dimY; y++)
            for (int x = 0; x < g.dimX; x++)
                for (int dz = -1; dz <= 1; dz++)
                    for (int dy = -1; dy <= 1; dy++)
                        for (int dx = -1; dx <= 1; dx++) {
                            const int k = (dx != 0) + (dy != 0) + (dz != 0);
                            if (k == 0 || (conn == RTO_CONN_FACE && k != 1)) continue;
                            const int a = x + dx, b = y + dy, c = z + dz;
                            if (a < 0 || a >= g.dimX || b < 0 || b >= g.dimY || c < 0 || c >= g.dimZ) continue;
                            f((int64_t)x + (int64_t)g.dimX * (y + (int64_t)g.dimY * z), (int64_t)a + (int64_t)g.dimX * (b + (int64_t)g.dimY * c));
                        }
}

static void check_segmentation(const VoxelGrid& g, int set, int conn, int ratio) {
    std::vector<int32_t> labels;
    std::vector<rto_part> parts;
    std::vector<rto_neck> necks;
    rto_parts_summary sum;
    const int64_t n = segmentPartsCPU(g, set, conn, ratio, labels, parts, necks, &sum);
    const int64_t nvox = (int64_t)g.dimX * g.dimY * g.dimZ;
    CHECK(n >= 0 && n == (int64_t)parts.size() && (int64_t)labels.size() == nvox);
    CHECK(sum.parts == n && sum.necks == (int64_t)necks.size() && sum.basins >= sum.parts);
    const VoxelState want = set == RTO_SET_SOLID ? VoxelState::FILLED : VoxelState::EMPTY;
    std::vector<int64_t> seen(parts.size(), 0);
    for (int64_t v = 0; v < nvox; v++) {
        CHECK((g.data[(size_t)v] == want) == (labels[(size_t)v] >= 0));
        const int32_t l = labels[(size_t)v];
        if (l < 0) continue;
        CHECK(l < n);
        if (seen[(size_t)l]++ == 0) CHECK(parts[(size_t)l].root == v);      // first voxel met = root
    }
    int64_t basins = 0;
    const int dims[3] = { g.dimX, g.dimY, g.dimZ };
    for (size_t i = 0; i < parts.size(); i++) {
        const rto_part& p = parts[i];
        basins += p.basins;
        CHECK(p.voxels == seen[i] && p.reserved == 0 && p.basins >= 1 && p.peak_h >= 1);
        CHECK(i == 0 || parts[i - 1].root < p.root);
        CHECK(p.peak >= 0 && p.peak < nvox && labels[(size_t)p.peak] == (int32_t)i);
        for (int a = 0; a < 3; a++) {
            CHECK(0 <= p.lo[a] && p.lo[a] <= p.hi[a] && p.hi[a] < dims[a]);
            CHECK(((p.touches >> a) & 1) == (p.lo[a] == 0));
            CHECK(((p.touches >> (3 + a)) & 1) == (p.hi[a] == dims[a] - 1));
        }
    }
    CHECK(basins == sum.basins);
    // necks: exactly the adjacent pairs of parts, each unordered voxel pair counted once
    std::map<std::pair<int32_t, int32_t>, int64_t> cross;
    adjacent(g, conn, [&](int64_t v, int64_t u) {
        const int32_t a = labels[(size_t)v], b = labels[(size_t)u];
        if (a >= 0 && b >= 0 && a < b) cross[{ a, b }]++;
    });
    CHECK(cross.size() == necks.size());
    int64_t pairs = 0;
    for (size_t i = 0; i < necks.size(); i++) {
        const rto_neck& k = necks[i];
        pairs += k.pairs;
        CHECK(k.part_lo < k.part_hi && k.reserved == 0 && k.h >= 1);
        CHECK(i == 0 || std::make_pair(necks[i - 1].part_lo, necks[i - 1].part_hi) < std::make_pair(k.part_lo, k.part_hi));
        auto it = cross.find({ k.part_lo, k.part_hi });
        CHECK(it != cross.end() && it->second == k.pairs);
        CHECK(k.at >= 0 && k.at < nvox && (labels[(size_t)k.at] == k.part_lo || labels[(size_t)k.at] == k.part_hi));
    }
    CHECK(pairs == sum.pairs);
    if (ratio == 0) {                                                     // the components, bit for bit
        std::vector<int32_t> cl;
        std::vector<rto_component> ct;
        CHECK(labelComponentsCPU(g, set, conn, cl, ct) == n && cl == labels && necks.empty());
    }
    if (ratio == RTO_PARTS_RATIO_MAX) CHECK(sum.basins == sum.parts);
    // the cut: changed is the number of voxels that differ, and no two former parts stay adjacent
    VoxelGrid e = g;
    const int64_t changed = splitAtNecksCPU(e, set, conn, ratio);
    int64_t diff = 0;
    for (int64_t v = 0; v < nvox; v++) diff += e.data[(size_t)v] != g.data[(size_t)v];
    CHECK(changed == diff && (changed == 0) == necks.empty());
    adjacent(e, conn, [&](int64_t v, int64_t u) {
        if (e.data[(size_t)v] == want && e.data[(size_t)u] == want) CHECK(labels[(size_t)v] == labels[(size_t)u]);
    });
}

static void check_grid(const VoxelGrid& g) {
    const int sets[2] = { RTO_SET_SOLID, RTO_SET_EMPTY }, conns[2] = { RTO_CONN_FACE, RTO_CONN_FULL };
    for (int set : sets)
        for (int conn : conns) {
            for (int ratio : { 0, 1, 600, 800, 1000, 1001 }) check_segmentation(g, set, conn, ratio);
            VoxelGrid e = g;
            CHECK(splitAtNecksCPU(e, set, conn, -1) == -1 && splitAtNecksCPU(e, set, conn, 1002) == -1);
            CHECK(e.data == g.data);
        }
    VoxelGrid e = g;
    CHECK(splitAtNecksCPU(e, 2, RTO_CONN_FACE, 800) == -1 && splitAtNecksCPU(e, RTO_SET_SOLID, 18, 800) == -1 && e.data == g.data);
}

int main() {
    const int shapes[][3] = { { 1, 1, 1 }, { 3, 2, 5 }, { 17, 9, 5 }, { 21, 20, 19 }, { 1, 40, 1 }, { 64, 1, 2 } };
    unsigned seed = 1;
    for (const auto& s : shapes)
        for (double fill : { 0.0, 0.3, 0.6, 0.85, 1.0 }) check_grid(make(s[0], s[1], s[2], seed++, fill));
    // two touching balls: one part at ratio 600, two of 2,063 voxels at ratio 800
    const VoxelGrid two = balls(40, 24, 24, 8, 13);
    check_grid(two);
    std::vector<int32_t> l;
    std::vector<rto_part> p;
    std::vector<rto_neck> k;
    CHECK(segmentPartsCPU(two, RTO_SET_SOLID, RTO_CONN_FACE, 600, l, p, k, nullptr) == 1 && p[0].voxels == 4126 && p[0].basins == 2);
    CHECK(segmentPartsCPU(two, RTO_SET_SOLID, RTO_CONN_FACE, 800, l, p, k, nullptr) == 2 && p[0].voxels == 2063 && p[1].voxels == 2063 && k.size() == 1);
    // a full grid: one part whose peak is voxel 0 at RTO_DIST_NONE
    const VoxelGrid full = make(7, 6, 5, 0, 1.0);
    CHECK(segmentPartsCPU(full, RTO_SET_SOLID, RTO_CONN_FULL, 1001, l, p, k, nullptr) == 1 && p[0].peak == 0 && p[0].peak_h == RTO_DIST_NONE);
    // no voxels at all: the transform's refusal is inherited
    VoxelGrid none;
    CHECK(segmentPartsCPU(none, RTO_SET_SOLID, RTO_CONN_FACE, 800, l, p, k, nullptr) == -1 && l.empty() && p.empty() && k.empty());
    if (g_fail) { std::fprintf(stderr, "parts selftest: %d checks failed\n", g_fail); return 1; }
    std::puts("parts selftest ok");
    return 0;
}
