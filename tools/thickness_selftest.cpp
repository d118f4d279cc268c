// tools/thickness_selftest.cpp -- the host layer's CPU form of the local-thickness rule (host/Thickness.cpp) as a stand-alone
// program, so that it can run under AddressSanitizer and UBSan with no Python and no GPU (tools/sanitize_thickness.sh).  Seeded
// random grids at 80 % and 90 % fill, full and empty grids, degenerate dims, walls of 1 to 9 voxels along each axis: both media and
// every cap against a plain triple loop over all pairs of voxels, the histogram and the summary, the refusals.  Exit code 0 and
// "thickness selftest ok" when all hold.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "Thickness.h"

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

static int64_t dist2(const VoxelGrid& g, int64_t a, int64_t b) {
    const int64_t x = (a % g.dimX) - (b % g.dimX), y = ((a / g.dimX) % g.dimY) - ((b / g.dimX) % g.dimY),
                  z = a / ((int64_t)g.dimX * g.dimY) - b / ((int64_t)g.dimX * g.dimY);
    return x * x + y * y + z * z;
}

// The rule as it is written: D by a minimum over all voxels of the other set, t2 by a maximum over all voxels of the grid.
static void check_field(const VoxelGrid& g, int medium, int64_t mq) {
    std::vector<int32_t> t2;
    std::vector<int64_t> bins;
    rto_thick_summary sm;
    CHECK(thicknessFieldCPU(g, medium, mq, t2, bins, &sm) == RTO_OK);
    const int64_t n = (int64_t)g.dimX * g.dimY * g.dimZ, c = mq * mq / 4096;
    CHECK((int64_t)t2.size() == n && (int64_t)bins.size() == c + 1);
    if ((int64_t)t2.size() != n || (int64_t)bins.size() != c + 1) return;
    const VoxelState in = medium == RTO_SET_SOLID ? VoxelState::FILLED : VoxelState::EMPTY;
    std::vector<int64_t> D((size_t)n, 0);
    for (int64_t q = 0; q < n; q++) {
        if (g.data[(size_t)q] != in) continue;
        int64_t m = c;
        for (int64_t u = 0; u < n; u++)
            if (g.data[(size_t)u] != in) m = std::min(m, dist2(g, q, u));
        D[(size_t)q] = m;
    }
    std::vector<int64_t> want((size_t)c + 1, 0);
    int64_t minT = -1, arg = -1, thin = 0, med = 0;
    for (int64_t p = 0; p < n; p++) {
        int64_t best = 0;
        if (g.data[(size_t)p] == in)
            for (int64_t q = 0; q < n; q++)
                if (dist2(g, p, q) < D[(size_t)q]) best = std::max(best, D[(size_t)q]);
        CHECK(t2[(size_t)p] == best);
        if (best == 0) continue;
        CHECK(best >= D[(size_t)p] && best <= c);
        want[(size_t)std::min(best, c)]++;
        med++;
        thin += best < c;
        if (minT < 0 || best < minT) { minT = best; arg = p; }
    }
    CHECK(bins == want && bins[0] == 0);
    CHECK(sm.min_t2 == minT && sm.argmin == arg && sm.thin == thin && sm.medium == med);
}

static VoxelGrid slab(int axis, int w) {
    const int dims[3] = { axis == 0 ? w + 6 : 5, axis == 1 ? w + 6 : 4, axis == 2 ? w + 6 : 3 };
    VoxelGrid g = make(dims[0], dims[1], dims[2], 0, 0.0);
    for (int z = 0; z < dims[2]; z++)
        for (int y = 0; y < dims[1]; y++)
            for (int x = 0; x < dims[0]; x++) {
                const int a = axis == 0 ? x : (axis == 1 ? y : z);
                if (a >= 3 && a < 3 + w) g.data[((size_t)z * dims[1] + y) * dims[0] + x] = VoxelState::FILLED;
            }
    return g;
}

int main() {
    const int64_t quanta[] = { 64, 96, 128, 256, 512, 515 };            // c = 1, 2, 4, 16, 64, 64
    const int shapes[][3] = { { 1, 1, 1 }, { 5, 3, 2 }, { 17, 9, 5 }, { 1, 40, 1 }, { 33, 1, 2 }, { 2, 3, 21 } };
    unsigned seed = 1;
    for (const auto& s : shapes)
        for (double fill : { 0.0, 0.8, 0.9, 1.0 }) {
            const VoxelGrid g = make(s[0], s[1], s[2], seed++, fill);
            for (int medium : { RTO_SET_SOLID, RTO_SET_EMPTY })
                for (int64_t mq : quanta) check_field(g, medium, mq);
        }
    for (int axis = 0; axis < 3; axis++)
        for (int w = 1; w <= 9; w++) {
            const VoxelGrid g = slab(axis, w);
            for (int64_t mq : { (int64_t)256, (int64_t)512 }) {
                check_field(g, RTO_SET_SOLID, mq);
                std::vector<int32_t> t2;
                std::vector<int64_t> bins;
                CHECK(thicknessFieldCPU(g, RTO_SET_SOLID, mq, t2, bins, nullptr) == RTO_OK);
                const int32_t want = (int32_t)std::min<int64_t>(((w + 1) / 2) * ((w + 1) / 2), mq * mq / 4096);
                for (size_t v = 0; v < t2.size(); v++) CHECK(t2[v] == (g.data[v] == VoxelState::FILLED ? want : 0));
            }
        }
    // the refusals, in rto_thickness_field's order
    const VoxelGrid g = make(5, 4, 3, 7, 0.5);
    std::vector<int32_t> t2;
    std::vector<int64_t> bins;
    CHECK(thicknessFieldCPU(g, 2, 64, t2, bins, nullptr) == RTO_E_INVALID && thicknessFieldCPU(g, -1, 1 << 28, t2, bins, nullptr) == RTO_E_INVALID);
    CHECK(thicknessFieldCPU(g, 1, -1, t2, bins, nullptr) == RTO_E_INVALID && thicknessFieldCPU(g, 1, (1ll << 28) + 1, t2, bins, nullptr) == RTO_E_INVALID);
    CHECK(thicknessFieldCPU(g, 1, 0, t2, bins, nullptr) == RTO_E_INVALID && thicknessFieldCPU(g, 0, 63, t2, bins, nullptr) == RTO_E_INVALID);
    CHECK(thicknessFieldCPU(g, 1, 516, t2, bins, nullptr) == RTO_E_UNSUPPORTED && thicknessFieldCPU(g, 0, 1 << 28, t2, bins, nullptr) == RTO_E_UNSUPPORTED);
    CHECK(t2.empty() && bins.empty());
    VoxelGrid none;
    CHECK(thicknessFieldCPU(none, 1, 64, t2, bins, nullptr) == RTO_E_UNSUPPORTED);
    VoxelGrid line = make(46342, 1, 1, 0, 0.0);
    CHECK(thicknessFieldCPU(line, 1, 64, t2, bins, nullptr) == RTO_E_UNSUPPORTED && t2.empty());
    if (g_fail) { std::fprintf(stderr, "thickness selftest: %d checks failed\n", g_fail); return 1; }
    std::puts("thickness selftest ok");
    return 0;
}
