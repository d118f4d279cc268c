// tools/distance_selftest.cpp -- the host layer's CPU form of the distance-field rule (host/Distance.cpp) as a stand-alone program,
// so that it can run under AddressSanitizer and UBSan with no Python and no GPU (tools/sanitize_distance.sh).  Seeded random grids,
// a single voxel in a corner, full and empty grids, degenerate dims, the longest line the 32-bit field allows: every set and cap
// against a brute-force minimum, the four operations with their algebra, the refusals.  Exit code 0 and "distance selftest ok"
// when all hold.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "Distance.h"

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

static void check_field(const VoxelGrid& g, int set, int64_t mq) {
    std::vector<int32_t> d2;
    rto_dist_summary sm;
    CHECK(distanceFieldCPU(g, set, mq, d2, &sm));
    const int64_t n = (int64_t)g.dimX * g.dimY * g.dimZ;
    CHECK((int64_t)d2.size() == n);
    const VoxelState want = set == RTO_SET_SOLID ? VoxelState::FILLED : VoxelState::EMPTY;
    int64_t finite = 0, best = -1, arg = -1;
    for (int64_t v = 0; v < n; v++) {
        const int x = (int)(v % g.dimX), y = (int)((v / g.dimX) % g.dimY), z = (int)(v / ((int64_t)g.dimX * g.dimY));
        int64_t m = RTO_DIST_NONE;
        for (int64_t u = 0; u < n; u++) {
            if (g.data[(size_t)u] != want) continue;
            const int64_t a = x - (int)(u % g.dimX), b = y - (int)((u / g.dimX) % g.dimY), c = z - (int)(u / ((int64_t)g.dimX * g.dimY));
            m = std::min<int64_t>(m, a * a + b * b + c * c);
        }
        if (mq >= 0 && m != RTO_DIST_NONE && 4096 * m > mq * mq) m = RTO_DIST_NONE;
        CHECK(d2[(size_t)v] == m);
        if (m != RTO_DIST_NONE) { finite++; if (m > best) { best = m; arg = v; } }
    }
    CHECK(sm.finite == finite && sm.max_d2 == best && sm.argmax == arg && sm.reserved == 0);
}

static bool inside(const VoxelGrid& a, const VoxelGrid& b) {
    for (size_t v = 0; v < a.data.size(); v++)
        if (a.data[v] == VoxelState::FILLED && b.data[v] != VoxelState::FILLED) return false;
    return true;
}

static void check_morphology(const VoxelGrid& g, int64_t rq) {
    VoxelGrid out[4];
    for (int op = RTO_MORPH_DILATE; op <= RTO_MORPH_CLOSE; op++) {
        out[op] = g;
        const int64_t changed = applyMorphologyCPU(out[op], op, rq);
        int64_t diff = 0;
        for (size_t v = 0; v < g.data.size(); v++) diff += out[op].data[v] != g.data[v];
        CHECK(changed == diff);
        if (rq == 0) CHECK(changed == 0);
    }
    CHECK(inside(g, out[RTO_MORPH_DILATE]) && inside(out[RTO_MORPH_ERODE], g) && inside(g, out[RTO_MORPH_CLOSE]) && inside(out[RTO_MORPH_OPEN], g));
    VoxelGrid again = out[RTO_MORPH_CLOSE];
    CHECK(applyMorphologyCPU(again, RTO_MORPH_CLOSE, rq) == 0);
    again = out[RTO_MORPH_OPEN];
    CHECK(applyMorphologyCPU(again, RTO_MORPH_OPEN, rq) == 0);
    VoxelGrid ed = out[RTO_MORPH_DILATE];                               // the adjunction with Y = dilate(X): X inside erode(Y)
    applyMorphologyCPU(ed, RTO_MORPH_ERODE, rq);
    CHECK(inside(g, ed));
    VoxelGrid e = g;
    CHECK(applyMorphologyCPU(e, 4, rq) == -1 && applyMorphologyCPU(e, -1, rq) == -1 && applyMorphologyCPU(e, 0, -1) == -1);
    CHECK(applyMorphologyCPU(e, 0, (1ll << 28) + 1) == -1 && e.data == g.data);
}

int main() {
    const int shapes[][3] = { { 1, 1, 1 }, { 3, 2, 5 }, { 17, 9, 5 }, { 1, 40, 1 }, { 64, 1, 2 }, { 2, 3, 33 } };
    unsigned seed = 1;
    for (const auto& s : shapes)
        for (double fill : { 0.0, 0.02, 0.2, 0.5, 1.0 }) {
            const VoxelGrid g = make(s[0], s[1], s[2], seed++, fill);
            for (int set : { RTO_SET_SOLID, RTO_SET_EMPTY })
                for (int64_t mq : { (int64_t)-1, (int64_t)0, (int64_t)64, (int64_t)160, (int64_t)191, (int64_t)192, (int64_t)1000 }) check_field(g, set, mq);
            for (int64_t rq : { (int64_t)0, (int64_t)64, (int64_t)96, (int64_t)160, (int64_t)(1 << 28) }) check_morphology(g, rq);
        }
    VoxelGrid corner = make(33, 17, 9, 0, 0.0);
    corner.data[0] = VoxelState::FILLED;
    check_field(corner, RTO_SET_SOLID, -1);
    // the longest line the field allows, and one voxel more
    VoxelGrid line = make(46341, 1, 1, 0, 0.0);
    line.data[0] = VoxelState::FILLED;
    std::vector<int32_t> d2;
    rto_dist_summary sm;
    CHECK(distanceFieldCPU(line, RTO_SET_SOLID, -1, d2, &sm) && sm.max_d2 == 46340ll * 46340ll && sm.argmax == 46340 && d2[46340] == 2147395600);
    line = make(46342, 1, 1, 0, 0.0);
    CHECK(!distanceFieldCPU(line, RTO_SET_SOLID, -1, d2, nullptr) && d2.empty() && applyMorphologyCPU(line, RTO_MORPH_DILATE, 64) == -1);
    VoxelGrid none;
    CHECK(!distanceFieldCPU(none, RTO_SET_SOLID, -1, d2, nullptr) && !distanceFieldCPU(corner, 2, -1, d2, nullptr));
    int64_t mq = 0;
    CHECK(quantizeDistanceCPU(3.0f / 64.0f, 1.0f / 64.0f, mq) && mq == 192);
    CHECK(quantizeDistanceCPU(INFINITY, 1.0f, mq) && mq == -1);
    CHECK(!quantizeDistanceCPU(NAN, 1.0f, mq) && !quantizeDistanceCPU(-1.0f, 1.0f, mq) && !quantizeDistanceCPU(4194305.0f, 1.0f, mq));
    CHECK(quantizeDistanceCPU(4194304.0f, 1.0f, mq) && mq == (1ll << 28));
    if (g_fail) { std::fprintf(stderr, "distance selftest: %d checks failed\n", g_fail); return 1; }
    std::puts("distance selftest ok");
    return 0;
}
