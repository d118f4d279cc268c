// tools/skeleton_selftest.cpp -- the host layer's CPU form of the skeleton rule (host/Skeleton.cpp) as a stand-alone program, so that
// it can run under AddressSanitizer and UBSan with no Python and no GPU (tools/sanitize_skeleton.sh).  The simple-point test against
// a walk over the 27 cells with a stack (random blocks, every block of at most 3 voxels and their complements, both
// connectivities); the field against the rule as it is written (M by a scan of the whole grid in every pass, every sub-step decided
// on a copy of X and applied at once) on seeded random grids, full grids and degenerate dims, for every connectivity and mode, with
// anchors and pass limits; the edit, its idempotence and the refusals.  Exit code 0 and "skeleton selftest ok" when all hold.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "Skeleton.h"

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

static int axes(int a, int b) {         // on how many axes cells a and b differ, and 9 when they are more than one step apart
    int n = 0;
    const int d[3] = { a % 3 - b % 3, (a / 3) % 3 - (b / 3) % 3, a / 9 - b / 9 };
    for (int k = 0; k < 3; k++) {
        if (d[k] < -1 || d[k] > 1) return 9;
        n += d[k] != 0;
    }
    return n;
}

// The cells of `inside` that a walk from `start` reaches, by steps that change at most `most` axes.
static uint32_t walk(uint32_t inside, int start, int most) {
    uint32_t seen = 1u << start;
    std::vector<int> stack{ start };
    while (!stack.empty()) {
        const int a = stack.back();
        stack.pop_back();
        for (int b = 0; b < 27; b++)
            if (((inside >> b) & 1u) && !((seen >> b) & 1u) && axes(a, b) >= 1 && axes(a, b) <= most) { seen |= 1u << b; stack.push_back(b); }
    }
    return seen;
}

static bool simple_slow(uint32_t mask, int connectivity) {
    uint32_t n26 = 0, n18 = 0, n6 = 0;
    for (int b = 0; b < 27; b++) {
        const int c = axes(b, 13);
        if (c >= 1) n26 |= 1u << b;
        if (c == 1 || c == 2) n18 |= 1u << b;
        if (c == 1) n6 |= 1u << b;
    }
    const uint32_t in = mask & n26, out = ~mask & n26;
    const uint32_t big = connectivity == RTO_CONN_FULL ? in : out, small = connectivity == RTO_CONN_FULL ? out : in;
    if (!big) return false;
    int first = 0;
    while (!((big >> first) & 1u)) first++;
    if (walk(big, first, 3) != big) return false;
    const uint32_t s18 = small & n18, s6 = small & n6;
    if (!s6) return false;
    first = 0;
    while (!((s6 >> first) & 1u)) first++;
    return (walk(s18, first, 1) & s6) == s6;
}

// The rule as it is written.
static void rule(const VoxelGrid& g, int set, int conn, int mode, const std::vector<int64_t>& anchors, int64_t maxPasses, std::vector<int32_t>& k) {
    const int dx = g.dimX, dy = g.dimY, dz = g.dimZ;
    const size_t n = (size_t)dx * dy * dz;
    const VoxelState want = set == RTO_SET_SOLID ? VoxelState::FILLED : VoxelState::EMPTY;
    std::vector<char> X(n), A(n, 0), M(n);
    k.assign(n, -1);
    for (size_t v = 0; v < n; v++) { X[v] = g.data[v] == want; if (X[v]) k[v] = 0; }
    for (int64_t a : anchors) A[(size_t)a] = 1;
    auto block = [&](const std::vector<char>& S, int x, int y, int z) {
        uint32_t m = 0;
        for (int b = 0; b < 27; b++) {
            const int nx = x + b % 3 - 1, ny = y + (b / 3) % 3 - 1, nz = z + b / 9 - 1;
            if (nx >= 0 && nx < dx && ny >= 0 && ny < dy && nz >= 0 && nz < dz && S[((size_t)nz * dy + ny) * dx + nx]) m |= 1u << b;
        }
        return m;
    };
    for (int64_t p = 1; p <= maxPasses; p++) {
        for (int z = 0; z < dz; z++)
            for (int y = 0; y < dy; y++)
                for (int x = 0; x < dx; x++) {
                    const size_t v = ((size_t)z * dy + y) * dx + x;
                    bool open = false;
                    const uint32_t m = block(X, x, y, z);
                    for (int b = 0; b < 27; b++) {
                        const int c = axes(b, 13);
                        if (c >= 1 && c <= (conn == RTO_CONN_FULL ? 1 : 3) && !((m >> b) & 1u)) open = true;
                    }
                    M[v] = X[v] && open;
                }
        bool any = false;
        for (int s = 0; s < 8; s++) {
            const std::vector<char> was = X;
            for (int z = 0; z < dz; z++)
                for (int y = 0; y < dy; y++)
                    for (int x = 0; x < dx; x++) {
                        const size_t v = ((size_t)z * dy + y) * dx + x;
                        if ((x & 1) + 2 * (y & 1) + 4 * (z & 1) != s || !M[v] || A[v] || !was[v]) continue;
                        const uint32_t m = block(was, x, y, z) & ~(1u << 13);
                        if (mode == RTO_SKEL_CURVE && m && !(m & (m - 1))) continue;
                        if (!simple_slow(m, conn)) continue;
                        X[v] = 0; k[v] = (int32_t)p; any = true;
                    }
        }
        if (!any) break;
    }
}

static void check_field(const VoxelGrid& g, int set, int conn, int mode, const std::vector<int64_t>& anchors, int64_t maxPasses) {
    std::vector<int32_t> k, want;
    rto_skel_summary sm;
    CHECK(skeletonFieldCPU(g, set, conn, mode, anchors.empty() ? nullptr : anchors.data(), (int64_t)anchors.size(), maxPasses, k, &sm) == RTO_OK);
    rule(g, set, conn, mode, anchors, maxPasses, want);
    CHECK(k == want);
    int64_t kept = 0, gone = 0, top = 0;
    for (int32_t q : want) { kept += q == 0; gone += q > 0; top = std::max<int64_t>(top, q); }
    CHECK(sm.kept == kept && sm.removed == gone && sm.passes == top && sm.reserved == 0);
    for (int64_t a : anchors) CHECK(k[(size_t)a] <= 0);
    // the edit, and a second one that changes nothing
    VoxelGrid e = g;
    CHECK(thinCPU(e, set, conn, mode, anchors.empty() ? nullptr : anchors.data(), (int64_t)anchors.size(), maxPasses) == gone);
    for (size_t v = 0; v < k.size(); v++) CHECK((e.data[v] != g.data[v]) == (k[v] > 0));
    if (maxPasses >= RTO_SKEL_NO_LIMIT)
        CHECK(thinCPU(e, set, conn, mode, anchors.empty() ? nullptr : anchors.data(), (int64_t)anchors.size(), maxPasses) == 0);
}

int main() {
    // the simple-point test
    unsigned s = 99u;
    for (int conn : { RTO_CONN_FACE, RTO_CONN_FULL }) {
        for (int i = 0; i < 20000; i++) {
            s = s * 1664525u + 1013904223u;
            const uint32_t m = (s >> 5) & ((1u << 27) - 1u);
            CHECK(skeletonSimpleCPU(m, conn) == simple_slow(m, conn));
        }
        for (int a = 0; a < 27; a++)
            for (int b = a; b < 27; b++)
                for (int c = b; c < 27; c++) {
                    const uint32_t m = (1u << a) | (1u << b) | (1u << c);
                    CHECK(skeletonSimpleCPU(m, conn) == simple_slow(m, conn));
                    CHECK(skeletonSimpleCPU(~m & ((1u << 27) - 1u), conn) == simple_slow(~m, conn));
                }
        CHECK(!skeletonSimpleCPU(0u, conn) && !skeletonSimpleCPU((1u << 27) - 1u, conn));
    }
    // the field
    const int shapes[][3] = { { 1, 1, 1 }, { 5, 3, 2 }, { 17, 9, 5 }, { 1, 40, 1 }, { 40, 1, 1 }, { 33, 1, 2 }, { 2, 3, 21 }, { 12, 11, 10 } };
    unsigned seed = 1;
    for (const auto& sh : shapes)
        for (double fill : { 0.0, 0.7, 0.9, 1.0 }) {
            const VoxelGrid g = make(sh[0], sh[1], sh[2], seed++, fill);
            const int64_t n = (int64_t)sh[0] * sh[1] * sh[2];
            const std::vector<int64_t> anchors{ 0, n - 1, n / 2, n / 2, n / 3 };
            for (int set : { RTO_SET_SOLID, RTO_SET_EMPTY }) {
                for (int64_t limit : { (int64_t)1, (int64_t)3, (int64_t)RTO_SKEL_NO_LIMIT }) {
                    check_field(g, set, RTO_CONN_FULL, RTO_SKEL_TOPOLOGY, {}, limit);
                    check_field(g, set, RTO_CONN_FULL, RTO_SKEL_CURVE, {}, limit);
                    check_field(g, set, RTO_CONN_FACE, RTO_SKEL_TOPOLOGY, {}, limit);
                }
                check_field(g, set, RTO_CONN_FULL, RTO_SKEL_TOPOLOGY, anchors, RTO_SKEL_NO_LIMIT);
                check_field(g, set, RTO_CONN_FACE, RTO_SKEL_TOPOLOGY, anchors, (int64_t)RTO_SKEL_NO_LIMIT + 5);
            }
        }
    // the refusals, in rto_skeleton_field's order
    const VoxelGrid g = make(5, 4, 3, 7, 0.5);
    std::vector<int32_t> k;
    const int64_t in[1] = { 3 }, below[1] = { -1 }, beyond[1] = { 60 };
    CHECK(skeletonFieldCPU(g, 2, 26, 0, nullptr, 0, 1, k, nullptr) == RTO_E_INVALID);
    CHECK(skeletonFieldCPU(g, 1, 18, 0, nullptr, 0, 1, k, nullptr) == RTO_E_INVALID);
    CHECK(skeletonFieldCPU(g, 1, 26, 2, nullptr, 0, 1, k, nullptr) == RTO_E_INVALID);
    CHECK(skeletonFieldCPU(g, 1, 6, RTO_SKEL_CURVE, nullptr, 0, 1, k, nullptr) == RTO_E_INVALID);
    CHECK(skeletonFieldCPU(g, 1, 26, 0, in, -1, 1, k, nullptr) == RTO_E_INVALID);
    CHECK(skeletonFieldCPU(g, 1, 26, 0, nullptr, 1, 1, k, nullptr) == RTO_E_INVALID);
    CHECK(skeletonFieldCPU(g, 1, 26, 0, in, 1, 0, k, nullptr) == RTO_E_INVALID);
    CHECK(skeletonFieldCPU(g, 1, 26, 0, below, 1, 1, k, nullptr) == RTO_E_INVALID);
    CHECK(skeletonFieldCPU(g, 1, 26, 0, beyond, 1, 1, k, nullptr) == RTO_E_INVALID);
    CHECK(k.empty());
    VoxelGrid e = g;
    CHECK(thinCPU(e, 1, 6, RTO_SKEL_CURVE, nullptr, 0, 1) == RTO_E_INVALID && e.data == g.data);
    VoxelGrid none;
    CHECK(skeletonFieldCPU(none, 1, 26, 0, nullptr, 0, 1, k, nullptr) == RTO_E_UNSUPPORTED);
    CHECK(skeletonFieldCPU(g, 1, 26, 0, in, 1, 1, k, nullptr) == RTO_OK && k.size() == 60);
    if (g_fail) { std::fprintf(stderr, "skeleton selftest: %d checks failed\n", g_fail); return 1; }
    std::puts("skeleton selftest ok");
    return 0;
}
