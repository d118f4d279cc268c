// tools/components_selftest.cpp -- the host layer's CPU form of the connected-component rule (host/Components.cpp) as a
// stand-alone program, so that it can run under AddressSanitizer and UBSan with no Python and no GPU (tools/sanitize_components.sh).
// Seeded random grids, a hollow box, a full and an empty grid, degenerate dims: every set, connectivity and selection, the
// refusals included, with the invariants of the rule checked on every answer.  Exit code 0 and "components selftest ok" when all hold.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "Components.h"

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

static void check_labelling(const VoxelGrid& g, int set, int conn) {
    std::vector<int32_t> labels;
    std::vector<rto_component> table;
    const int64_t n = labelComponentsCPU(g, set, conn, labels, table);
    const int64_t nvox = (int64_t)g.dimX * g.dimY * g.dimZ;
    CHECK(n >= 0 && n == (int64_t)table.size() && (int64_t)labels.size() == nvox);
    int64_t inSet = 0, sum = 0;
    std::vector<int64_t> seen(table.size(), 0);
    const VoxelState want = set == RTO_SET_SOLID ? VoxelState::FILLED : VoxelState::EMPTY;
    for (int64_t v = 0; v < nvox; v++) {
        const bool in = g.data[(size_t)v] == want;
        inSet += in;
        CHECK(in == (labels[(size_t)v] >= 0));
        if (labels[(size_t)v] >= 0) {
            CHECK(labels[(size_t)v] < n);
            if (seen[(size_t)labels[(size_t)v]]++ == 0) CHECK(table[(size_t)labels[(size_t)v]].root == v);   // first voxel met = root
        }
    }
    for (size_t i = 0; i < table.size(); i++) {
        sum += table[i].voxels;
        CHECK(table[i].voxels == seen[i] && table[i].reserved == 0);
        CHECK(i == 0 || table[i - 1].root < table[i].root);
        const int dims[3] = { g.dimX, g.dimY, g.dimZ };
        for (int a = 0; a < 3; a++) {
            CHECK(0 <= table[i].lo[a] && table[i].lo[a] <= table[i].hi[a] && table[i].hi[a] < dims[a]);
            CHECK(((table[i].touches >> a) & 1) == (table[i].lo[a] == 0));
            CHECK(((table[i].touches >> (3 + a)) & 1) == (table[i].hi[a] == dims[a] - 1));
        }
    }
    CHECK(sum == inSet);
}

static void check_selections(const VoxelGrid& g) {
    const int64_t nvox = (int64_t)g.dimX * g.dimY * g.dimZ;
    const int sets[2] = { RTO_SET_SOLID, RTO_SET_EMPTY }, conns[2] = { RTO_CONN_FACE, RTO_CONN_FULL };
    for (int set : sets)
        for (int conn : conns) {
            check_labelling(g, set, conn);
            for (int sel = RTO_SELECT_SMALLER_THAN; sel <= RTO_SELECT_NOT_CONTAINING; sel++)
                for (int64_t arg : { (int64_t)0, (int64_t)1, (int64_t)5, nvox / 2, nvox - 1 }) {
                    if (arg < 0) continue;
                    VoxelGrid e = g;
                    const int64_t changed = applyComponentSelectionCPU(e, set, conn, sel, arg);
                    if ((sel == RTO_SELECT_CONTAINING || sel == RTO_SELECT_NOT_CONTAINING) && arg >= nvox) { CHECK(changed == -1); continue; }
                    CHECK(changed >= 0);
                    int64_t diff = 0;
                    for (int64_t v = 0; v < nvox; v++) diff += e.data[(size_t)v] != g.data[(size_t)v];
                    CHECK(diff == changed);
                }
            VoxelGrid e = g;
            CHECK(applyComponentSelectionCPU(e, set, conn, 5, 0) == -1);
            CHECK(applyComponentSelectionCPU(e, set, conn, -1, 0) == -1);
            CHECK(applyComponentSelectionCPU(e, set, conn, RTO_SELECT_SMALLER_THAN, -1) == -1);
            CHECK(applyComponentSelectionCPU(e, set, conn, RTO_SELECT_CONTAINING, -1) == -1);
            CHECK(applyComponentSelectionCPU(e, set, conn, RTO_SELECT_CONTAINING, nvox) == -1);
            CHECK(applyComponentSelectionCPU(e, set, conn, RTO_SELECT_NOT_CONTAINING, nvox + 3) == -1);
            CHECK(e.data == g.data);
        }
    VoxelGrid e = g;
    CHECK(applyComponentSelectionCPU(e, 2, RTO_CONN_FACE, 0, 0) == -1 && applyComponentSelectionCPU(e, RTO_SET_SOLID, 18, 0, 0) == -1);
}

int main() {
    const int shapes[][3] = { { 1, 1, 1 }, { 3, 2, 5 }, { 17, 9, 5 }, { 33, 33, 33 }, { 1, 40, 1 }, { 64, 1, 2 } };
    unsigned seed = 1;
    for (const auto& s : shapes)
        for (double fill : { 0.0, 0.2, 0.31, 0.5, 0.7, 1.0 }) check_selections(make(s[0], s[1], s[2], seed++, fill));
    // a hollow box: its inside is the one enclosed empty component
    VoxelGrid box = make(9, 9, 9, 0, 0.0);
    for (int z = 2; z < 7; z++)
        for (int y = 2; y < 7; y++)
            for (int x = 2; x < 7; x++)
                if (x == 2 || x == 6 || y == 2 || y == 6 || z == 2 || z == 6) box.data[(size_t)box.index(x, y, z)] = VoxelState::FILLED;
    check_selections(box);
    VoxelGrid filled = box;
    CHECK(applyComponentSelectionCPU(filled, RTO_SET_EMPTY, RTO_CONN_FACE, RTO_SELECT_ENCLOSED, 0) == 27);
    box.data[(size_t)box.index(6, 4, 4)] = VoxelState::EMPTY;
    CHECK(applyComponentSelectionCPU(box, RTO_SET_EMPTY, RTO_CONN_FACE, RTO_SELECT_ENCLOSED, 0) == 0);
    // no voxels at all
    VoxelGrid none;
    std::vector<int32_t> l;
    std::vector<rto_component> t;
    CHECK(labelComponentsCPU(none, RTO_SET_SOLID, RTO_CONN_FACE, l, t) == 0 && l.empty() && t.empty());
    if (g_fail) { std::fprintf(stderr, "components selftest: %d checks failed\n", g_fail); return 1; }
    std::puts("components selftest ok");
    return 0;
}
