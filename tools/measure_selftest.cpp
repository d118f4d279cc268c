// tools/measure_selftest.cpp -- the host layer's CPU form of the component-measure rule (host/Measure.cpp) as a stand-alone
// program, so that it can run under AddressSanitizer and UBSan with no Python and no GPU (tools/sanitize_measure.sh).  Seeded random
// grids at 20 %, 50 % and 80 % fill, full and empty grids, degenerate dims, a cube, a shell, a ring and a corner pair: both sets and
// both connectivities against a per-component brute force, where each component alone in an empty grid is measured by the
// whole-set rule (cells marked on their own lattices, no attribution to voxels); the total row; the closed forms; the refusals.
// Exit code 0 and "measure selftest ok" when all hold.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "Measure.h"

static int g_fail = 0;
#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); g_fail++; } \
    } while (0)

struct Grid {
    int dx, dy, dz;
    std::vector<unsigned char> v;
    size_t at(int i, int j, int k) const { return ((size_t)k * dy + j) * dx + i; }
    bool inside(int i, int j, int k) const { return i >= 0 && i < dx && j >= 0 && j < dy && k >= 0 && k < dz; }
};

static Grid make(int dx, int dy, int dz, unsigned seed, double fill) {
    Grid g{ dx, dy, dz, std::vector<unsigned char>((size_t)dx * dy * dz) };
    unsigned s = seed * 2654435761u + 12345u;
    for (auto& v : g.v) {
        s = s * 1664525u + 1013904223u;
        v = (double)(s >> 8) / (double)(1u << 24) < fill ? 1 : 0;
    }
    return g;
}

// Labels by flood fill; any numbering serves the measures.
static int64_t label(const Grid& g, int set, int conn, std::vector<int32_t>& labels) {
    labels.assign(g.v.size(), -1);
    int64_t count = 0;
    std::vector<int> stack;
    for (int k0 = 0; k0 < g.dz; k0++)
        for (int j0 = 0; j0 < g.dy; j0++)
            for (int i0 = 0; i0 < g.dx; i0++) {
                if (g.v[g.at(i0, j0, k0)] != set || labels[g.at(i0, j0, k0)] >= 0) continue;
                labels[g.at(i0, j0, k0)] = (int32_t)count;
                stack.assign({ i0, j0, k0 });
                while (!stack.empty()) {
                    const int k = stack.back(); stack.pop_back();
                    const int j = stack.back(); stack.pop_back();
                    const int i = stack.back(); stack.pop_back();
                    for (int c = -1; c <= 1; c++)
                        for (int b = -1; b <= 1; b++)
                            for (int a = -1; a <= 1; a++) {
                                const int steps = (a != 0) + (b != 0) + (c != 0);
                                if (steps == 0 || (conn == RTO_CONN_FACE && steps != 1)) continue;
                                if (!g.inside(i + a, j + b, k + c)) continue;
                                const size_t w = g.at(i + a, j + b, k + c);
                                if (g.v[w] != set || labels[w] >= 0) continue;
                                labels[w] = (int32_t)count;
                                stack.insert(stack.end(), { i + a, j + b, k + c });
                            }
                }
                count++;
            }
    return count;
}

// The whole-set rule for the voxels with labels[v] == c, as if nothing else were in the grid.
static rto_measure brute(const Grid& g, const std::vector<int32_t>& labels, int32_t c, int conn) {
    rto_measure m;
    std::memset(&m, 0, sizeof m);
    auto in = [&](int i, int j, int k) { return g.inside(i, j, k) && labels[g.at(i, j, k)] == c; };
    const int X = g.dx, Y = g.dy, Z = g.dz;
    // lattices: vertices (X+1)(Y+1)(Z+1); edges and faces by the axes they span
    auto lattice = [&](int sx, int sy, int sz) {
        // a cell spans a voxel on the axes with s = 1 and sits on a lattice plane on the others
        const int nx = X + 1 - sx, ny = Y + 1 - sy, nz = Z + 1 - sz;
        std::vector<char> mark((size_t)nx * ny * nz, 0);
        for (int k = 0; k < Z; k++)
            for (int j = 0; j < Y; j++)
                for (int i = 0; i < X; i++) {
                    if (!in(i, j, k)) continue;
                    for (int c2 = 0; c2 <= 1 - sz; c2++)
                        for (int b = 0; b <= 1 - sy; b++)
                            for (int a = 0; a <= 1 - sx; a++) mark[((size_t)(k + c2) * ny + (j + b)) * nx + (i + a)] = 1;
                }
        int64_t n = 0;
        for (char v : mark) n += v;
        return n;
    };
    for (int k = 0; k < Z; k++)
        for (int j = 0; j < Y; j++)
            for (int i = 0; i < X; i++) {
                if (!in(i, j, k)) continue;
                m.voxels++;
                m.faces[0] += !in(i - 1, j, k); m.faces[1] += !in(i + 1, j, k);
                m.faces[2] += !in(i, j - 1, k); m.faces[3] += !in(i, j + 1, k);
                m.faces[4] += !in(i, j, k - 1); m.faces[5] += !in(i, j, k + 1);
                m.sum[0] += i; m.sum[1] += j; m.sum[2] += k;
                m.sum2[0] += (int64_t)i * i; m.sum2[1] += (int64_t)j * j; m.sum2[2] += (int64_t)k * k;
                m.sum2[3] += (int64_t)i * j; m.sum2[4] += (int64_t)i * k; m.sum2[5] += (int64_t)j * k;
                if (conn == RTO_CONN_FACE) {
                    const bool x = in(i + 1, j, k), y = in(i, j + 1, k), z = in(i, j, k + 1);
                    const bool xy = in(i + 1, j + 1, k), xz = in(i + 1, j, k + 1), yz = in(i, j + 1, k + 1);
                    m.cells[0] += x + y + z;
                    m.cells[1] += (x && y && xy) + (x && z && xz) + (y && z && yz);
                    m.cells[2] += x && y && z && xy && xz && yz && in(i + 1, j + 1, k + 1);
                }
            }
    if (conn == RTO_CONN_FULL) {
        m.cells[0] = lattice(0, 0, 0);
        m.cells[1] = lattice(1, 0, 0) + lattice(0, 1, 0) + lattice(0, 0, 1);
        m.cells[2] = lattice(1, 1, 0) + lattice(1, 0, 1) + lattice(0, 1, 1);
        m.euler = m.cells[0] - m.cells[1] + m.cells[2] - m.voxels;
    } else {
        m.euler = m.voxels - m.cells[0] + m.cells[1] - m.cells[2];
    }
    return m;
}

static rto_measure check_grid(const Grid& g, int set, int conn) {
    std::vector<int32_t> labels;
    const int64_t count = label(g, set, conn, labels);
    std::vector<rto_measure> table;
    rto_measure total, sum;
    std::memset(&sum, 0, sizeof sum);
    CHECK(measureComponentsCPU(g.dx, g.dy, g.dz, labels.data(), count, conn, table, &total) == RTO_OK);
    CHECK((int64_t)table.size() == count);
    if ((int64_t)table.size() != count) return sum;
    for (int64_t c = 0; c < count; c++) {
        const rto_measure want = brute(g, labels, (int32_t)c, conn);
        CHECK(std::memcmp(&table[(size_t)c], &want, sizeof want) == 0);
        for (size_t f = 0; f < sizeof(rto_measure) / 8; f++) reinterpret_cast<int64_t*>(&sum)[f] += reinterpret_cast<const int64_t*>(&want)[f];
        if (conn == RTO_CONN_FULL) {
            int64_t faces = 0;
            for (int d = 0; d < 6; d++) faces += want.faces[d];
            CHECK(2 * want.cells[2] == 6 * want.voxels + faces);
        }
    }
    CHECK(std::memcmp(&total, &sum, sizeof sum) == 0);
    return total;
}

int main() {
    const int shapes[][3] = { { 1, 1, 1 }, { 5, 3, 2 }, { 11, 10, 9 }, { 1, 40, 1 }, { 33, 1, 2 }, { 2, 3, 21 } };
    unsigned seed = 1;
    for (const auto& s : shapes)
        for (double fill : { 0.0, 0.2, 0.5, 0.8, 1.0 }) {
            const Grid g = make(s[0], s[1], s[2], seed++, fill);
            for (int set : { RTO_SET_SOLID, RTO_SET_EMPTY })
                for (int conn : { RTO_CONN_FACE, RTO_CONN_FULL }) check_grid(g, set, conn);
        }
    // the closed forms: a 5^3 cube, the same without its centre, a 5 x 5 ring, two voxels touching at a corner
    Grid cube = make(7, 7, 7, 0, 0.0);
    for (int k = 1; k < 6; k++)
        for (int j = 1; j < 6; j++)
            for (int i = 1; i < 6; i++) cube.v[cube.at(i, j, k)] = 1;
    Grid shell = cube;
    shell.v[shell.at(3, 3, 3)] = 0;
    Grid ring = make(7, 7, 3, 0, 0.0);
    for (int j = 1; j < 6; j++)
        for (int i = 1; i < 6; i++) ring.v[ring.at(i, j, 1)] = (i == 1 || i == 5 || j == 1 || j == 5) ? 1 : 0;
    Grid pair = make(4, 4, 4, 0, 0.0);
    pair.v[pair.at(1, 1, 1)] = 1; pair.v[pair.at(2, 2, 2)] = 1;
    for (int conn : { RTO_CONN_FACE, RTO_CONN_FULL }) {
        const rto_measure c = check_grid(cube, RTO_SET_SOLID, conn);
        CHECK(c.euler == 1 && c.voxels == 125 && c.faces[0] == 25 && c.faces[5] == 25);
        if (conn == RTO_CONN_FULL) CHECK(c.cells[0] == 216 && c.cells[1] == 540 && c.cells[2] == 450);
        else CHECK(c.cells[0] == 300 && c.cells[1] == 240 && c.cells[2] == 64);
        CHECK(check_grid(shell, RTO_SET_SOLID, conn).euler == 2);
        CHECK(check_grid(ring, RTO_SET_SOLID, conn).euler == 0);
        CHECK(check_grid(pair, RTO_SET_SOLID, conn).euler == (conn == RTO_CONN_FULL ? 1 : 2));
    }
    // the refusals
    std::vector<int32_t> labels;
    const Grid g = make(5, 4, 3, 7, 0.5);
    const int64_t count = label(g, 1, RTO_CONN_FACE, labels);
    std::vector<rto_measure> table;
    CHECK(measureComponentsCPU(5, 4, 3, labels.data(), count, 18, table, nullptr) == RTO_E_INVALID);
    CHECK(measureComponentsCPU(5, 4, 3, labels.data(), count - 1, RTO_CONN_FACE, table, nullptr) == RTO_E_INVALID && table.empty());
    CHECK(measureComponentsCPU(0, 4, 3, labels.data(), count, RTO_CONN_FACE, table, nullptr) == RTO_E_INVALID);
    CHECK(measureComponentsCPU(5, 4, 3, nullptr, count, RTO_CONN_FACE, table, nullptr) == RTO_E_INVALID);
    CHECK(measureComponentsCPU(32769, 1, 1, labels.data(), count, RTO_CONN_FACE, table, nullptr) == RTO_E_UNSUPPORTED);
    // the largest dimension: one row of 32768, sum of ii above 2^43
    std::vector<int32_t> row(32768, 0);
    rto_measure t;
    CHECK(measureComponentsCPU(32768, 1, 1, row.data(), 1, RTO_CONN_FULL, table, &t) == RTO_OK);
    CHECK(t.voxels == 32768 && t.sum[0] == 32767ll * 32768 / 2 && t.sum2[0] == 32767ll * 32768 * 65535 / 6 && t.euler == 1);
    if (g_fail) { std::fprintf(stderr, "measure selftest: %d checks failed\n", g_fail); return 1; }
    std::puts("measure selftest ok");
    return 0;
}
