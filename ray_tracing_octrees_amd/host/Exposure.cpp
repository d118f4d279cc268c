#include "Exposure.h"

#include <algorithm>
#include <cstdlib>

namespace {

int gcd3(int a, int b, int c) {
    auto g = [](int x, int y) { while (y) { const int t = x % y; x = y; y = t; } return x; };
    return g(g(std::abs(a), std::abs(b)), std::abs(c));
}

int checkArgs(const VoxelGrid& grid, const int32_t* dirs, const int32_t* weights, int n, int mode, int reach, int64_t& W) {
    if (!dirs) return RTO_E_INVALID;
    if (n < 1 || n > RTO_EXPO_MAX_DIRS) return RTO_E_INVALID;
    for (int i = 0; i < n; i++) {
        const int32_t* d = dirs + 3 * (size_t)i;
        if (!d[0] && !d[1] && !d[2]) return RTO_E_INVALID;
        for (int a = 0; a < 3; a++)
            if (d[a] < -RTO_EXPO_MAX_COMP || d[a] > RTO_EXPO_MAX_COMP) return RTO_E_INVALID;
    }
    W = 0;
    for (int i = 0; i < n; i++) {
        const int64_t w = weights ? weights[i] : 1;
        if (w < 0) return RTO_E_INVALID;
        W += w;
    }
    if (W > 0x7fffffffll) return RTO_E_INVALID;
    if (mode != RTO_EXPO_ALL && mode != RTO_EXPO_SKIN) return RTO_E_INVALID;
    if (reach < 1) return RTO_E_INVALID;
    if (grid.dimX <= 0 || grid.dimY <= 0 || grid.dimZ <= 0) return RTO_E_UNSUPPORTED;
    const int64_t nvox = (int64_t)grid.dimX * grid.dimY * grid.dimZ;
    if (nvox > 0x7ffffffell || (int64_t)grid.data.size() < nvox) return RTO_E_UNSUPPORTED;
    return RTO_OK;
}

}  // namespace

// The planes of axis a are crossed at t = (2 m + 1) / (2 |d_a|), m = 0 .. |d_a| - 1: the next crossing of every axis is kept as the
// fraction (2 m + 1) / |d_a|, the smallest is found by cross-multiplication (products below 2^18), and every axis that ties moves.
bool exposureTemplate(const int32_t d[3], std::vector<int32_t>& offsets, int32_t prim[3]) {
    offsets.clear();
    for (int a = 0; a < 3; a++)
        if (d[a] < -RTO_EXPO_MAX_COMP || d[a] > RTO_EXPO_MAX_COMP) return false;
    const int g = gcd3(d[0], d[1], d[2]);
    if (!g) return false;
    int len[3], sign[3], m[3] = { 0, 0, 0 }, at[3] = { 0, 0, 0 };
    for (int a = 0; a < 3; a++) {
        prim[a] = d[a] / g;
        len[a] = std::abs(prim[a]);
        sign[a] = prim[a] < 0 ? -1 : 1;
    }
    while (m[0] < len[0] || m[1] < len[1] || m[2] < len[2]) {
        int first = -1;
        for (int a = 0; a < 3; a++)
            if (m[a] < len[a] && (first < 0 || (2 * m[a] + 1) * len[first] < (2 * m[first] + 1) * len[a])) first = a;
        const int num = 2 * m[first] + 1, den = len[first];
        for (int a = 0; a < 3; a++)
            if (m[a] < len[a] && (2 * m[a] + 1) * den == num * len[a]) { m[a]++; at[a] += sign[a]; }
        offsets.insert(offsets.end(), { at[0], at[1], at[2] });
    }
    return true;
}

int exposureFieldCPU(const VoxelGrid& grid, const int32_t* dirs, const int32_t* weights, int n, int mode, int reach, std::vector<int32_t>& e,
                     rto_expo_summary* summary, int64_t* steps) {
    e.clear();
    int64_t W = 0;
    const int rc = checkArgs(grid, dirs, weights, n, mode, reach, W);
    if (rc != RTO_OK) return rc;
    const int dx = grid.dimX, dy = grid.dimY, dz = grid.dimZ;
    const size_t nvox = (size_t)dx * dy * dz;
    struct Dir { std::vector<int32_t> off; int32_t prim[3]; int32_t w; };
    std::vector<Dir> T((size_t)n);
    for (int i = 0; i < n; i++) {
        exposureTemplate(dirs + 3 * (size_t)i, T[(size_t)i].off, T[(size_t)i].prim);
        T[(size_t)i].w = weights ? weights[i] : 1;
    }
    auto solid = [&](int x, int y, int z) { return grid.data[((size_t)z * dy + y) * dx + x] == VoxelState::FILLED; };
    e.assign(nvox, -1);
    int64_t evaluated = 0, total = 0, dark = 0, open = 0, marched = 0;
    for (int z = 0; z < dz; z++)
        for (int y = 0; y < dy; y++)
            for (int x = 0; x < dx; x++) {
                if (solid(x, y, z)) continue;
                if (mode == RTO_EXPO_SKIN &&
                    !((x > 0 && solid(x - 1, y, z)) || (x + 1 < dx && solid(x + 1, y, z)) || (y > 0 && solid(x, y - 1, z)) ||
                      (y + 1 < dy && solid(x, y + 1, z)) || (z > 0 && solid(x, y, z - 1)) || (z + 1 < dz && solid(x, y, z + 1))))
                    continue;
                int64_t sum = 0;
                for (const Dir& t : T) {
                    bool blocked = false, live = true;
                    const size_t entries = t.off.size() / 3;
                    for (int64_t bx = 0, by = 0, bz = 0; live; bx += t.prim[0], by += t.prim[1], bz += t.prim[2])
                        for (size_t j = 0; j < entries && live; j++) {
                            marched++;
                            // offsets from the voxel: at most the grid's size and one period, far inside 64 bits
                            const int64_t rx = bx + t.off[3 * j], ry = by + t.off[3 * j + 1], rz = bz + t.off[3 * j + 2];
                            const int64_t far = std::max(std::max(rx < 0 ? -rx : rx, ry < 0 ? -ry : ry), rz < 0 ? -rz : rz);
                            const int64_t qx = x + rx, qy = y + ry, qz = z + rz;
                            if (far > reach || qx < 0 || qx >= dx || qy < 0 || qy >= dy || qz < 0 || qz >= dz) live = false;
                            else if (solid((int)qx, (int)qy, (int)qz)) { blocked = true; live = false; }
                        }
                    if (!blocked) sum += t.w;
                }
                e[((size_t)z * dy + y) * dx + x] = (int32_t)sum;
                evaluated++;
                total += sum;
                dark += sum == 0;
                open += sum == W;
            }
    if (summary) { summary->evaluated = evaluated; summary->total = total; summary->dark = dark; summary->open = open; }
    if (steps) *steps = marched;
    return RTO_OK;
}
