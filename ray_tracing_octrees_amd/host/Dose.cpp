#include "Dose.h"

#include <algorithm>
#include <cstdlib>

namespace {

int checkArgs(const VoxelGrid& grid, const int32_t* sources, int n, const uint32_t* transmit, int m, int falloff, int mode, int reach, int* badSource) {
    if (!sources) return RTO_E_INVALID;
    if (n < 1 || n > RTO_DOSE_MAX_SOURCES) return RTO_E_INVALID;
    int64_t W = 0;
    for (int i = 0; i < n; i++) {
        const int64_t w = sources[4 * (size_t)i + 3];
        if (w < 0) return RTO_E_INVALID;
        W += w;
    }
    if (W > 0x7fffffffll) return RTO_E_INVALID;
    if (transmit) {
        if (m < 1 || m > RTO_DOSE_MAX_TABLE) return RTO_E_INVALID;
        for (int i = 0; i < m; i++)
            if (transmit[i] > 65536u) return RTO_E_INVALID;
    }
    if (falloff != RTO_DOSE_FALLOFF_NONE && falloff != RTO_DOSE_FALLOFF_INVERSE_SQUARE) return RTO_E_INVALID;
    if (mode != RTO_DOSE_ALL && mode != RTO_DOSE_SKIN) return RTO_E_INVALID;
    if (reach < 1) return RTO_E_INVALID;
    if (grid.dimX <= 0 || grid.dimY <= 0 || grid.dimZ <= 0) return RTO_E_UNSUPPORTED;
    const int64_t nvox = (int64_t)grid.dimX * grid.dimY * grid.dimZ;
    if (nvox > 0x7ffffffell || (int64_t)grid.data.size() < nvox) return RTO_E_UNSUPPORTED;
    const int dims[3] = { grid.dimX, grid.dimY, grid.dimZ };
    for (int i = 0; i < n; i++)
        for (int a = 0; a < 3; a++)
            if (sources[4 * (size_t)i + a] < 0 || sources[4 * (size_t)i + a] >= dims[a]) {
                if (badSource) *badSource = i;
                return RTO_E_INVALID;
            }
    return RTO_OK;
}

// The walk of one pair: visit(x, y, z) for every crossed voxel in order, until it returns false or the segment arrives at s.  The
// planes of axis a are crossed at t = (2 m + 1) / (2 |d_a|): the next crossing of every axis is kept as the fraction
// (2 m + 1) / |d_a|, the smallest found by cross-multiplication (64-bit: any grid), and every axis that ties moves in the same step.
template <class Visit> void walk(const int32_t p[3], const int32_t s[3], Visit visit) {
    int64_t len[3], m[3] = { 0, 0, 0 };
    int32_t at[3], sign[3];
    for (int a = 0; a < 3; a++) {
        const int64_t d = (int64_t)s[a] - p[a];
        len[a] = d < 0 ? -d : d;
        sign[a] = d < 0 ? -1 : 1;
        at[a] = p[a];
    }
    for (;;) {
        int first = -1;
        for (int a = 0; a < 3; a++)
            if (m[a] < len[a] && (first < 0 || (2 * m[a] + 1) * len[first] < (2 * m[first] + 1) * len[a])) first = a;
        if (first < 0) return;                                          // p == s
        const int64_t num = 2 * m[first] + 1, den = len[first];
        for (int a = 0; a < 3; a++)
            if (m[a] < len[a] && (2 * m[a] + 1) * den == num * len[a]) { m[a]++; at[a] += sign[a]; }
        if (m[0] == len[0] && m[1] == len[1] && m[2] == len[2]) return; // arrived: s itself is not crossed
        if (!visit(at[0], at[1], at[2])) return;
    }
}

}  // namespace

void doseSegment(const int32_t p[3], const int32_t s[3], std::vector<int32_t>& crossed) {
    crossed.clear();
    walk(p, s, [&](int32_t x, int32_t y, int32_t z) { crossed.insert(crossed.end(), { x, y, z }); return true; });
}

int doseFieldCPU(const VoxelGrid& grid, const int32_t* sources, int n, const uint32_t* transmit, int m, int falloff, int mode, int reach,
                 std::vector<int32_t>& e, std::vector<int64_t>* covered, rto_dose_summary* summary, int64_t* steps, int* badSource) {
    e.clear();
    if (covered) covered->clear();
    const int rc = checkArgs(grid, sources, n, transmit, m, falloff, mode, reach, badSource);
    if (rc != RTO_OK) return rc;
    const uint32_t sight[1] = { 65536u };
    if (!transmit) { transmit = sight; m = 1; }
    int stop = m;                                                       // from here on every entry is zero; never below 1: k = 0 must be told from k >= 1
    while (stop > 1 && transmit[stop - 1] == 0u) stop--;
    const int r = std::min(reach, RTO_DOSE_MAX_REACH);
    const int dx = grid.dimX, dy = grid.dimY, dz = grid.dimZ;
    const size_t nvox = (size_t)dx * dy * dz;
    auto solid = [&](int x, int y, int z) { return grid.data[((size_t)z * dy + y) * dx + x] == VoxelState::FILLED; };
    e.assign(nvox, -1);
    std::vector<int64_t> cover((size_t)n, 0);
    int64_t evaluated = 0, total = 0, dark = 0, seen = 0, peak = -1, peakVoxel = -1, marched = 0;
    for (int z = 0; z < dz; z++)
        for (int y = 0; y < dy; y++)
            for (int x = 0; x < dx; x++) {
                if (solid(x, y, z)) continue;
                if (mode == RTO_DOSE_SKIN &&
                    !((x > 0 && solid(x - 1, y, z)) || (x + 1 < dx && solid(x + 1, y, z)) || (y > 0 && solid(x, y - 1, z)) ||
                      (y + 1 < dy && solid(x, y + 1, z)) || (z > 0 && solid(x, y, z - 1)) || (z + 1 < dz && solid(x, y, z + 1))))
                    continue;
                const int32_t p[3] = { x, y, z };
                int64_t sum = 0;
                bool sees = false;
                for (int i = 0; i < n; i++) {
                    const int32_t* s = sources + 4 * (size_t)i;
                    const int64_t ax = std::abs((int64_t)s[0] - x), ay = std::abs((int64_t)s[1] - y), az = std::abs((int64_t)s[2] - z);
                    if (std::max(ax, std::max(ay, az)) > r) continue;
                    int k = 0;
                    walk(p, s, [&](int32_t qx, int32_t qy, int32_t qz) {
                        marched++;
                        if (solid(qx, qy, qz)) k++;
                        return k < stop;
                    });
                    uint64_t c = ((uint64_t)s[3] * (uint64_t)(k < m ? transmit[k] : 0u)) >> 16;
                    if (falloff == RTO_DOSE_FALLOFF_INVERSE_SQUARE) c /= (uint64_t)std::max<int64_t>(1, ax * ax + ay * ay + az * az);
                    sum += (int64_t)c;
                    if (k == 0) { cover[(size_t)i]++; sees = true; }
                }
                const int64_t v = ((int64_t)z * dy + y) * dx + x;
                e[(size_t)v] = (int32_t)sum;
                evaluated++;
                total += sum;
                dark += sum == 0;
                seen += sees;
                if (sum > peak) { peak = sum; peakVoxel = v; }
            }
    if (summary) {
        summary->evaluated = evaluated; summary->total = total; summary->dark = dark; summary->seen = seen;
        summary->peak = peak; summary->peak_voxel = peakVoxel;
    }
    if (covered) *covered = cover;
    if (steps) *steps = marched;
    return RTO_OK;
}
