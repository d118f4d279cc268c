#include "Distance.h"

#include <algorithm>
#include <cmath>

bool quantizeDistanceCPU(float dist, float voxelSize, int64_t& mq) {
    if (std::isinf(dist) && dist > 0.0f) { mq = -1; return true; }
    const double a = (double)dist / (double)voxelSize;
    const double b = a * 64.0;
    const double f = std::floor(b + 0.5);
    if (!(f <= 268435456.0 && dist >= 0.0f)) return false;             // NaN fails both
    mq = (int64_t)f;
    return true;
}

namespace {

// One line of n values, `stride` apart: f[u] <- min over s of f[s] + (u - s)^2, the lower envelope of the parabolas (Meijster):
// parabola s[q] is the lowest from u = t[q] on.  RTO_DIST_NONE entries are never pushed.  val[] keeps f at the pushed positions so
// that the line can be rewritten in place.  The forward sweep pops at most what it pushed.
void envelopeLine(int32_t* f, int n, size_t stride, int64_t reach, std::vector<int32_t>& s, std::vector<int32_t>& t, std::vector<int32_t>& val) {
    int q = -1;
    for (int u = 0; u < n; u++) {
        const int32_t g = f[(size_t)u * stride];
        if (g == RTO_DIST_NONE) continue;
        while (q >= 0) {
            const int64_t a = (int64_t)(t[q] - s[q]) * (t[q] - s[q]) + val[q], b = (int64_t)(t[q] - u) * (t[q] - u) + g;
            if (a <= b) break;
            q--;
        }
        if (q < 0) { q = 0; s[0] = u; t[0] = 0; val[0] = g; }
        else {
            const int64_t num = (int64_t)u * u - (int64_t)s[q] * s[q] + (int64_t)g - (int64_t)val[q];     // >= 0: the quotient is at least t[q]
            const int64_t w = 1 + num / (int64_t)(2 * (u - s[q]));
            if (w < n) { q++; s[q] = u; t[q] = (int32_t)w; val[q] = g; }
        }
    }
    for (int u = n - 1; u >= 0; u--) {
        int32_t out = RTO_DIST_NONE;
        if (q >= 0) {
            const int64_t d = (int64_t)(u - s[q]) * (u - s[q]) + val[q];
            if (d <= reach) out = (int32_t)d;
            if (u == t[q]) q--;
        }
        f[(size_t)u * stride] = out;
    }
}

bool fieldFits(const VoxelGrid& grid) {
    const int64_t dims[3] = { grid.dimX, grid.dimY, grid.dimZ };
    if (dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0) return false;
    const int64_t n = dims[0] * dims[1] * dims[2];
    if (n > 0x7ffffffell || (int64_t)grid.data.size() < n) return false;
    int64_t diag = 0;
    for (int a = 0; a < 3; a++) diag += (dims[a] - 1) * (dims[a] - 1);
    return diag < 0x7fffffffll;
}

}  // namespace

bool distanceFieldCPU(const VoxelGrid& grid, int set, int64_t mq, std::vector<int32_t>& d2, rto_dist_summary* summary) {
    d2.clear();
    if (set != RTO_SET_SOLID && set != RTO_SET_EMPTY) return false;
    if (!fieldFits(grid)) return false;
    const int dx = grid.dimX, dy = grid.dimY, dz = grid.dimZ;
    const size_t n = (size_t)dx * dy * dz;
    const int64_t reach = mq < 0 ? (int64_t)RTO_DIST_NONE - 1 : std::min<int64_t>(mq * mq / 4096, (int64_t)RTO_DIST_NONE - 1);
    const VoxelState want = set == RTO_SET_SOLID ? VoxelState::FILLED : VoxelState::EMPTY;
    d2.assign(n, RTO_DIST_NONE);
    // x: the nearest voxel of the set to the left, then to the right
    for (size_t row = 0; row < (size_t)dy * dz; row++) {
        const VoxelState* v = grid.data.data() + row * dx;
        int32_t* f = d2.data() + row * dx;
        int last = -1;
        for (int x = 0; x < dx; x++) {
            if (v[x] == want) last = x;
            if (last >= 0) f[x] = (int32_t)((int64_t)(x - last) * (x - last));
        }
        last = -1;
        for (int x = dx - 1; x >= 0; x--) {
            if (v[x] == want) last = x;
            if (last >= 0) f[x] = std::min<int32_t>(f[x], (int32_t)((int64_t)(last - x) * (last - x)));
            if ((int64_t)f[x] > reach) f[x] = RTO_DIST_NONE;
        }
    }
    std::vector<int32_t> s((size_t)std::max(dy, dz)), t(s.size()), val(s.size());
    for (int z = 0; z < dz; z++)
        for (int x = 0; x < dx; x++) envelopeLine(d2.data() + (size_t)z * dx * dy + x, dy, (size_t)dx, reach, s, t, val);
    for (size_t c = 0; c < (size_t)dx * dy; c++) envelopeLine(d2.data() + c, dz, (size_t)dx * dy, reach, s, t, val);
    if (summary) {
        summary->max_d2 = -1; summary->argmax = -1; summary->finite = 0; summary->reserved = 0;
        for (size_t v = 0; v < n; v++) {
            if (d2[v] == RTO_DIST_NONE) continue;
            summary->finite++;
            if ((int64_t)d2[v] > summary->max_d2) { summary->max_d2 = d2[v]; summary->argmax = (int64_t)v; }
        }
    }
    return true;
}

int64_t applyMorphologyCPU(VoxelGrid& grid, int op, int64_t rq) {
    if (op < RTO_MORPH_DILATE || op > RTO_MORPH_CLOSE || rq < 0 || rq > 268435456ll) return -1;
    if (!fieldFits(grid)) return -1;
    if (rq == 0) return 0;
    const size_t n = (size_t)grid.dimX * grid.dimY * grid.dimZ;
    const std::vector<VoxelState> before(grid.data.begin(), grid.data.begin() + n);
    const int first = (op == RTO_MORPH_DILATE || op == RTO_MORPH_CLOSE) ? RTO_SET_SOLID : RTO_SET_EMPTY;
    const int steps = (op == RTO_MORPH_OPEN || op == RTO_MORPH_CLOSE) ? 2 : 1;
    std::vector<int32_t> d2;
    for (int step = 0; step < steps; step++) {
        const int set = step == 0 ? first : (first == RTO_SET_SOLID ? RTO_SET_EMPTY : RTO_SET_SOLID);
        if (!distanceFieldCPU(grid, set, rq, d2, nullptr)) { std::copy(before.begin(), before.end(), grid.data.begin()); return -1; }
        const VoxelState from = set == RTO_SET_SOLID ? VoxelState::EMPTY : VoxelState::FILLED;
        const VoxelState to = set == RTO_SET_SOLID ? VoxelState::FILLED : VoxelState::EMPTY;
        for (size_t v = 0; v < n; v++)
            if (d2[v] != RTO_DIST_NONE && grid.data[v] == from) grid.data[v] = to;
    }
    int64_t changed = 0;
    for (size_t v = 0; v < n; v++) changed += grid.data[v] != before[v];
    return changed;
}
