#include "Skeleton.h"

#include <algorithm>

namespace {

constexpr uint32_t bitsWhere(int axis, int value) {
    uint32_t m = 0;
    for (int b = 0; b < 27; b++) {
        const int d[3] = { b % 3 - 1, (b / 3) % 3 - 1, b / 9 - 1 };
        if (d[axis] == value) m |= 1u << b;
    }
    return m;
}
constexpr uint32_t bitsWithin(int lo, int hi) {       // the cells that differ from the centre on lo .. hi axes
    uint32_t m = 0;
    for (int b = 0; b < 27; b++) {
        const int c = (b % 3 != 1) + ((b / 3) % 3 != 1) + (b / 9 != 1);
        if (c >= lo && c <= hi) m |= 1u << b;
    }
    return m;
}
constexpr uint32_t kAll = (1u << 27) - 1u, kN26 = bitsWithin(1, 3), kN18 = bitsWithin(1, 2), kN6 = bitsWithin(1, 1);
constexpr uint32_t kX0 = bitsWhere(0, -1), kX2 = bitsWhere(0, 1), kY0 = bitsWhere(1, -1), kY2 = bitsWhere(1, 1);

// One step of growth along an axis inside the 3 x 3 x 3 block; every shift is masked back to the block's 27 bits.
inline uint32_t growX(uint32_t m) { return m | ((m << 1) & (kAll & ~kX0)) | ((m >> 1) & (kAll & ~kX2)); }
inline uint32_t growY(uint32_t m) { return m | ((m << 3) & (kAll & ~kY0)) | ((m >> 3) & (kAll & ~kY2)); }
inline uint32_t growZ(uint32_t m) { return m | ((m << 9) & kAll) | (m >> 9); }

// What of `inside` the lowest bit of `from` reaches: by 26 (the three growths composed) or by 6 (their union).
template <bool BY26> inline uint32_t flood(uint32_t from, uint32_t inside) {
    uint32_t f = from & (0u - from);
    for (;;) {
        const uint32_t g = (BY26 ? growZ(growY(growX(f))) : (growX(f) | growY(f) | growZ(f))) & inside;
        if (g == f) return f;
        f = g;
    }
}

inline bool simpleFull(uint32_t n) {
    n &= kN26;
    if (!n || flood<true>(n, n) != n) return false;
    const uint32_t b = ~n & kN18, b6 = b & kN6;
    return b6 && (flood<false>(b6, b) & b6) == b6;
}

int checkArgs(const VoxelGrid& grid, int set, int connectivity, int mode, const int64_t* anchors, int64_t n, int64_t maxPasses) {
    if (set != RTO_SET_SOLID && set != RTO_SET_EMPTY) return RTO_E_INVALID;
    if (connectivity != RTO_CONN_FACE && connectivity != RTO_CONN_FULL) return RTO_E_INVALID;
    if (mode != RTO_SKEL_TOPOLOGY && mode != RTO_SKEL_CURVE) return RTO_E_INVALID;
    if (mode == RTO_SKEL_CURVE && connectivity != RTO_CONN_FULL) return RTO_E_INVALID;
    if (n < 0 || (n > 0 && !anchors) || maxPasses < 1) return RTO_E_INVALID;
    if (grid.dimX <= 0 || grid.dimY <= 0 || grid.dimZ <= 0) return RTO_E_UNSUPPORTED;
    const int64_t nvox = (int64_t)grid.dimX * grid.dimY * grid.dimZ;
    if (nvox > 0x7ffffffell || (int64_t)grid.data.size() < nvox) return RTO_E_UNSUPPORTED;
    for (int64_t i = 0; i < n; i++)
        if (anchors[i] < 0 || anchors[i] >= nvox) return RTO_E_INVALID;
    return RTO_OK;
}

}  // namespace

bool skeletonSimpleCPU(uint32_t mask, int connectivity) { return simpleFull(connectivity == RTO_CONN_FULL ? mask : ~mask & kN26); }

int skeletonFieldCPU(const VoxelGrid& grid, int set, int connectivity, int mode, const int64_t* anchors, int64_t n, int64_t maxPasses,
                     std::vector<int32_t>& k, rto_skel_summary* summary) {
    k.clear();
    const int rc = checkArgs(grid, set, connectivity, mode, anchors, n, maxPasses);
    if (rc != RTO_OK) return rc;
    const int dx = grid.dimX, dy = grid.dimY, dz = grid.dimZ;
    const size_t nvox = (size_t)dx * dy * dz;
    const VoxelState want = set == RTO_SET_SOLID ? VoxelState::FILLED : VoxelState::EMPTY;
    const bool full = connectivity == RTO_CONN_FULL;
    // state[v]: bit 0 in X, bit 1 anchor, bit 2 in the list of marked voxels
    std::vector<uint8_t> state(nvox, 0);
    k.assign(nvox, -1);
    for (size_t v = 0; v < nvox; v++)
        if (grid.data[v] == want) { state[v] = 1; k[v] = 0; }
    for (int64_t i = 0; i < n; i++) state[(size_t)anchors[i]] |= 2;
    // the 27-bit block of v; beyond the grid is not in X
    auto blockOf = [&](int x, int y, int z) {
        uint32_t m = 0;
        if (x > 0 && x < dx - 1 && y > 0 && y < dy - 1 && z > 0 && z < dz - 1) {       // the whole block lies in the grid
            for (int r = 0; r < 9; r++) {
                const uint8_t* p = state.data() + ((size_t)(z + r / 3 - 1) * dy + (y + r % 3 - 1)) * dx + (x - 1);
                m |= (uint32_t)((p[0] & 1) | (p[1] & 1) << 1 | (p[2] & 1) << 2) << (3 * r);
            }
            return m;
        }
        for (int b = 0; b < 27; b++) {
            const int nx = x + b % 3 - 1, ny = y + (b / 3) % 3 - 1, nz = z + b / 9 - 1;
            if (nx < 0 || nx >= dx || ny < 0 || ny >= dy || nz < 0 || nz >= dz) continue;
            m |= (uint32_t)(state[((size_t)nz * dy + ny) * dx + nx] & 1) << b;
        }
        return m;
    };
    const uint32_t need = full ? kN6 : kN26;                        // a marked voxel lacks one of these neighbours
    // M of pass 1 by a scan; M of pass p + 1 is what pass p left of its M (a neighbour that is out stays out) and the voxels of X
    // beside a voxel that pass p removed
    std::vector<int32_t> marked, next, removed;
    for (int z = 0; z < dz; z++)
        for (int y = 0; y < dy; y++)
            for (int x = 0; x < dx; x++) {
                const size_t v = ((size_t)z * dy + y) * dx + x;
                if ((state[v] & 1) && (blockOf(x, y, z) & need) != need) { state[v] |= 4; marked.push_back((int32_t)v); }
            }
    int64_t passes = 0, gone = 0;
    std::vector<int32_t> sub[8];
    for (int64_t p = 1; p <= maxPasses && !marked.empty(); p++) {
        for (auto& s : sub) s.clear();
        for (const int32_t v : marked) {
            const int x = v % dx, y = (v / dx) % dy, z = v / (dx * dy);
            sub[(x & 1) + 2 * (y & 1) + 4 * (z & 1)].push_back(v);
        }
        removed.clear();
        next.clear();
        for (int s = 0; s < 8; s++)
            for (const int32_t v : sub[s]) {
                bool go = !(state[(size_t)v] & 2);
                if (go) {
                    const uint32_t m = blockOf(v % dx, (v / dx) % dy, v / (dx * dy)) & kN26;
                    if (mode == RTO_SKEL_CURVE && m && !(m & (m - 1))) go = false;
                    else go = simpleFull(full ? m : ~m & kN26);
                }
                if (go) { state[(size_t)v] = 0; k[(size_t)v] = (int32_t)p; removed.push_back(v); }
                else next.push_back(v);
            }
        if (removed.empty()) break;
        passes = p;
        gone += (int64_t)removed.size();
        for (const int32_t v : removed) {
            const int x = v % dx, y = (v / dx) % dy, z = v / (dx * dy);
            for (int b = 0; b < 27; b++) {
                if (!((need >> b) & 1u)) continue;
                const int nx = x + b % 3 - 1, ny = y + (b / 3) % 3 - 1, nz = z + b / 9 - 1;
                if (nx < 0 || nx >= dx || ny < 0 || ny >= dy || nz < 0 || nz >= dz) continue;
                const size_t u = ((size_t)nz * dy + ny) * dx + nx;
                if ((state[u] & 5) == 1) { state[u] |= 4; next.push_back((int32_t)u); }
            }
        }
        marked.swap(next);
    }
    if (summary) {
        int64_t in = 0;
        for (size_t v = 0; v < nvox; v++) in += k[v] >= 0;
        summary->kept = in - gone; summary->removed = gone; summary->passes = passes; summary->reserved = 0;
    }
    return RTO_OK;
}

int64_t thinCPU(VoxelGrid& grid, int set, int connectivity, int mode, const int64_t* anchors, int64_t n, int64_t maxPasses) {
    std::vector<int32_t> k;
    const int rc = skeletonFieldCPU(grid, set, connectivity, mode, anchors, n, maxPasses, k, nullptr);
    if (rc != RTO_OK) return rc;
    const VoxelState to = set == RTO_SET_SOLID ? VoxelState::EMPTY : VoxelState::FILLED;
    int64_t changed = 0;
    for (size_t v = 0; v < k.size(); v++)
        if (k[v] > 0) { grid.data[v] = to; changed++; }
    return changed;
}
