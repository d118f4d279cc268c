#include "Geodesic.h"

#include <algorithm>

namespace {

int checkArgs(const VoxelGrid& grid, int medium, int connectivity, const int64_t* seeds, int64_t n, int64_t limit) {
    if (medium != RTO_SET_SOLID && medium != RTO_SET_EMPTY) return RTO_E_INVALID;
    if (connectivity != RTO_CONN_FACE && connectivity != RTO_CONN_FULL) return RTO_E_INVALID;
    if (n < 1 || !seeds || limit < 0) return RTO_E_INVALID;
    if (grid.dimX <= 0 || grid.dimY <= 0 || grid.dimZ <= 0) return RTO_E_UNSUPPORTED;
    const int64_t nvox = (int64_t)grid.dimX * grid.dimY * grid.dimZ;
    if (nvox > 0x7ffffffell || (int64_t)grid.data.size() < nvox) return RTO_E_UNSUPPORTED;
    const int64_t wmax = connectivity == RTO_CONN_FULL ? 5 : 1;
    if (wmax * (nvox - 1) >= 0x7fffffffll) return RTO_E_UNSUPPORTED;
    for (int64_t i = 0; i < n; i++)
        if (seeds[i] < 0 || seeds[i] >= nvox) return RTO_E_INVALID;
    return RTO_OK;
}

}  // namespace

int geodesicFieldCPU(const VoxelGrid& grid, int medium, int connectivity, const int64_t* seeds, int64_t n, int64_t limit,
                     std::vector<int32_t>& g, rto_geo_summary* summary) {
    g.clear();
    const int rc = checkArgs(grid, medium, connectivity, seeds, n, limit);
    if (rc != RTO_OK) return rc;
    const int dims[3] = { grid.dimX, grid.dimY, grid.dimZ };
    const size_t nvox = (size_t)dims[0] * dims[1] * dims[2];
    const VoxelState want = medium == RTO_SET_SOLID ? VoxelState::FILLED : VoxelState::EMPTY;
    const int64_t reach = std::min<int64_t>(limit, (int64_t)RTO_DIST_NONE - 1);
    const bool full = connectivity == RTO_CONN_FULL;
    g.assign(nvox, RTO_DIST_NONE);
    // bucket d % 6 holds voxels whose tentative value is d; a voxel is settled when it is popped with its current value
    std::vector<int32_t> bucket[6];
    for (int64_t i = 0; i < n; i++) {
        const size_t v = (size_t)seeds[i];
        if (grid.data[v] == want && g[v] != 0) { g[v] = 0; bucket[0].push_back((int32_t)v); }
    }
    int64_t pending = (int64_t)bucket[0].size();
    for (int64_t d = 0; pending > 0; d++) {
        std::vector<int32_t>& b = bucket[d % 6];
        for (size_t head = 0; head < b.size(); head++) {            // weights are positive: nothing is pushed into b while it drains
            const int32_t v = b[head];
            pending--;
            if ((int64_t)g[(size_t)v] != d) continue;               // lowered since it was pushed
            const int p[3] = { v % dims[0], (v / dims[0]) % dims[1], v / (dims[0] * dims[1]) };
            for (int dz = -1; dz <= 1; dz++)
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        const int changed = (dx != 0) + (dy != 0) + (dz != 0);
                        if (changed == 0 || (!full && changed != 1)) continue;
                        const int q[3] = { p[0] + dx, p[1] + dy, p[2] + dz };
                        if (q[0] < 0 || q[0] >= dims[0] || q[1] < 0 || q[1] >= dims[1] || q[2] < 0 || q[2] >= dims[2]) continue;
                        const size_t u = (size_t)q[0] + (size_t)dims[0] * ((size_t)q[1] + (size_t)dims[1] * (size_t)q[2]);
                        if (grid.data[u] != want) continue;
                        const int64_t nd = d + (full ? 2 + changed : 1);
                        if (nd > reach || nd >= (int64_t)g[u]) continue;
                        g[u] = (int32_t)nd;
                        bucket[nd % 6].push_back((int32_t)u);
                        pending++;
                    }
        }
        b.clear();
    }
    if (summary) {
        summary->max_g = -1; summary->argmax = -1; summary->reached = 0; summary->reserved = 0;
        for (size_t v = 0; v < nvox; v++) {
            if (g[v] == RTO_DIST_NONE) continue;
            summary->reached++;
            if ((int64_t)g[v] > summary->max_g) { summary->max_g = g[v]; summary->argmax = (int64_t)v; }
        }
    }
    return RTO_OK;
}

int geodesicPathsCPU(const VoxelGrid& grid, int connectivity, const std::vector<int32_t>& g, const int64_t* targets, int64_t n,
                     int64_t maxLen, int64_t* outVoxels, int64_t* outLen) {
    if (connectivity != RTO_CONN_FACE && connectivity != RTO_CONN_FULL) return RTO_E_INVALID;
    if (n < 1 || !targets || !outLen || maxLen < 0 || (maxLen > 0 && !outVoxels)) return RTO_E_INVALID;
    const int dims[3] = { grid.dimX, grid.dimY, grid.dimZ };
    const int64_t nvox = (int64_t)dims[0] * dims[1] * dims[2];
    if (nvox <= 0 || (int64_t)g.size() != nvox) return RTO_E_INVALID;
    for (int64_t i = 0; i < n; i++)
        if (targets[i] < 0 || targets[i] >= nvox) return RTO_E_INVALID;
    const bool full = connectivity == RTO_CONN_FULL;
    for (int64_t i = 0; i < n; i++) {
        int64_t* row = maxLen > 0 ? outVoxels + i * maxLen : nullptr;
        int64_t p = targets[i];
        int64_t len = 0;
        if (g[(size_t)p] == RTO_DIST_NONE) len = -1;
        else {
            for (;;) {
                if (len < maxLen) row[len] = p;
                len++;
                const int32_t gp = g[(size_t)p];
                if (gp == 0) break;
                const int c[3] = { (int)(p % dims[0]), (int)((p / dims[0]) % dims[1]), (int)(p / ((int64_t)dims[0] * dims[1])) };
                int64_t nextP = -1;
                for (int dz = -1; dz <= 1 && nextP < 0; dz++)          // ascending linear index: the first match is the smallest
                    for (int dy = -1; dy <= 1 && nextP < 0; dy++)
                        for (int dx = -1; dx <= 1 && nextP < 0; dx++) {
                            const int changed = (dx != 0) + (dy != 0) + (dz != 0);
                            if (changed == 0 || (!full && changed != 1)) continue;
                            const int q[3] = { c[0] + dx, c[1] + dy, c[2] + dz };
                            if (q[0] < 0 || q[0] >= dims[0] || q[1] < 0 || q[1] >= dims[1] || q[2] < 0 || q[2] >= dims[2]) continue;
                            const int64_t u = (int64_t)q[0] + (int64_t)dims[0] * ((int64_t)q[1] + (int64_t)dims[1] * q[2]);
                            const int32_t gu = g[(size_t)u];
                            if (gu != RTO_DIST_NONE && (int64_t)gu + (full ? 2 + changed : 1) == (int64_t)gp) nextP = u;
                        }
                if (nextP < 0) break;                                    // not a field of this grid
                p = nextP;
            }
        }
        for (int64_t k = std::max<int64_t>(len, 0); k < maxLen; k++) row[k] = -1;
        outLen[i] = len;
    }
    return RTO_OK;
}

int64_t floodGeodesicCPU(VoxelGrid& grid, int medium, int connectivity, const int64_t* seeds, int64_t n, int64_t limit) {
    std::vector<int32_t> g;
    const int rc = geodesicFieldCPU(grid, medium, connectivity, seeds, n, limit, g, nullptr);
    if (rc != RTO_OK) return rc;
    const VoxelState to = medium == RTO_SET_SOLID ? VoxelState::EMPTY : VoxelState::FILLED;
    int64_t changed = 0;
    for (size_t v = 0; v < g.size(); v++)
        if (g[v] != RTO_DIST_NONE) { grid.data[v] = to; changed++; }
    return changed;
}
