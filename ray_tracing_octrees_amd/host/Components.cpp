#include "Components.h"

#include <algorithm>

int64_t labelComponentsCPU(const VoxelGrid& grid, int set, int connectivity, std::vector<int32_t>& labels,
                           std::vector<rto_component>& table) {
    labels.clear();
    table.clear();
    if (set != RTO_SET_SOLID && set != RTO_SET_EMPTY) return -1;
    if (connectivity != RTO_CONN_FACE && connectivity != RTO_CONN_FULL) return -1;
    const int dims[3] = { grid.dimX, grid.dimY, grid.dimZ };
    const int64_t n = (int64_t)dims[0] * dims[1] * dims[2];
    if (dims[0] < 0 || dims[1] < 0 || dims[2] < 0 || n > 0x7ffffffell || (int64_t)grid.data.size() < n) return -1;
    const VoxelState want = set == RTO_SET_SOLID ? VoxelState::FILLED : VoxelState::EMPTY;
    labels.assign((size_t)n, -1);
    std::vector<int32_t> queue;
    // seeds in ascending linear index: the seed of a component is its root, and components come out numbered by root
    for (int64_t seed = 0; seed < n; seed++) {
        if (grid.data[(size_t)seed] != want || labels[(size_t)seed] >= 0) continue;
        const int32_t id = (int32_t)table.size();
        rto_component c;
        c.root = seed; c.voxels = 0;
        for (int a = 0; a < 3; a++) { c.lo[a] = 0x7fffffff; c.hi[a] = -1; }
        c.touches = 0; c.reserved = 0;
        queue.clear();
        queue.push_back((int32_t)seed);
        labels[(size_t)seed] = id;
        for (size_t head = 0; head < queue.size(); head++) {
            const int32_t v = queue[head];
            const int p[3] = { v % dims[0], (v / dims[0]) % dims[1], v / (dims[0] * dims[1]) };
            c.voxels++;
            for (int a = 0; a < 3; a++) {
                c.lo[a] = std::min(c.lo[a], p[a]); c.hi[a] = std::max(c.hi[a], p[a]);
                if (p[a] == 0) c.touches |= 1 << a;
                if (p[a] == dims[a] - 1) c.touches |= 8 << a;
            }
            for (int dz = -1; dz <= 1; dz++)
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        const int changed = (dx != 0) + (dy != 0) + (dz != 0);
                        if (changed == 0 || (connectivity == RTO_CONN_FACE && changed != 1)) continue;
                        const int q[3] = { p[0] + dx, p[1] + dy, p[2] + dz };
                        if (q[0] < 0 || q[0] >= dims[0] || q[1] < 0 || q[1] >= dims[1] || q[2] < 0 || q[2] >= dims[2]) continue;
                        const size_t w = (size_t)q[0] + (size_t)dims[0] * ((size_t)q[1] + (size_t)dims[1] * (size_t)q[2]);
                        if (grid.data[w] != want || labels[w] >= 0) continue;
                        labels[w] = id;
                        queue.push_back((int32_t)w);
                    }
        }
        table.push_back(c);
    }
    return (int64_t)table.size();
}

int64_t applyComponentSelectionCPU(VoxelGrid& grid, int set, int connectivity, int select, int64_t arg) {
    if (select < RTO_SELECT_SMALLER_THAN || select > RTO_SELECT_NOT_CONTAINING) return -1;
    const int64_t n = (int64_t)grid.dimX * grid.dimY * grid.dimZ;
    const bool byVoxel = select == RTO_SELECT_CONTAINING || select == RTO_SELECT_NOT_CONTAINING;
    if ((byVoxel || select == RTO_SELECT_SMALLER_THAN) && arg < 0) return -1;
    if (byVoxel && arg >= n) return -1;
    std::vector<int32_t> labels;
    std::vector<rto_component> table;
    if (labelComponentsCPU(grid, set, connectivity, labels, table) < 0) return -1;
    if (table.empty()) return 0;
    std::vector<uint8_t> sel(table.size(), 0);
    size_t keep = 0;
    for (size_t i = 1; i < table.size(); i++)
        if (table[i].voxels > table[keep].voxels) keep = i;          // ascending root: the first of equals stays
    const int32_t at = byVoxel ? labels[(size_t)arg] : -1;
    for (size_t i = 0; i < table.size(); i++) {
        bool s = false;
        switch (select) {
            case RTO_SELECT_SMALLER_THAN: s = table[i].voxels < arg; break;
            case RTO_SELECT_ALL_BUT_LARGEST: s = i != keep; break;
            case RTO_SELECT_ENCLOSED: s = table[i].touches == 0; break;
            case RTO_SELECT_CONTAINING: s = at >= 0 && (int32_t)i == at; break;
            default: s = at >= 0 && (int32_t)i != at; break;
        }
        sel[i] = s ? 1 : 0;
    }
    const VoxelState to = set == RTO_SET_SOLID ? VoxelState::EMPTY : VoxelState::FILLED;
    int64_t changed = 0;
    for (int64_t v = 0; v < n; v++) {
        const int32_t l = labels[(size_t)v];
        if (l >= 0 && sel[(size_t)l]) { grid.data[(size_t)v] = to; changed++; }
    }
    return changed;
}
