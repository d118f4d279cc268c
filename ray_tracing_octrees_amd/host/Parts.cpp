#include "Parts.h"

#include <algorithm>
#include <map>
#include <utility>

#include "Distance.h"

namespace {

struct BasinEdge { int32_t a, b; int64_t s, at, pairs; };

// Calls f(u) for every neighbour u of v under the connectivity that lies in the grid.
template <class F> void forNeighbours(const int dims[3], int connectivity, int64_t v, F f) {
    const int p[3] = { (int)(v % dims[0]), (int)((v / dims[0]) % dims[1]), (int)(v / ((int64_t)dims[0] * dims[1])) };
    for (int dz = -1; dz <= 1; dz++)
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                const int changed = (dx != 0) + (dy != 0) + (dz != 0);
                if (changed == 0 || (connectivity == RTO_CONN_FACE && changed != 1)) continue;
                const int q[3] = { p[0] + dx, p[1] + dy, p[2] + dz };
                if (q[0] < 0 || q[0] >= dims[0] || q[1] < 0 || q[1] >= dims[1] || q[2] < 0 || q[2] >= dims[2]) continue;
                f((int64_t)q[0] + (int64_t)dims[0] * ((int64_t)q[1] + (int64_t)dims[1] * (int64_t)q[2]));
            }
}

}  // namespace

int64_t segmentPartsCPU(const VoxelGrid& grid, int set, int connectivity, int ratio, std::vector<int32_t>& labels, std::vector<rto_part>& parts,
                        std::vector<rto_neck>& necks, rto_parts_summary* summary) {
    labels.clear();
    parts.clear();
    necks.clear();
    if (summary) *summary = rto_parts_summary{ 0, 0, 0, 0 };
    if (set != RTO_SET_SOLID && set != RTO_SET_EMPTY) return -1;
    if (connectivity != RTO_CONN_FACE && connectivity != RTO_CONN_FULL) return -1;
    if (ratio < 0 || ratio > RTO_PARTS_RATIO_MAX) return -1;
    const int dims[3] = { grid.dimX, grid.dimY, grid.dimZ };
    if (dims[0] < 0 || dims[1] < 0 || dims[2] < 0) return -1;
    const int64_t n = (int64_t)dims[0] * dims[1] * dims[2];
    if ((int64_t)grid.data.size() < n) return -1;
    // (1) the height: the transform of the other set, uncapped; it is 0 exactly off S
    std::vector<int32_t> h;
    if (!distanceFieldCPU(grid, set == RTO_SET_SOLID ? RTO_SET_EMPTY : RTO_SET_SOLID, -1, h, nullptr)) return -1;
    labels.assign((size_t)n, -1);
    // (2) ascent: the neighbour with the largest key (h, -v)
    std::vector<int64_t> up((size_t)n, -1);
    for (int64_t v = 0; v < n; v++) {
        if (h[(size_t)v] <= 0) continue;
        int64_t best = v;
        forNeighbours(dims, connectivity, v, [&](int64_t u) {
            if (h[(size_t)u] > h[(size_t)best] || (h[(size_t)u] == h[(size_t)best] && u < best)) best = u;
        });
        up[(size_t)v] = best;
    }
    // (3) every chain ends at its peak (walk, then point the whole walk at the end); peaks in index order number the basins
    std::vector<int64_t> walk;
    for (int64_t v = 0; v < n; v++) {
        if (up[(size_t)v] < 0) continue;
        walk.clear();
        int64_t u = v;
        while (up[(size_t)u] != u) { walk.push_back(u); u = up[(size_t)u]; }
        for (int64_t w : walk) up[(size_t)w] = u;
    }
    struct Basin { int64_t peak, first, voxels; int lo[3], hi[3]; };
    std::vector<Basin> basins;
    std::vector<int32_t> basinOf((size_t)n, -1);
    for (int64_t v = 0; v < n; v++)
        if (up[(size_t)v] == v) {
            basinOf[(size_t)v] = (int32_t)basins.size();
            basins.push_back(Basin{ v, -1, 0, { 0x7fffffff, 0x7fffffff, 0x7fffffff }, { -1, -1, -1 } });
        }
    for (int64_t v = 0; v < n; v++) {
        if (up[(size_t)v] < 0) continue;
        const int32_t b = basinOf[(size_t)up[(size_t)v]];
        basinOf[(size_t)v] = b;
        Basin& B = basins[(size_t)b];
        if (B.first < 0) B.first = v;
        B.voxels++;
        const int p[3] = { (int)(v % dims[0]), (int)((v / dims[0]) % dims[1]), (int)(v / ((int64_t)dims[0] * dims[1])) };
        for (int a = 0; a < 3; a++) { B.lo[a] = std::min(B.lo[a], p[a]); B.hi[a] = std::max(B.hi[a], p[a]); }
    }
    // (4) basin edges: every unordered pair once, from its smaller voxel
    std::map<std::pair<int32_t, int32_t>, BasinEdge> found;
    for (int64_t v = 0; v < n; v++) {
        const int32_t a = basinOf[(size_t)v];
        if (a < 0) continue;
        forNeighbours(dims, connectivity, v, [&](int64_t u) {
            const int32_t b = basinOf[(size_t)u];
            if (u < v || b < 0 || b == a) return;
            const int64_t s = std::min(h[(size_t)v], h[(size_t)u]);
            const std::pair<int32_t, int32_t> key(std::min(a, b), std::max(a, b));
            auto it = found.find(key);
            if (it == found.end()) found.emplace(key, BasinEdge{ key.first, key.second, s, v, 1 });
            else {
                BasinEdge& e = it->second;
                if (s > e.s || (s == e.s && v < e.at)) { e.s = s; e.at = v; }
                e.pairs++;
            }
        });
    }
    std::vector<BasinEdge> edges;
    edges.reserve(found.size());
    for (const auto& kv : found) edges.push_back(kv.second);
    std::stable_sort(edges.begin(), edges.end(), [](const BasinEdge& x, const BasinEdge& y) { return x.s > y.s; });      // the map's order is (A, B)
    // (5) merge
    const int nb = (int)basins.size();
    std::vector<int> top((size_t)nb), P((size_t)nb);
    for (int i = 0; i < nb; i++) { top[(size_t)i] = i; P[(size_t)i] = h[(size_t)basins[(size_t)i].peak]; }
    auto find = [&](int a) { while (top[(size_t)a] != a) { top[(size_t)a] = top[(size_t)top[(size_t)a]]; a = top[(size_t)a]; } return a; };
    const int64_t r2 = (int64_t)ratio * ratio;
    for (const BasinEdge& e : edges) {
        const int a = find(e.a), b = find(e.b);
        if (a == b) continue;
        if (1000000ll * e.s >= r2 * (int64_t)std::min(P[(size_t)a], P[(size_t)b])) { top[(size_t)b] = a; P[(size_t)a] = std::max(P[(size_t)a], P[(size_t)b]); }
    }
    // (6) parts in ascending order of their smallest voxel: the first voxel met of every cluster, in index order
    std::vector<int32_t> number((size_t)nb, -1);
    for (int64_t v = 0; v < n; v++) {
        const int32_t b = basinOf[(size_t)v];
        if (b < 0) continue;
        const int r = find(b);
        if (number[(size_t)r] < 0) {
            number[(size_t)r] = (int32_t)parts.size();
            rto_part p{};
            p.root = v;
            for (int a = 0; a < 3; a++) { p.lo[a] = 0x7fffffff; p.hi[a] = -1; }
            p.peak = -1;
            parts.push_back(p);
        }
        labels[(size_t)v] = number[(size_t)r];
    }
    for (int i = 0; i < nb; i++) {
        const Basin& B = basins[(size_t)i];
        rto_part& p = parts[(size_t)number[(size_t)find(i)]];
        p.voxels += B.voxels;
        for (int a = 0; a < 3; a++) {
            p.lo[a] = std::min(p.lo[a], B.lo[a]); p.hi[a] = std::max(p.hi[a], B.hi[a]);
            if (B.lo[a] == 0) p.touches |= 1 << a;
            if (B.hi[a] == dims[a] - 1) p.touches |= 8 << a;
        }
        p.basins++;
        const int32_t ph = h[(size_t)B.peak];
        if (p.peak < 0 || ph > p.peak_h || (ph == p.peak_h && B.peak < p.peak)) { p.peak = B.peak; p.peak_h = ph; }
    }
    // (7) necks
    std::map<std::pair<int32_t, int32_t>, rto_neck> between;
    int64_t pairs = 0;
    for (const BasinEdge& e : edges) {
        const int32_t a = number[(size_t)find(e.a)], b = number[(size_t)find(e.b)];
        if (a == b) continue;
        const std::pair<int32_t, int32_t> key(std::min(a, b), std::max(a, b));
        auto it = between.find(key);
        if (it == between.end()) between.emplace(key, rto_neck{ key.first, key.second, (int32_t)e.s, 0, e.at, e.pairs });
        else {
            rto_neck& k = it->second;
            if (e.s > k.h || (e.s == k.h && e.at < k.at)) { k.h = (int32_t)e.s; k.at = e.at; }
            k.pairs += e.pairs;
        }
        pairs += e.pairs;
    }
    for (const auto& kv : between) necks.push_back(kv.second);
    if (summary) *summary = rto_parts_summary{ (int64_t)parts.size(), nb, (int64_t)necks.size(), pairs };
    return (int64_t)parts.size();
}

int64_t splitAtNecksCPU(VoxelGrid& grid, int set, int connectivity, int ratio) {
    std::vector<int32_t> labels;
    std::vector<rto_part> parts;
    std::vector<rto_neck> necks;
    if (segmentPartsCPU(grid, set, connectivity, ratio, labels, parts, necks, nullptr) < 0) return -1;
    const int dims[3] = { grid.dimX, grid.dimY, grid.dimZ };
    const int64_t n = (int64_t)dims[0] * dims[1] * dims[2];
    const VoxelState to = set == RTO_SET_SOLID ? VoxelState::EMPTY : VoxelState::FILLED;
    int64_t changed = 0;
    for (int64_t v = 0; v < n; v++) {
        const int32_t l = labels[(size_t)v];
        if (l < 0) continue;
        bool hit = false;
        forNeighbours(dims, connectivity, v, [&](int64_t u) { hit = hit || labels[(size_t)u] > l; });
        if (hit) { grid.data[(size_t)v] = to; changed++; }
    }
    return changed;
}
