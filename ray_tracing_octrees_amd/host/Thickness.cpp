#include "Thickness.h"

#include <algorithm>

int thicknessFieldCPU(const VoxelGrid& grid, int medium, int64_t mq, std::vector<int32_t>& t2, std::vector<int64_t>& bins,
                      rto_thick_summary* summary) {
    t2.clear();
    bins.clear();
    if (medium != RTO_SET_SOLID && medium != RTO_SET_EMPTY) return RTO_E_INVALID;
    if (mq < 0 || mq > 268435456ll) return RTO_E_INVALID;              // no cap (+inf) is c > 64 for the caller: it passes 2^28
    const int64_t c64 = mq * mq / 4096;
    if (c64 == 0) return RTO_E_INVALID;
    if (c64 > RTO_THICK_MAX_C) return RTO_E_UNSUPPORTED;
    const int c = (int)c64;
    // D: the transform to the other set, in reach of c; RTO_DIST_NONE (out of reach, or no other set) clips to c
    std::vector<int32_t> D;
    if (!distanceFieldCPU(grid, medium == RTO_SET_SOLID ? RTO_SET_EMPTY : RTO_SET_SOLID, mq, D, nullptr)) return RTO_E_UNSUPPORTED;
    const int dx = grid.dimX, dy = grid.dimY, dz = grid.dimZ;
    const size_t n = (size_t)dx * dy * dz;
    int32_t M = 0;
    for (size_t v = 0; v < n; v++) { D[v] = std::min<int32_t>(D[v], c); M = std::max(M, D[v]); }
    const int lim = std::min<int32_t>(c, M);                            // an offset with o^2 >= M is inside no ball
    int h = 0;
    while ((h + 1) * (h + 1) < lim) h++;                                // isqrt(lim - 1)
    t2 = D;                                                             // voxels that hold 0 or c keep them
    for (int z = 0; z < dz; z++)
        for (int y = 0; y < dy; y++)
            for (int x = 0; x < dx; x++) {
                const size_t p = ((size_t)z * dy + y) * dx + x;
                if (D[p] == 0 || D[p] == c) continue;
                int32_t best = D[p];
                for (int oz = std::max(-h, -z); oz <= std::min(h, dz - 1 - z) && best < M; oz++)
                    for (int oy = std::max(-h, -y); oy <= std::min(h, dy - 1 - y); oy++) {
                        const int32_t* row = D.data() + ((size_t)(z + oz) * dy + (y + oy)) * dx + x;
                        const int part = oz * oz + oy * oy;
                        for (int ox = std::max(-h, -x); ox <= std::min(h, dx - 1 - x); ox++)
                            if (row[ox] > part + ox * ox) best = std::max(best, row[ox]);
                    }
                t2[p] = best;
            }
    bins.assign((size_t)c + 1, 0);
    int64_t minT = -1, arg = -1;
    for (size_t v = 0; v < n; v++) {
        if (t2[v] == 0) continue;
        bins[(size_t)t2[v]]++;
        if (minT < 0 || t2[v] < minT) { minT = t2[v]; arg = (int64_t)v; }
    }
    if (summary) {
        summary->min_t2 = minT; summary->argmin = arg; summary->thin = 0; summary->medium = 0;
        for (int t = 0; t <= c; t++) { summary->medium += bins[(size_t)t]; if (t < c) summary->thin += bins[(size_t)t]; }
    }
    return RTO_OK;
}
