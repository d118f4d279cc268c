#include "Measure.h"

#include <cstring>

namespace {

struct Volume {
    int dx, dy, dz;
    const int32_t* labels;
    bool in(int i, int j, int k) const {
        return i >= 0 && i < dx && j >= 0 && j < dy && k >= 0 && k < dz && labels[((size_t)k * dy + j) * dx + i] >= 0;
    }
};

// Is voxel (i, j, k) the incident set voxel with the smallest linear index of the cell given per axis by mode[a]: 0 the voxel's own
// extent on that axis (the incident voxels have offset 0 there), 1 the near end (offsets -1 and 0), 2 the far end (offsets 0, +1).
// Smaller linear index = smaller (k, j, i) in that order.
bool ownsCell(const Volume& v, int i, int j, int k, const int mode[3]) {
    int lo[3], hi[3];
    for (int a = 0; a < 3; a++) { lo[a] = mode[a] == 1 ? -1 : 0; hi[a] = mode[a] == 2 ? 1 : 0; }
    for (int c = lo[2]; c <= hi[2]; c++)
        for (int b = lo[1]; b <= hi[1]; b++)
            for (int a = lo[0]; a <= hi[0]; a++) {
                const bool before = c < 0 || (c == 0 && (b < 0 || (b == 0 && a < 0)));
                if (before && v.in(i + a, j + b, k + c)) return false;
            }
    return true;
}

// Are all voxels of the box [i, i + ex] x [j, j + ey] x [k, k + ez] in the set?
bool allSet(const Volume& v, int i, int j, int k, int ex, int ey, int ez) {
    for (int c = 0; c <= ez; c++)
        for (int b = 0; b <= ey; b++)
            for (int a = 0; a <= ex; a++)
                if (!v.in(i + a, j + b, k + c)) return false;
    return true;
}

}  // namespace

int measureComponentsCPU(int dimX, int dimY, int dimZ, const int32_t* labels, int64_t count, int connectivity,
                         std::vector<rto_measure>& out, rto_measure* total) {
    out.clear();
    if (connectivity != RTO_CONN_FACE && connectivity != RTO_CONN_FULL) return RTO_E_INVALID;
    if (dimX < 1 || dimY < 1 || dimZ < 1 || count < 0 || !labels) return RTO_E_INVALID;
    if (dimX > RTO_MEASURE_MAX_DIM || dimY > RTO_MEASURE_MAX_DIM || dimZ > RTO_MEASURE_MAX_DIM) return RTO_E_UNSUPPORTED;
    const size_t n = (size_t)dimX * dimY * dimZ;
    for (size_t v = 0; v < n; v++)
        if (labels[v] < -1 || labels[v] >= count) return RTO_E_INVALID;
    const bool full = connectivity == RTO_CONN_FULL;
    const Volume vol{ dimX, dimY, dimZ, labels };
    rto_measure zero;
    std::memset(&zero, 0, sizeof zero);
    out.assign((size_t)count, zero);
    static const int dirs[6][3] = { { -1, 0, 0 }, { 1, 0, 0 }, { 0, -1, 0 }, { 0, 1, 0 }, { 0, 0, -1 }, { 0, 0, 1 } };
    for (int k = 0; k < dimZ; k++)
        for (int j = 0; j < dimY; j++)
            for (int i = 0; i < dimX; i++) {
                const int32_t l = labels[((size_t)k * dimY + j) * dimX + i];
                if (l < 0) continue;
                rto_measure& m = out[(size_t)l];
                m.voxels++;
                for (int d = 0; d < 6; d++)
                    if (!vol.in(i + dirs[d][0], j + dirs[d][1], k + dirs[d][2])) m.faces[d]++;
                if (full) {
                    // the 26 cells of the voxel's cube: 8 vertices (three ends), 12 edges (two), 6 faces (one)
                    int mode[3];
                    for (mode[2] = 0; mode[2] < 3; mode[2]++)
                        for (mode[1] = 0; mode[1] < 3; mode[1]++)
                            for (mode[0] = 0; mode[0] < 3; mode[0]++) {
                                const int ends = (mode[0] != 0) + (mode[1] != 0) + (mode[2] != 0);
                                if (ends && ownsCell(vol, i, j, k, mode)) m.cells[3 - ends]++;
                            }
                } else {
                    for (int e = 1; e < 8; e++) {                  // the boxes with this voxel at their lowest corner
                        const int ex = e & 1, ey = (e >> 1) & 1, ez = e >> 2;
                        if (allSet(vol, i, j, k, ex, ey, ez)) m.cells[ex + ey + ez - 1]++;
                    }
                }
                m.sum[0] += i; m.sum[1] += j; m.sum[2] += k;
                m.sum2[0] += (int64_t)i * i; m.sum2[1] += (int64_t)j * j; m.sum2[2] += (int64_t)k * k;
                m.sum2[3] += (int64_t)i * j; m.sum2[4] += (int64_t)i * k; m.sum2[5] += (int64_t)j * k;
            }
    rto_measure sum = zero;
    for (rto_measure& m : out) {
        m.euler = full ? m.cells[0] - m.cells[1] + m.cells[2] - m.voxels : m.voxels - m.cells[0] + m.cells[1] - m.cells[2];
        const int64_t* w = reinterpret_cast<const int64_t*>(&m);
        int64_t* s = reinterpret_cast<int64_t*>(&sum);
        for (size_t f = 0; f < sizeof(rto_measure) / sizeof(int64_t); f++) s[f] += w[f];
    }
    if (total) *total = sum;
    return RTO_OK;
}
