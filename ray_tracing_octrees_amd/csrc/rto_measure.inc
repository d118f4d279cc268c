// rto_measure.inc -- component measures (include/rto_hip.h, rto_measure_components): for every component of the resident labelling
// and for the whole set its exposed faces by direction, its cell counts and Euler number, and the first and second moments of its
// voxel indices.  Included at the end of rto_api.hip, after rto_components.inc, whose tile and whose CcDims it uses.
//
// Rule (DESIGN.md section 22).  In the set: label >= 0; beyond the grid: not in the set.  FULL counts the lattice vertices, edges
// and faces of the component's cubes, each at the incident set voxel with the smallest linear index; FACE counts the fully set
// pairs, 2 x 2 squares and 2 x 2 x 2 blocks at their lowest corner.
//
// k_measure: one workgroup per 32 x 8 x 8 tile.  Membership of the tile and a halo of one voxel (34 x 10 x 10) is staged in LDS
// as one 64-bit word per (y, z) row, from the label volume alone.  A thread owns 8 voxels of a tile row, as in k_cc_local, and
// works on all 8 at once: every per-voxel predicate (this face is exposed, this corner is mine) is one 8-bit mask made from the 9
// row words around it, and a count is a popcount.  A thread folds its x-runs while the label stays the same; what is left is
// reduced over the wave when the wave holds one label, then over the workgroup's waves in LDS, in tile-local coordinates that fit
// 32 bits; the 64-bit sums of global indices are made from them where they leave the workgroup.  What a workgroup has left for
// its first label, in a large component the whole tile, goes to the tile's slot with plain stores; k_measure_fold, the launch
// after, adds up the slots of consecutive tiles that hold one label, so that such a component costs one set of atomics per 256
// tiles.  Everything else goes straight to the table.  Every store to the table is a relaxed agent-scope 64-bit atomicAdd into a
// record that a memset zeroed before the launch, and nothing another workgroup wrote is read inside a launch: the kernel
// boundaries are the only synchronisation.  k_measure_total, the last launch, writes every record's Euler number and sums the
// records into the total row.

namespace rto {

constexpr int kMsRowsY = kCcTileY + 2, kMsRowsZ = kCcTileZ + 2;          // halo rows
constexpr int kMsRows = kMsRowsY * kMsRowsZ;                             // 100 row words
constexpr int kMsSegs = kCcTileX / kCcSeg;                               // 4 segments of 8 voxels per row
constexpr int kMsHaloRows = kMsRows - kCcTileY * kCcTileZ;               // 36 rows outside the tile
constexpr int kMsJobs = kMsHaloRows * kMsSegs + 2 * kMsRows;             // halo segments, then the two x-halo voxels of every row
constexpr int kMsWords = 20;                                             // rto_measure in 64-bit words
// rto_measure's words
constexpr int kMsVoxels = 0, kMsFaces = 1, kMsCells = 7, kMsEuler = 10, kMsSum = 11, kMsSum2 = 14;
// the 19 tile-local sums of a workgroup: voxels, faces[6], cells[3], then lx, ly, lz, lxlx, lyly, lzlz, lxly, lxlz, lylz
constexpr int kMsLocal = 19;
static_assert(sizeof(rto_measure) == kMsWords * 8, "rto_measure is 160 bytes");
static_assert(kBlock == kCcTileY * kCcTileZ * kMsSegs, "one thread per 8-voxel segment of the tile");
static_assert(kMsJobs <= 2 * kBlock, "two rounds of halo jobs");

// A row word: bit 8 + lx is voxel lx of the row, lx = -1 .. 32, so that the left halo is the top bit of byte 0, segment s is byte
// s + 1 and the right halo the low bit of byte 5: every byte has one writer.
__device__ __forceinline__ void ms_put(unsigned long long* rows, int row, int byte, unsigned value) {
    reinterpret_cast<uint8_t*>(rows)[row * 8 + byte] = (uint8_t)value;
}

// The labels of 8 consecutive voxels of one row (-1 beyond the grid) and the mask of those in the set.  WIDE: dimX % 16 == 0, so
// the 8 lie inside the row or beyond it together and start on 32 bytes.
template <bool WIDE>
__device__ __forceinline__ unsigned ms_load8(const int* __restrict__ labels, const CcDims& D, int gx0, int gy, int gz, int (&ls)[kCcSeg]) {
#pragma unroll
    for (int j = 0; j < kCcSeg; j++) ls[j] = -1;
    if (gy < 0 || gy >= D.y || gz < 0 || gz >= D.z || gx0 >= D.x) return 0u;
    const size_t base = ((size_t)gz * D.y + gy) * (size_t)D.x + (size_t)gx0;
    if (WIDE) {
        const int4 a = *reinterpret_cast<const int4*>(labels + base), b = *reinterpret_cast<const int4*>(labels + base + 4);
        ls[0] = a.x; ls[1] = a.y; ls[2] = a.z; ls[3] = a.w; ls[4] = b.x; ls[5] = b.y; ls[6] = b.z; ls[7] = b.w;
    } else {
#pragma unroll
        for (int j = 0; j < kCcSeg; j++)
            if (gx0 + j < D.x) ls[j] = labels[base + j];
    }
    unsigned in = 0u;
#pragma unroll
    for (int j = 0; j < kCcSeg; j++) in |= (ls[j] >= 0 ? 1u : 0u) << j;
    return in;
}

// R[dz + 1][dy + 1]: bits 0 .. 9 are the voxels lx0 - 1 .. lx0 + 8 of the row at (dy, dz) from the thread's.  Bit j of ms_nb is
// the neighbour at (dx, dy, dz) of the thread's voxel j (bits above 7 are rubbish: the callers mask).
__device__ __forceinline__ unsigned ms_nb(const unsigned (&R)[3][3], int dx, int dy, int dz) { return R[dz + 1][dy + 1] >> (1 + dx); }

// The neighbours in the box [lox, hix] x [loy, hiy] x [loz, hiz] of offsets that precede the voxel in linear index, OR-ed: a
// cell whose incident voxels are that box is the voxel's own when none of them is in the set.  All arguments are constants.
__device__ __forceinline__ unsigned ms_before(const unsigned (&R)[3][3], int lox, int hix, int loy, int hiy, int loz, int hiz) {
    unsigned m = 0u;
#pragma unroll
    for (int dz = -1; dz <= 1; dz++)
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const bool inBox = dx >= lox && dx <= hix && dy >= loy && dy <= hiy && dz >= loz && dz <= hiz;
                const bool before = dz < 0 || (dz == 0 && (dy < 0 || (dy == 0 && dx < 0)));
                if (inBox && before) m |= ms_nb(R, dx, dy, dz);
            }
    return m;
}
// The neighbours in the box [0, hix] x [0, hiy] x [0, hiz], AND-ed: a pair, square or block with the voxel at its lowest corner.
__device__ __forceinline__ unsigned ms_all(const unsigned (&R)[3][3], int hix, int hiy, int hiz) {
    unsigned m = 0xffu;
#pragma unroll
    for (int dz = 0; dz <= 1; dz++)
#pragma unroll
        for (int dy = 0; dy <= 1; dy++)
#pragma unroll
            for (int dx = 0; dx <= 1; dx++)
                if (dx <= hix && dy <= hiy && dz <= hiz) m &= ms_nb(R, dx, dy, dz);
    return m;
}

// What a thread carries: one label, and of its voxels the count, the sums of lx and lx lx (ly and lz are the thread's own), the
// exposed faces and the cells.
struct MsAcc { int label; unsigned n, sx, sxx, f[6], c[3]; };

__device__ __forceinline__ void ms_add(unsigned long long* p, unsigned long long v) {
    if (v) atomicAdd(p, v);
}

// Tile-local sums e[] of one label, taken over voxels of the tile at (x0, y0, z0), as the words of a record (g[kMsEuler] = 0).
__device__ __forceinline__ void ms_global(const unsigned (&e)[kMsLocal], int x0, int y0, int z0, unsigned long long (&g)[kMsWords]) {
    const unsigned long long n = e[0], X = (unsigned long long)x0, Y = (unsigned long long)y0, Z = (unsigned long long)z0;
    const unsigned long long sx = e[10], sy = e[11], sz = e[12];
    g[kMsVoxels] = n;
#pragma unroll
    for (int k = 0; k < 9; k++) g[kMsFaces + k] = e[1 + k];              // faces[6], cells[3]
    g[kMsEuler] = 0ull;
    g[kMsSum + 0] = n * X + sx;
    g[kMsSum + 1] = n * Y + sy;
    g[kMsSum + 2] = n * Z + sz;
    g[kMsSum2 + 0] = n * X * X + 2ull * X * sx + e[13];
    g[kMsSum2 + 1] = n * Y * Y + 2ull * Y * sy + e[14];
    g[kMsSum2 + 2] = n * Z * Z + 2ull * Z * sz + e[15];
    g[kMsSum2 + 3] = n * X * Y + X * sy + Y * sx + e[16];
    g[kMsSum2 + 4] = n * X * Z + X * sz + Z * sx + e[17];
    g[kMsSum2 + 5] = n * Y * Z + Y * sz + Z * sy + e[18];
}
// The words of g into the label's record; words that are zero send nothing.
__device__ __forceinline__ void ms_send_words(rto_measure* __restrict__ recs, int label, const unsigned long long (&g)[kMsWords]) {
    unsigned long long* r = reinterpret_cast<unsigned long long*>(recs + label);
#pragma unroll
    for (int k = 0; k < kMsWords; k++)
        if (k != kMsEuler) ms_add(r + k, g[k]);
}
__device__ __forceinline__ void ms_send(rto_measure* __restrict__ recs, int label, const unsigned (&e)[kMsLocal], int x0, int y0, int z0) {
    unsigned long long g[kMsWords];
    ms_global(e, x0, y0, z0, g);
    ms_send_words(recs, label, g);
}

// A thread's accumulator as tile-local sums.  FULL: a voxel's three far faces are always its own, a near face when the neighbour
// behind it is not in the set: n2 = 3 voxels + faces[-x] + faces[-y] + faces[-z].
template <bool FULL>
__device__ __forceinline__ void ms_expand(const MsAcc& a, int ly, int lz, unsigned (&e)[kMsLocal]) {
    e[0] = a.n;
#pragma unroll
    for (int d = 0; d < 6; d++) e[1 + d] = a.f[d];
    e[7] = a.c[0]; e[8] = a.c[1];
    e[9] = FULL ? 3u * a.n + a.f[0] + a.f[2] + a.f[4] : a.c[2];
    e[10] = a.sx; e[11] = a.n * (unsigned)ly; e[12] = a.n * (unsigned)lz;
    e[13] = a.sxx; e[14] = a.n * (unsigned)(ly * ly); e[15] = a.n * (unsigned)(lz * lz);
    e[16] = a.sx * (unsigned)ly; e[17] = a.sx * (unsigned)lz; e[18] = a.n * (unsigned)(ly * lz);
}

template <bool WIDE, bool FULL>
__global__ __launch_bounds__(kBlock) void k_measure(const int* __restrict__ labels, CcDims D, int tilesX, int tilesY, rto_measure* __restrict__ recs,
                                                   rto_measure* __restrict__ slots) {
    __shared__ unsigned long long rows[kMsRows];
    __shared__ int waveLabel[kBlock / kWave];
    __shared__ unsigned waveSums[kBlock / kWave][kMsLocal];
    const int t = (int)threadIdx.x;
    const int bid = (int)blockIdx.x;
    const int x0 = (bid % tilesX) * kCcTileX, y0 = ((bid / tilesX) % tilesY) * kCcTileY, z0 = (bid / (tilesX * tilesY)) * kCcTileZ;
    const int row = t / kMsSegs, seg = t % kMsSegs;
    const int lx0 = seg * kCcSeg, ly = row % kCcTileY, lz = row / kCcTileY;
    // the tile: the thread's own 8 labels stay in registers
    int ls[kCcSeg];
    const unsigned in = ms_load8<WIDE>(labels, D, x0 + lx0, y0 + ly, z0 + lz, ls);
    ms_put(rows, (lz + 1) * kMsRowsY + (ly + 1), seg + 1, in);
    // the halo: 36 rows of 4 segments, then the voxels at lx = -1 and lx = 32 of all 100 rows
#pragma unroll
    for (int round = 0; round < 2; round++) {
        const int q = t + round * kBlock;
        if (q < kMsHaloRows * kMsSegs) {
            const int hr = q / kMsSegs, hseg = q % kMsSegs;
            int hy, hz;                                             // rows 0 .. 9: hz = 0; 10 .. 19: hz = 9; then hy = 0 or 9 of hz = 1 .. 8
            if (hr < kMsRowsY) { hy = hr; hz = 0; }
            else if (hr < 2 * kMsRowsY) { hy = hr - kMsRowsY; hz = kMsRowsZ - 1; }
            else { hy = ((hr - 2 * kMsRowsY) & 1) ? kMsRowsY - 1 : 0; hz = 1 + (hr - 2 * kMsRowsY) / 2; }
            int unused[kCcSeg];
            const unsigned m = ms_load8<WIDE>(labels, D, x0 + hseg * kCcSeg, y0 + hy - 1, z0 + hz - 1, unused);
            ms_put(rows, hz * kMsRowsY + hy, hseg + 1, m);
        } else if (q < kMsJobs) {
            const int cell = q - kMsHaloRows * kMsSegs;
            const int hrow = cell >> 1, right = cell & 1;
            const int gx = right ? x0 + kCcTileX : x0 - 1, gy = y0 + hrow % kMsRowsY - 1, gz = z0 + hrow / kMsRowsY - 1;
            unsigned m = 0u;
            if (gx >= 0 && gx < D.x && gy >= 0 && gy < D.y && gz >= 0 && gz < D.z)
                m = labels[((size_t)gz * D.y + gy) * (size_t)D.x + (size_t)gx] >= 0 ? 1u : 0u;
            ms_put(rows, hrow, right ? 5 : 0, right ? m : m << 7);
        }
    }
    __syncthreads();

    MsAcc a;
    a.label = -1; a.n = a.sx = a.sxx = 0u;
#pragma unroll
    for (int d = 0; d < 6; d++) a.f[d] = 0u;
    a.c[0] = a.c[1] = a.c[2] = 0u;
    if (in) {
        unsigned R[3][3];
#pragma unroll
        for (int dz = 0; dz < 3; dz++)
#pragma unroll
            for (int dy = 0; dy < 3; dy++) R[dz][dy] = (unsigned)(rows[(lz + dz) * kMsRowsY + (ly + dy)] >> (8 * seg + 7)) & 0x3ffu;
        // exposed faces, one byte per direction
        const unsigned fw0 = (in & ~ms_nb(R, -1, 0, 0)) | (in & ~ms_nb(R, 1, 0, 0)) << 8 | (in & ~ms_nb(R, 0, -1, 0)) << 16 | (in & ~ms_nb(R, 0, 1, 0)) << 24;
        const unsigned fw1 = (in & ~ms_nb(R, 0, 0, -1)) | (in & ~ms_nb(R, 0, 0, 1)) << 8;
        // cells, one byte per cell of the voxel: cw0 and cw1 count into cells[0], cw2 .. cw4 into cells[1], cw5 into cells[2]
        unsigned cw[6] = { 0u, 0u, 0u, 0u, 0u, 0u };
        if (FULL) {
#pragma unroll
            for (int k = 0; k < 8; k++) {                                // the vertex at corner (cx, cy, cz)
                const int cx = k & 1, cy = (k >> 1) & 1, cz = k >> 2;
                cw[k >> 2] |= (in & ~ms_before(R, cx - 1, cx, cy - 1, cy, cz - 1, cz)) << (8 * (k & 3));
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {                                // the edges along x, y and z at corner (p, q) of the other two axes
                const int p = k & 1, q = k >> 1;
                cw[2] |= (in & ~ms_before(R, 0, 0, p - 1, p, q - 1, q)) << (8 * k);
                cw[3] |= (in & ~ms_before(R, p - 1, p, 0, 0, q - 1, q)) << (8 * k);
                cw[4] |= (in & ~ms_before(R, p - 1, p, q - 1, q, 0, 0)) << (8 * k);
            }
        } else {
            cw[0] = (in & ms_all(R, 1, 0, 0)) | (in & ms_all(R, 0, 1, 0)) << 8 | (in & ms_all(R, 0, 0, 1)) << 16;       // pairs
            cw[2] = (in & ms_all(R, 1, 1, 0)) | (in & ms_all(R, 1, 0, 1)) << 8 | (in & ms_all(R, 0, 1, 1)) << 16;       // squares
            cw[5] = in & ms_all(R, 1, 1, 1);                                                                            // the block
        }
        unsigned m = in;
        while (m) {                                                      // the runs of set voxels, lowest first: one label each
            const int first = __ffs((int)m) - 1;
            const unsigned next = m + (1u << first);
            const unsigned run = m & ~next;
            m &= next;
            int l = ls[0];
#pragma unroll
            for (int j = 1; j < kCcSeg; j++) l = first == j ? ls[j] : l;
            if (l != a.label) {
                if (a.label >= 0) {
                    unsigned e[kMsLocal];
                    ms_expand<FULL>(a, ly, lz, e);
                    ms_send(recs, a.label, e, x0, y0, z0);
                }
                a.label = l; a.n = a.sx = a.sxx = 0u;
#pragma unroll
                for (int d = 0; d < 6; d++) a.f[d] = 0u;
                a.c[0] = a.c[1] = a.c[2] = 0u;
            }
            const int n = __popc(run), lo = lx0 + first - 1, hi = lx0 + first + n - 1;       // lx = lo + 1 .. hi
            a.n += (unsigned)n;
            a.sx += (unsigned)(hi * (hi + 1) / 2 - lo * (lo + 1) / 2);
            a.sxx += (unsigned)(hi * (hi + 1) * (2 * hi + 1) / 6 - lo * (lo + 1) * (2 * lo + 1) / 6);
            const unsigned r4 = run * 0x01010101u;
#pragma unroll
            for (int d = 0; d < 4; d++) a.f[d] += (unsigned)__popc(fw0 & (run << (8 * d)));
            a.f[4] += (unsigned)__popc(fw1 & run); a.f[5] += (unsigned)__popc(fw1 & (run << 8));
            a.c[0] += (unsigned)(__popc(cw[0] & r4) + __popc(cw[1] & r4));
            a.c[1] += (unsigned)(__popc(cw[2] & r4) + __popc(cw[3] & r4) + __popc(cw[4] & r4));
            a.c[2] += (unsigned)__popc(cw[5] & r4);
        }
    }
    // the wave: one label among the lanes that hold any -> one set of sums
    const int lane = t % kWave, wave = t / kWave;
    const bool have = a.label >= 0;
    int first;
    const bool uniform = wave_uniform_label(have, a.label, first);
    unsigned e[kMsLocal];
    ms_expand<FULL>(a, ly, lz, e);                                       // all zero in a lane that holds nothing
    if (uniform) {
#pragma unroll
        for (int k = 0; k < kMsLocal; k++) {
            const unsigned v = wave_sum(e[k]);
            if (lane == 0) waveSums[wave][k] = v;
        }
        if (lane == 0) waveLabel[wave] = first;
    } else {
        if (have) ms_send(recs, a.label, e, x0, y0, z0);
        if (lane == 0) waveLabel[wave] = -1;
    }
    __syncthreads();
    // the workgroup: waves that hold the same label go together.  The first such group, in a large component the whole tile, goes
    // to the tile's slot with plain stores (slot word kMsEuler = label + 1, 0: nothing) for k_measure_fold to add up; a further
    // group goes to its record
    if (t == 0) {
        unsigned long long* slot = reinterpret_cast<unsigned long long*>(slots + bid);
        bool slotUsed = false;
        for (int w = 0; w < kBlock / kWave; w++) {
            const int l = waveLabel[w];
            if (l < 0) continue;
            unsigned s[kMsLocal];
            for (int k = 0; k < kMsLocal; k++) s[k] = waveSums[w][k];
            for (int u = w + 1; u < kBlock / kWave; u++) {
                if (waveLabel[u] != l) continue;
                for (int k = 0; k < kMsLocal; k++) s[k] += waveSums[u][k];
                waveLabel[u] = -1;
            }
            unsigned long long g[kMsWords];
            ms_global(s, x0, y0, z0, g);
            if (!slotUsed) {
                g[kMsEuler] = (unsigned long long)l + 1ull;
#pragma unroll
                for (int k = 0; k < kMsWords; k++) slot[k] = g[k];
                slotUsed = true;
            } else {
                ms_send_words(recs, l, g);
            }
        }
        if (!slotUsed) slot[kMsEuler] = 0ull;
    }
}

// One thread per tile slot of the launch before: the slots of a large component, which holds runs of consecutive tiles, are added
// up over the wave when the wave holds one label and over the workgroup's waves in LDS, so that such a component costs one set of
// atomics per 256 tiles; a slot that shares its wave with another label goes to its record as it is.
__global__ __launch_bounds__(kBlock) void k_measure_fold(const rto_measure* __restrict__ slots, unsigned tiles, rto_measure* __restrict__ recs) {
    __shared__ int waveLabel[kBlock / kWave];
    __shared__ unsigned long long waveSums[kBlock / kWave][kMsWords];
    const unsigned i = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    unsigned long long g[kMsWords];
#pragma unroll
    for (int k = 0; k < kMsWords; k++) g[k] = 0ull;
    if (i < tiles) {
        const unsigned long long* slot = reinterpret_cast<const unsigned long long*>(slots + i);
        g[kMsEuler] = slot[kMsEuler];
        if (g[kMsEuler]) {
#pragma unroll
            for (int k = 0; k < kMsWords; k++)
                if (k != kMsEuler) g[k] = slot[k];
        }
    }
    const int label = (int)g[kMsEuler] - 1;
    g[kMsEuler] = 0ull;
    const int lane = (int)threadIdx.x % kWave, wave = (int)threadIdx.x / kWave;
    const bool have = label >= 0;
    int first;
    const bool uniform = wave_uniform_label(have, label, first);
    if (uniform) {
#pragma unroll
        for (int k = 0; k < kMsWords; k++) {
            const unsigned long long v = wave_sum(g[k]);
            if (lane == 0) waveSums[wave][k] = v;
        }
        if (lane == 0) waveLabel[wave] = first;
    } else {
        if (have) ms_send_words(recs, label, g);
        if (lane == 0) waveLabel[wave] = -1;
    }
    __syncthreads();
    if ((int)threadIdx.x < kMsWords) {                                   // thread k: word k of every group of waves with one label
        const int k = (int)threadIdx.x;
        for (int w = 0; w < kBlock / kWave; w++) {
            const int l = waveLabel[w];
            if (l < 0) continue;
            bool firstOfLabel = true;
            for (int u = 0; u < w; u++) firstOfLabel = firstOfLabel && waveLabel[u] != l;
            if (!firstOfLabel) continue;
            unsigned long long v = 0ull;
            for (int u = w; u < kBlock / kWave; u++)
                if (waveLabel[u] == l) v += waveSums[u][k];
            ms_add(reinterpret_cast<unsigned long long*>(recs + l) + k, v);
        }
    }
}

// Writes every record's Euler number and adds the records into recs[count], the total row (zero before the launch).  A thread
// strides over the records; a workgroup sends one set of atomics.
__global__ __launch_bounds__(kBlock) void k_measure_total(rto_measure* __restrict__ recs, unsigned count, int full) {
    __shared__ long long waveSums[kBlock / kWave][kMsWords];
    long long s[kMsWords];
#pragma unroll
    for (int k = 0; k < kMsWords; k++) s[k] = 0;
    for (unsigned i = blockIdx.x * (unsigned)kBlock + threadIdx.x; i < count; i += gridDim.x * (unsigned)kBlock) {
        long long* r = reinterpret_cast<long long*>(recs + i);
        long long w[kMsWords];
#pragma unroll
        for (int k = 0; k < kMsWords; k++) w[k] = r[k];
        w[kMsEuler] = full ? w[kMsCells] - w[kMsCells + 1] + w[kMsCells + 2] - w[kMsVoxels] : w[kMsVoxels] - w[kMsCells] + w[kMsCells + 1] - w[kMsCells + 2];
        r[kMsEuler] = w[kMsEuler];
#pragma unroll
        for (int k = 0; k < kMsWords; k++) s[k] += w[k];
    }
    const int lane = (int)threadIdx.x % kWave, wave = (int)threadIdx.x / kWave;
#pragma unroll
    for (int k = 0; k < kMsWords; k++) {
        long long v = s[k];
        for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) waveSums[wave][k] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < kMsWords) {
        long long v = 0;
        for (int w = 0; w < kBlock / kWave; w++) v += waveSums[w][threadIdx.x];
        ms_add(reinterpret_cast<unsigned long long*>(recs + count) + threadIdx.x, (unsigned long long)v);
    }
}

}  // namespace rto

extern "C" {

int rto_measure_components(rto_context* c, rto_measure* total) {
    using namespace rto;
    if (!c) return RTO_E_INVALID;
    if (!c->d_ccLabels) return fail(c, RTO_E_INVALID, "rto_measure_components: no labels are resident (not labelled yet, or the grid has changed since)");
    for (int a = 0; a < 3; a++)
        if (c->voxDim[a] > RTO_MEASURE_MAX_DIM) return fail(c, RTO_E_UNSUPPORTED, "rto_measure_components: a dimension of the grid is above 32768");
    const CcDims D{ c->voxDim[0], c->voxDim[1], c->voxDim[2], (unsigned)grid_voxels(c) };
    const unsigned count = (unsigned)c->ccCount;
    RTO_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    RTO_HIP(c, hipStreamSynchronize(s));
    StreamEvents<3> events;
    RTO_HIP(c, events.create());
    struct Table { rto_measure* d = nullptr; ~Table() { (void)hipFree(d); } } table;       // count records, then the total row
    RTO_HIP(c, hipMalloc(&table.d, ((size_t)count + 1) * sizeof(rto_measure)));
    RTO_HIP(c, events.record(0, s));
    RTO_HIP(c, hipMemsetAsync(table.d, 0, ((size_t)count + 1) * sizeof(rto_measure), s));
    BuildScratch scratch(s);
    if (count) {
        const CcTiles T(c->voxDim);
        const unsigned tiles = (unsigned)T.count();
        rto_measure* d_slots = nullptr;                                 // one per tile; every workgroup writes its own
        RTO_HIP(c, scratch.alloc(&d_slots, (size_t)tiles));
        const dim3 g(tiles), b(kBlock);
        const bool wide = D.x % kCcVec == 0, full = c->ccConn == RTO_CONN_FULL;
        if (wide && full) hipLaunchKernelGGL((k_measure<true, true>), g, b, 0, s, c->d_ccLabels, D, T.x, T.y, table.d, d_slots);
        else if (wide) hipLaunchKernelGGL((k_measure<true, false>), g, b, 0, s, c->d_ccLabels, D, T.x, T.y, table.d, d_slots);
        else if (full) hipLaunchKernelGGL((k_measure<false, true>), g, b, 0, s, c->d_ccLabels, D, T.x, T.y, table.d, d_slots);
        else hipLaunchKernelGGL((k_measure<false, false>), g, b, 0, s, c->d_ccLabels, D, T.x, T.y, table.d, d_slots);
        RTO_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(k_measure_fold, dim3((tiles + kBlock - 1) / kBlock), b, 0, s, d_slots, tiles, table.d);
        RTO_HIP(c, hipGetLastError());
    }
    RTO_HIP(c, events.record(1, s));
    rto_measure sum;
    if (count) {
        const unsigned blocks = std::min<unsigned>((count + kBlock - 1) / kBlock, 1024u);
        hipLaunchKernelGGL(k_measure_total, dim3(blocks), dim3(kBlock), 0, s, table.d, count, c->ccConn == RTO_CONN_FULL ? 1 : 0);
        RTO_HIP(c, hipGetLastError());
    }
    RTO_HIP(c, hipMemcpyAsync(&sum, table.d + count, sizeof sum, hipMemcpyDeviceToHost, s));
    RTO_HIP(c, events.record(2, s));
    RTO_HIP(c, hipStreamSynchronize(s));
    float ms[2];
    for (int i = 0; i < 2; i++) RTO_HIP(c, events.elapsed(i, i + 1, &ms[i]));
    (void)hipFree(c->d_ccMeasures);
    c->d_ccMeasures = table.d;
    table.d = nullptr;
    c->measureMs[0] = ms[0]; c->measureMs[1] = ms[1];
    if (total) *total = sum;
    return RTO_OK;
}

int rto_download_measures(rto_context* c, rto_measure* out, int64_t capacity, int64_t* count) {
    if (!c) return RTO_E_INVALID;
    if (!c->d_ccMeasures) return fail(c, RTO_E_INVALID, "rto_download_measures: no measures are resident (not measured yet, or the labels have gone since)");
    if (count) *count = c->ccCount;
    if (!out) return RTO_OK;
    return download_resident(c, "rto_download_measures", out, capacity, c->d_ccMeasures, c->ccCount, sizeof(rto_measure));
}

int rto_measures_device(rto_context* c, rto_measure** d_measures, int64_t* count) {
    if (!c) return RTO_E_INVALID;
    if (!c->d_ccMeasures) return fail(c, RTO_E_INVALID, "rto_measures_device: no measures are resident (not measured yet, or the labels have gone since)");
    if (d_measures) *d_measures = c->d_ccMeasures;
    if (count) *count = c->ccCount;
    return RTO_OK;
}

int rto_last_measure_ms(const rto_context* c, float ms[2]) { return copy_last_ms(c, &rto_context::measureMs, ms); }

}  // extern "C"
