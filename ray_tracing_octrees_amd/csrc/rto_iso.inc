// rto_iso.inc -- field isosurfaces (include/rto_hip.h, rto_extract_isosurface_*): marching cubes of an int32 volume of the resident
// grid at a float level -- the reference's marchingCubesVolume (453-skeleton/MarchingCubes.cpp:622-689) with its marchingCubesCell /
// vertexInterp (:544-620) word for word, over the voxel centres.  Included at the end of rto_api.hip, after rto_field_view.inc
// (field_view_volume) and rto_mesh.inc (whose record layout this shares).
//
// Rule (DESIGN.md section 30).  All floats are float32, one IEEE operation per operator, in the order written, no contraction.
//   samples   one per voxel, at its centre: origin[a] = gridMin[a] + 0.5f * voxelSize, P_a(i) = origin[a] + (float)i * voxelSize; i
//             may be -1 or dim under pad.
//   value     a voxel inside the box [lo, hi) (the clip box, or [0, dim)) whose value v lies in [valid_lo, valid_hi] has (float)v;
//             every other sample (unvalued, outside the box, the pad ring) has `outside`.  Values above 2^24 round to nearest.
//   cells     without pad lo[a] <= c < hi[a] - 1 on every axis; with pad lo[a] - 1 <= c < hi[a].
//   cell      corners 0..7 at (0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1) (1,0,1) (1,1,1) (0,1,1); bit i of the case is set when
//             val_i < level; the 12 edges join the reference's corner pairs; a vertex is p1 when fabsf(level - v1) < 1e-6f, else p2
//             when fabsf(level - v2) < 1e-6f, else p1 when fabsf(v1 - v2) < 1e-6f, else p1 + ((level - v1) / (v2 - v1)) * (p2 - p1)
//             per component; the triangles are the case's row of the table (host/mc_cases.inc), in row order.
//   normal    n = cross(v1 - v0, v2 - v0), l2 = dot(n, n); l2 > 0 and finite: n * inversesqrt(l2); else (+0, +0, +0) and the
//             triangle stays in the list and counts as degenerate.
//   order     cells z slowest, then y, then x; within a cell the table's.
//   record    12 floats: v0, v1, v2, normal; tri_cell = ((z + 1) * (dimY + 1) + (y + 1)) * (dimX + 1) + (x + 1) of the owning cell.
//
// Shape.  Cells are addressed by u = c + 1 (never negative).  A run is 32 cells along x at an aligned u; runs are numbered in raster
// order over the cell box, so an exclusive scan of the runs' triangle counts is the reference's order and nothing is sorted.
//   k_iso_bricks   (with the table on) each 8^3 brick's smallest and largest substituted value, the volume read once.
//   k_iso_count    a workgroup per tile of 32 x 8 x 8 cells: a tile the level cannot cross (by the bricks its 33 x 9 x 9 samples
//                  touch) writes zero counts and leaves; the others stage their samples in LDS as floats with `outside` substituted,
//                  form every cell's case byte, keep it, and write one count per run (a half-wave sum).  No atomics.
//   k_iso_sums / k_iso_scan_sums / k_iso_offsets
//                  the exclusive scan of the triangles in 64 bits and, beside it in a word of its own, of the runs that hold a
//                  triangle, so the emit pass is launched over those alone.
//   k_iso_place    a half-wave per active run, a lane per cell: the lane's offset is the run's plus the prefix inside the run; it
//                  writes tri_cell and the triangle's place in its case for each of its up to 5 triangles, and counts active cells.
//   k_iso_emit     one thread per triangle, as k_mesh_emit_mc: it re-reads the two samples of each of its three edges and writes
//                  three float4; degenerate triangles are counted here.  Chosen for its balance (about 3 of a run's 32 cells hold a
//                  triangle on the 512^3 sphere); the one-thread-per-cell form with its samples in LDS was built first and timed
//                  only while the tally below still sat on one word, so no figure separates the two (DESIGN.md section 30).

namespace rto {

constexpr int kIsoTileX = 32, kIsoTileY = 8, kIsoTileZ = 8;
constexpr int kIsoSmpX = kIsoTileX + 1, kIsoSmpY = kIsoTileY + 1, kIsoSmpZ = kIsoTileZ + 1;
constexpr int kIsoSamples = kIsoSmpX * kIsoSmpY * kIsoSmpZ;
constexpr int kIsoRunsPerThread = 8;                         // k_iso_sums / k_iso_offsets: runs a thread scans
constexpr int kIsoRunsPerBlock = kIsoRunsPerThread * kBlock;
constexpr long long kIsoTooMany = 0x80000000ll;              // the count saturates here
constexpr int kIsoTallySlots = 256;                          // (active cells, degenerate triangles) pairs the workgroups add into: on one
                                                             // word the 175,000 adds of the 512^3 sphere took 2 ms, the whole emit pass
static_assert(kBlock == kIsoTileX * kIsoTileY, "k_iso_count: one thread per (x, y) column of a tile");

struct IsoArgs {
    const int* volume;               // dimZ x dimY x dimX, x fastest
    int dimX, dimY, dimZ;
    int lo[3], hi[3];                // the box of valued samples
    int uLo[3], uHi[3];              // the cells, as u = c + 1: uLo <= u < uHi
    int t0[3];                       // the first tile on each axis (uLo / the tile's edge)
    int runsX, ny, nz;               // runs along x, cells along y and z
    int validLo, validHi;
    float level, outside;
    float org[3], vs;
    int nbx, nby, nbz;               // bricks of the grid
    int useTable;
};

__device__ __forceinline__ float iso_sample(const IsoArgs& A, int x, int y, int z) {
    const bool in = x >= A.lo[0] && x < A.hi[0] && y >= A.lo[1] && y < A.hi[1] && z >= A.lo[2] && z < A.hi[2];
    if (!in) return A.outside;
    const int v = A.volume[((size_t)z * (size_t)A.dimY + (size_t)y) * (size_t)A.dimX + (size_t)x];
    return v >= A.validLo && v <= A.validHi ? (float)v : A.outside;
}

// One wave per run of 8 bricks along x, as k_project_bricks reads the volume: lane l owns column x = 64 run + l of the run's
// 8 x 8 (y, z) rows, groups of 8 lanes fold into one (min, max) per brick.  Unvalued voxels count as `outside`; the box does not
// enter (k_iso_count adds `outside` for a tile that reaches beyond it), so the table only ever widens a tile's range.
__global__ __launch_bounds__(kBlock) void k_iso_bricks(IsoArgs A, int runsX, unsigned waves, float2* __restrict__ bricks) {
    const unsigned w = blockIdx.x * (unsigned)(kBlock / kWave) + (threadIdx.x >> 6);      // wave-uniform
    if (w >= waves) return;
    const int lane = threadIdx.x & 63;
    const int rx = (int)(w % (unsigned)runsX);
    const unsigned row = w / (unsigned)runsX;
    const int by = (int)(row % (unsigned)A.nby), bz = (int)(row / (unsigned)A.nby);
    const int x = rx * 64 + lane;
    const int y1 = min(by * 8 + 8, A.dimY), z1 = min(bz * 8 + 8, A.dimZ);
    float mn = __builtin_inff(), mx = -__builtin_inff();
    if (x < A.dimX) {
        for (int z = bz * 8; z < z1; z++) {
            const int* row0 = A.volume + ((size_t)z * (size_t)A.dimY + (size_t)(by * 8)) * (size_t)A.dimX + (size_t)x;
            int v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = by * 8 + k < y1 ? row0[(size_t)k * (size_t)A.dimX] : 0;      // eight loads in flight
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const float f = v[k] >= A.validLo && v[k] <= A.validHi ? (float)v[k] : A.outside;
                if (by * 8 + k < y1) { mn = fminf(mn, f); mx = fmaxf(mx, f); }
            }
        }
    }
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) {              // the 8 lanes of a brick; min and max of finite floats: any order
        mn = fminf(mn, lane_xor(mn, off));
        mx = fmaxf(mx, lane_xor(mx, off));
    }
    const int bx = rx * 8 + (lane >> 3);
    if ((lane & 7) == 0 && bx < A.nbx) bricks[((size_t)bz * (size_t)A.nby + (size_t)by) * (size_t)A.nbx + (size_t)bx] = make_float2(mn, mx);
}

__device__ __forceinline__ size_t iso_run(const IsoArgs& A, int bx, int uy, int uz) {
    return ((size_t)(uz - A.uLo[2]) * (size_t)A.ny + (size_t)(uy - A.uLo[1])) * (size_t)A.runsX + (size_t)bx;
}

__global__ __launch_bounds__(kBlock) void k_iso_count(IsoArgs A, int tilesX, int tilesY, const unsigned long long* __restrict__ mcCases,
                                                     const float2* __restrict__ bricks, unsigned* __restrict__ runCount,
                                                     uint8_t* __restrict__ cases) {
    __shared__ float smp[kIsoSamples];
    __shared__ uint8_t triCount[256];
    const int t = (int)threadIdx.x;
    const int bx = (int)(blockIdx.x % (unsigned)tilesX);
    const unsigned rest = blockIdx.x / (unsigned)tilesX;
    const int by = (int)(rest % (unsigned)tilesY), bz = (int)(rest / (unsigned)tilesY);
    const int u0x = (A.t0[0] + bx) * kIsoTileX, u0y = (A.t0[1] + by) * kIsoTileY, u0z = (A.t0[2] + bz) * kIsoTileZ;
    const int s0x = u0x - 1, s0y = u0y - 1, s0z = u0z - 1;       // the tile's first sample

    if (A.useTable) {                                            // block-uniform: before any barrier
        float mn = __builtin_inff(), mx = -__builtin_inff();
        bool beyond = s0x < A.lo[0] || s0x + kIsoTileX >= A.hi[0] || s0y < A.lo[1] || s0y + kIsoTileY >= A.hi[1] ||
                      s0z < A.lo[2] || s0z + kIsoTileZ >= A.hi[2];
        for (int kz = s0z >> 3; kz <= (s0z + kIsoTileZ) >> 3; kz++)
            for (int ky = s0y >> 3; ky <= (s0y + kIsoTileY) >> 3; ky++)
                for (int kx = s0x >> 3; kx <= (s0x + kIsoTileX) >> 3; kx++) {
                    if (kx < 0 || ky < 0 || kz < 0 || kx >= A.nbx || ky >= A.nby || kz >= A.nbz) continue;      // `beyond` is set
                    const float2 r = bricks[((size_t)kz * (size_t)A.nby + (size_t)ky) * (size_t)A.nbx + (size_t)kx];
                    mn = fminf(mn, r.x); mx = fmaxf(mx, r.y);
                }
        if (beyond) { mn = fminf(mn, A.outside); mx = fmaxf(mx, A.outside); }
        if (mn >= A.level || mx < A.level) {                     // every case is 0, or every case is 255: no triangle
            if (t < kIsoTileY * kIsoTileZ) {
                const int uy = u0y + (t & 7), uz = u0z + (t >> 3);
                if (uy >= A.uLo[1] && uy < A.uHi[1] && uz >= A.uLo[2] && uz < A.uHi[2]) runCount[iso_run(A, bx, uy, uz)] = 0u;
            }
            return;
        }
    }

    triCount[t] = (uint8_t)(mcCases[t] >> 60);
    for (int i = t; i < kIsoSamples; i += kBlock) {
        const int sx = i % kIsoSmpX, r = i / kIsoSmpX;
        const int sy = r % kIsoSmpY, sz = r / kIsoSmpY;
        smp[i] = iso_sample(A, s0x + sx, s0y + sy, s0z + sz);
    }
    __syncthreads();

    const int lx = t & 31, ly = t >> 5;
    const int ux = u0x + lx, uy = u0y + ly;
    const bool inXY = ux >= A.uLo[0] && ux < A.uHi[0] && uy >= A.uLo[1] && uy < A.uHi[1];
    const bool rowY = uy >= A.uLo[1] && uy < A.uHi[1];           // uniform over the half-wave
    const float* col = smp + ly * kIsoSmpX + lx;
    const float level = A.level;
    // corners 0 1 2 3 of the cell above are corners 4 5 6 7 of this one
    unsigned low = (col[0] < level ? 1u : 0u) | (col[1] < level ? 2u : 0u) | (col[kIsoSmpX + 1] < level ? 4u : 0u) | (col[kIsoSmpX] < level ? 8u : 0u);
#pragma unroll
    for (int lz = 0; lz < kIsoTileZ; lz++) {
        const float* up = col + (lz + 1) * (kIsoSmpX * kIsoSmpY);
        const unsigned high = (up[0] < level ? 1u : 0u) | (up[1] < level ? 2u : 0u) | (up[kIsoSmpX + 1] < level ? 4u : 0u) | (up[kIsoSmpX] < level ? 8u : 0u);
        const int uz = u0z + lz;
        const bool rowZ = uz >= A.uLo[2] && uz < A.uHi[2];
        const unsigned cs = inXY && rowZ ? (low | high << 4) : 0u;             // a cell outside the box: case 0, no triangle
        unsigned n = triCount[cs];
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) n += lane_xor(n, off);          // the half-wave's 32 cells
        if (rowY && rowZ) {
            const size_t run = iso_run(A, bx, uy, uz);
            cases[run * 32 + (size_t)lx] = (uint8_t)cs;
            if (lx == 0) runCount[run] = n;
        }
        low = high;
    }
}

// Two quantities are scanned side by side, each in a word of its own: the triangles (64 bits: up to 5 a cell, below 2^34) and the
// runs that hold a triangle (32 bits: there are fewer than 2^31 runs).
__global__ __launch_bounds__(kBlock) void k_iso_sums(const unsigned* __restrict__ runCount, long long runs, long long* __restrict__ blockTris,
                                                    unsigned* __restrict__ blockActive) {
    const long long first = (long long)blockIdx.x * kIsoRunsPerBlock + (long long)threadIdx.x * kIsoRunsPerThread;
    long long tris = 0;
    unsigned active = 0u;
#pragma unroll
    for (int k = 0; k < kIsoRunsPerThread; k++) {
        const unsigned c = first + k < runs ? runCount[first + k] : 0u;
        tris += (long long)c;
        active += c ? 1u : 0u;
    }
    tris = block_sum<kBlock>(tris);
    active = block_sum<kBlock>(active);
    if (threadIdx.x == 0) { blockTris[blockIdx.x] = tris; blockActive[blockIdx.x] = active; }
}

// ONE workgroup: the exclusive scan of both arrays of block sums, in place, and the two totals.  k_scan_counts twice over, in one
// launch.
__global__ __launch_bounds__(1024) void k_iso_scan_sums(long long* __restrict__ blockTris, unsigned* __restrict__ blockActive, int n,
                                                        long long* __restrict__ totalTris, unsigned* __restrict__ totalActive) {
    long long carryTris = 0;
    unsigned carryActive = 0u;
    for (int i0 = 0; i0 < n; i0 += 1024) {
        const unsigned i = (unsigned)i0 + threadIdx.x;
        const bool in = i < (unsigned)n;
        long long allTris;
        unsigned allActive;
        const long long beforeTris = block_exclusive_scan<1024>(in ? blockTris[i] : 0ll, &allTris);
        const unsigned beforeActive = block_exclusive_scan<1024>(in ? blockActive[i] : 0u, &allActive);
        if (in) { blockTris[i] = carryTris + beforeTris; blockActive[i] = carryActive + beforeActive; }
        carryTris += allTris; carryActive += allActive;
        __syncthreads();                                     // the partials are read: the next round may write them
    }
    if (threadIdx.x == 0) { *totalTris = carryTris; *totalActive = carryActive; }
}

// The runs that hold a triangle, in order, and where each begins in the list (saturated: the call refuses such a total).
__global__ __launch_bounds__(kBlock) void k_iso_offsets(const unsigned* __restrict__ runCount, long long runs, const long long* __restrict__ blockTris,
                                                       const unsigned* __restrict__ blockActive, unsigned* __restrict__ activeRun,
                                                       unsigned* __restrict__ activeOff) {
    const long long first = (long long)blockIdx.x * kIsoRunsPerBlock + (long long)threadIdx.x * kIsoRunsPerThread;
    unsigned cnt[kIsoRunsPerThread];
    long long tris = 0;
    unsigned active = 0u;
#pragma unroll
    for (int k = 0; k < kIsoRunsPerThread; k++) {
        cnt[k] = first + k < runs ? runCount[first + k] : 0u;
        tris += (long long)cnt[k];
        active += cnt[k] ? 1u : 0u;
    }
    long long off = blockTris[blockIdx.x] + block_exclusive_scan<kBlock>(tris);
    unsigned rank = blockActive[blockIdx.x] + block_exclusive_scan<kBlock>(active);      // < the runs: inside both arrays
#pragma unroll
    for (int k = 0; k < kIsoRunsPerThread; k++) {
        if (cnt[k]) {
            activeRun[rank] = (unsigned)(first + k);
            activeOff[rank] = off > kIsoTooMany ? (unsigned)kIsoTooMany : (unsigned)off;
            rank++;
        }
        off += (long long)cnt[k];
    }
}

// A half-wave per active run, a lane per cell: the lane's offset is the run's plus the prefix inside the run; it writes, for each
// of its triangles, the owning cell (tri_cell itself) and case | k << 8 (k: the triangle's place in the case's row).
__global__ __launch_bounds__(kBlock) void k_iso_place(IsoArgs A, const unsigned long long* __restrict__ mcCases, const uint8_t* __restrict__ cases,
                                                     const unsigned* __restrict__ activeRun, const unsigned* __restrict__ activeOff, unsigned active,
                                                     int* __restrict__ triCell, unsigned short* __restrict__ triWhich, unsigned long long* __restrict__ tally) {
    __shared__ uint8_t triCount[256];
    const int t = (int)threadIdx.x;
    triCount[t] = (uint8_t)(mcCases[t] >> 60);
    __syncthreads();
    const unsigned hw = blockIdx.x * (unsigned)(kBlock / 32) + ((unsigned)t >> 5);
    const int lane = t & 31;
    const bool live = hw < active;                  // uniform over the half-wave, not over the wave
    unsigned cs = 0u, base = 0u;
    int cell = 0;
    if (live) {
        const unsigned run = activeRun[hw];
        base = activeOff[hw];
        const unsigned rx = run % (unsigned)A.runsX, q = run / (unsigned)A.runsX;
        const int ux = (A.t0[0] + (int)rx) * kIsoTileX + lane;
        const int uy = A.uLo[1] + (int)(q % (unsigned)A.ny), uz = A.uLo[2] + (int)(q / (unsigned)A.ny);
        cs = cases[(size_t)run * 32 + (size_t)lane];
        cell = (uz * (A.dimY + 1) + uy) * (A.dimX + 1) + ux;       // < 2^31 (iso_check)
    }
    const unsigned n = triCount[cs];
    unsigned incl = n;                              // the prefix inside the run
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {
        const unsigned up = __shfl_up(incl, off, 32);
        if (lane >= off) incl += up;
    }
    const size_t d0 = (size_t)base + (size_t)(incl - n);
    for (unsigned k = 0; k < n; k++) {
        triCell[d0 + k] = cell;
        triWhich[d0 + k] = (unsigned short)(cs | k << 8);
    }
    const unsigned nCells = block_sum<kBlock>(n ? 1u : 0u);      // every thread of the workgroup is here
    if (t == 0 && nCells) atomicAdd(tally + 2 * (blockIdx.x % kIsoTallySlots), (unsigned long long)nCells);
}

constexpr unsigned long long kIsoEdgeA = 0x321076543210ull, kIsoEdgeB = 0x765447650321ull;      // edge e joins corners nibble e of A and of B
constexpr unsigned kIsoCornerX = 0x66u, kIsoCornerY = 0xccu, kIsoCornerZ = 0xf0u;               // bit i: corner i sits at +1 on that axis

// One thread per triangle: its cell and its row of the case come from k_iso_place, the two samples of each of its three edges
// are re-read (the triangles of a cell and of its neighbours sit in the same wave: the loads hit the same lines).
__global__ __launch_bounds__(kBlock) void k_iso_emit(IsoArgs A, const unsigned long long* __restrict__ mcCases, const unsigned short* __restrict__ triWhich,
                                                    const int* __restrict__ triCell, unsigned total, float4* __restrict__ dst,
                                                    unsigned long long* __restrict__ tally) {
    const unsigned d = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    unsigned degenerate = 0u;
    if (d < total) {
        const unsigned which = triWhich[d], k = which >> 8;
        const unsigned long long cs = mcCases[which & 255u];
        const int cell = triCell[d];
        const int ux = cell % (A.dimX + 1), r = cell / (A.dimX + 1);
        const int x = ux - 1, y = r % (A.dimY + 1) - 1, z = r / (A.dimY + 1) - 1;
        const float level = A.level, vs = A.vs;
        float v[3][3];
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const unsigned e = (unsigned)(cs >> (4u * (3u * k + (unsigned)q))) & 15u;
            const unsigned a = (unsigned)(kIsoEdgeA >> (4u * e)) & 15u, b = (unsigned)(kIsoEdgeB >> (4u * e)) & 15u;
            const int ax = x + (int)((kIsoCornerX >> a) & 1u), ay = y + (int)((kIsoCornerY >> a) & 1u), az = z + (int)((kIsoCornerZ >> a) & 1u);
            const int bx = x + (int)((kIsoCornerX >> b) & 1u), by = y + (int)((kIsoCornerY >> b) & 1u), bz = z + (int)((kIsoCornerZ >> b) & 1u);
            const float v1 = iso_sample(A, ax, ay, az), v2 = iso_sample(A, bx, by, bz);
            const float p1x = A.org[0] + (float)ax * vs, p1y = A.org[1] + (float)ay * vs, p1z = A.org[2] + (float)az * vs;
            const float p2x = A.org[0] + (float)bx * vs, p2y = A.org[1] + (float)by * vs, p2z = A.org[2] + (float)bz * vs;
            if (fabsf(level - v1) < 1e-6f) { v[q][0] = p1x; v[q][1] = p1y; v[q][2] = p1z; }
            else if (fabsf(level - v2) < 1e-6f) { v[q][0] = p2x; v[q][1] = p2y; v[q][2] = p2z; }
            else if (fabsf(v1 - v2) < 1e-6f) { v[q][0] = p1x; v[q][1] = p1y; v[q][2] = p1z; }
            else {
                const float mu = (level - v1) / (v2 - v1);
                v[q][0] = p1x + mu * (p2x - p1x); v[q][1] = p1y + mu * (p2y - p1y); v[q][2] = p1z + mu * (p2z - p1z);
            }
        }
        const float ax = v[1][0] - v[0][0], ay = v[1][1] - v[0][1], az = v[1][2] - v[0][2];
        const float bx = v[2][0] - v[0][0], by = v[2][1] - v[0][1], bz = v[2][2] - v[0][2];
        const float cx = ay * bz - by * az, cy = az * bx - bz * ax, cz = ax * by - bx * ay;      // glm cross
        const float tx = cx * cx, ty = cy * cy, tz = cz * cz;
        const float l2 = tx + ty + tz;
        float nx = 0.0f, ny = 0.0f, nz = 0.0f;
        if (l2 > 0.0f && __builtin_isfinite(l2)) {
            const float inv = inversesqrt(l2);
            nx = cx * inv; ny = cy * inv; nz = cz * inv;
        } else degenerate = 1u;
        float4* o = dst + 3 * (size_t)d;
        o[0] = make_float4(v[0][0], v[0][1], v[0][2], v[1][0]);
        o[1] = make_float4(v[1][1], v[1][2], v[2][0], v[2][1]);
        o[2] = make_float4(v[2][2], nx, ny, nz);
    }
    const unsigned nDeg = wave_sum(degenerate);     // every lane of the wave is here
    if ((threadIdx.x & 63) == 0 && nDeg) atomicAdd(tally + 2 * (blockIdx.x % kIsoTallySlots) + 1, (unsigned long long)nDeg);
}

}  // namespace rto

// ---------------------------------------------------------------- host side
static_assert(sizeof(rto_iso_params) == 64 && sizeof(rto_iso_summary) == 32, "the ABI's sizes");

// Every check of an extraction up to the volume, in the order the ABI promises; *volume: the int32 volume to contour (CALLER: the
// pointer given, which the host form replaces by its upload).
static int iso_check(rto_context* c, const char* fn, const rto_iso_params* p, const int32_t* given, const int** volume) {
    const std::string name(fn);
    if (!p) return fail(c, RTO_E_INVALID, name + ": params is NULL");
    if ((reinterpret_cast<uintptr_t>(given) & 3) != 0) return fail(c, RTO_E_INVALID, name + ": the volume must be 4-byte aligned");
    if (p->source < RTO_FIELD_DISTANCE || p->source > RTO_FIELD_CALLER) return fail(c, RTO_E_INVALID, name + ": unknown source " + std::to_string(p->source));
    for (int r : p->reserved) if (r != 0) return fail(c, RTO_E_INVALID, name + ": params.reserved must be 0");
    int rc = check_valid_window(c, name, p->valid_lo, p->valid_hi);
    if (rc != RTO_OK) return rc;
    if (!std::isfinite(p->level) || !std::isfinite(p->outside)) return fail(c, RTO_E_INVALID, name + ": level and outside must be finite");
    if (p->pad != 0 && p->pad != 1) return fail(c, RTO_E_INVALID, name + ": pad must be 0 or 1");
    if ((rc = check_caller_volume(c, name, p->source, given)) != RTO_OK) return rc;
    if (c->numNodes <= 0) return fail(c, RTO_E_NO_OCTREE, name + ": no octree uploaded");
    if (!c->d_vox) return fail(c, RTO_E_UNSUPPORTED, name + ": the octree came from rto_upload_octree: no voxel grid is resident");
    if (((int64_t)c->voxDim[0] + 1) * ((int64_t)c->voxDim[1] + 1) * ((int64_t)c->voxDim[2] + 1) >= 0x80000000ll)
        return fail(c, RTO_E_UNSUPPORTED, name + ": (dimX + 1)(dimY + 1)(dimZ + 1) is 2^31 or more: a cell's index does not fit tri_cell");
    if ((rc = check_clip_box(c, name, p->clip, p->clip_lo, p->clip_hi)) != RTO_OK) return rc;
    return field_view_volume(c, fn, p->source, given, volume);
}

// The extraction itself: the device is set, every check but the triangle count has passed, `volume` is on the device.
static int iso_extract(rto_context* c, const char* fn, const rto_iso_params* p, const int* volume, rto_iso_summary* summary) {
    using namespace rto;
    hipStream_t s = c->stream;
    IsoArgs A;
    std::memset(&A, 0, sizeof A);
    A.volume = volume;
    A.dimX = c->voxDim[0]; A.dimY = c->voxDim[1]; A.dimZ = c->voxDim[2];
    bool empty = false;
    const int tile[3] = { kIsoTileX, kIsoTileY, kIsoTileZ };
    int tiles[3] = { 0, 0, 0 }, cells[3] = { 0, 0, 0 };
    for (int a = 0; a < 3; a++) {
        A.lo[a] = p->clip ? p->clip_lo[a] : 0;
        A.hi[a] = p->clip ? p->clip_hi[a] : c->voxDim[a];
        A.uLo[a] = A.lo[a] - p->pad + 1;                         // cells lo - pad <= c < hi - 1 + pad, as u = c + 1
        A.uHi[a] = A.hi[a] - 1 + p->pad + 1;
        cells[a] = A.uHi[a] - A.uLo[a];
        if (cells[a] <= 0) { empty = true; continue; }
        A.t0[a] = A.uLo[a] / tile[a];
        tiles[a] = (A.uHi[a] + tile[a] - 1) / tile[a] - A.t0[a];
        A.org[a] = c->gridMin[a] + 0.5f * c->voxelSize;
    }
    A.vs = c->voxelSize;
    A.runsX = tiles[0]; A.ny = cells[1]; A.nz = cells[2];
    A.validLo = p->valid_lo; A.validHi = p->valid_hi;
    A.level = p->level; A.outside = p->outside;
    A.nbx = (A.dimX + 7) / 8; A.nby = (A.dimY + 7) / 8; A.nbz = (A.dimZ + 7) / 8;
    A.useTable = c->pjTable ? 1 : 0;

    long long total = 0, activeRuns = 0;
    std::vector<unsigned long long> slots(2 * kIsoTallySlots, 0ull);
    unsigned long long tally[2] = { 0ull, 0ull };
    float ms[3] = { -1.f, -1.f, -1.f };                       // an empty cell box runs no kernel
    if (!empty) {
        if (!c->d_mcCases) {
            unsigned long long packed[256];
            pack_mc_cases(packed);
            RTO_HIP(c, hipMalloc(&c->d_mcCases, sizeof packed));
            RTO_HIP(c, hipMemcpy(c->d_mcCases, packed, sizeof packed, hipMemcpyHostToDevice));
        }
        // count: events 0 .. 1 (the brick table with it); rank: 1 .. 2; emit: 3 .. 4, begun after the count's read-back and the
        // output buffer's growth, which belong to the call's wall time and to no phase
        StreamEvents<5> events;
        RTO_HIP(c, events.create());
        BuildScratch scratch(s);
        const long long runs = (long long)A.runsX * A.ny * A.nz;             // < 2^31 cells / 32 + the rows' ends
        const long long nb = (runs + kIsoRunsPerBlock - 1) / kIsoRunsPerBlock;
        unsigned *d_runCount = nullptr, *d_activeRun = nullptr, *d_activeOff = nullptr;
        uint8_t* d_cases = nullptr;
        long long *d_blockTris = nullptr, *d_total = nullptr;
        unsigned *d_blockActive = nullptr, *d_totalActive = nullptr;
        float2* d_bricks = nullptr;
        unsigned long long* d_tally = nullptr;
        RTO_HIP(c, scratch.alloc(&d_runCount, (size_t)runs));
        RTO_HIP(c, scratch.alloc(&d_activeRun, (size_t)runs));
        RTO_HIP(c, scratch.alloc(&d_activeOff, (size_t)runs));
        RTO_HIP(c, scratch.alloc(&d_cases, (size_t)runs * 32));
        RTO_HIP(c, scratch.alloc(&d_blockTris, (size_t)nb));
        RTO_HIP(c, scratch.alloc(&d_blockActive, (size_t)nb));
        RTO_HIP(c, scratch.alloc(&d_total, 1));
        RTO_HIP(c, scratch.alloc(&d_totalActive, 1));
        RTO_HIP(c, scratch.alloc(&d_tally, slots.size()));
        if (A.useTable) RTO_HIP(c, scratch.alloc(&d_bricks, (size_t)A.nbx * A.nby * A.nbz));
        RTO_HIP(c, hipMemsetAsync(d_tally, 0, slots.size() * sizeof(unsigned long long), s));

        RTO_HIP(c, events.record(0, s));
        if (A.useTable) {
            const int runsB = (A.nbx + 7) / 8;
            const int64_t waves = (int64_t)runsB * A.nby * A.nbz;
            hipLaunchKernelGGL(k_iso_bricks, dim3((unsigned)((waves + kBlock / kWave - 1) / (kBlock / kWave))), dim3(kBlock), 0, s, A, runsB, (unsigned)waves, d_bricks);
        }
        hipLaunchKernelGGL(k_iso_count, dim3((unsigned)((int64_t)tiles[0] * tiles[1] * tiles[2])), dim3(kBlock), 0, s, A, tiles[0], tiles[1], c->d_mcCases,
                           d_bricks, d_runCount, d_cases);
        RTO_HIP(c, hipGetLastError());
        RTO_HIP(c, events.record(1, s));
        hipLaunchKernelGGL(k_iso_sums, dim3((unsigned)nb), dim3(kBlock), 0, s, d_runCount, runs, d_blockTris, d_blockActive);
        hipLaunchKernelGGL(k_iso_scan_sums, dim3(1), dim3(1024), 0, s, d_blockTris, d_blockActive, (int)nb, d_total, d_totalActive);
        hipLaunchKernelGGL(k_iso_offsets, dim3((unsigned)nb), dim3(kBlock), 0, s, d_runCount, runs, d_blockTris, d_blockActive, d_activeRun, d_activeOff);
        RTO_HIP(c, hipGetLastError());
        RTO_HIP(c, events.record(2, s));
        unsigned active = 0u;
        RTO_HIP(c, hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, s));     // the read-back that sizes the output
        RTO_HIP(c, hipMemcpyAsync(&active, d_totalActive, sizeof active, hipMemcpyDeviceToHost, s));
        RTO_HIP(c, hipStreamSynchronize(s));
        activeRuns = (long long)active;
        if (total >= kIsoTooMany) return fail(c, RTO_E_UNSUPPORTED, std::string(fn) + ": more than 2^31 - 1 triangles");

        // ---- emit into a buffer of the context's own (the previous isosurface lives until here)
        if (total > c->isoCap || !c->d_iso) {
            float4* d_new = nullptr;
            int* d_newCell = nullptr;
            const size_t cap = total ? (size_t)total : 1;
            RTO_HIP(c, hipMalloc(&d_new, cap * 3 * sizeof(float4)));
            if (hipMalloc(&d_newCell, cap * sizeof(int)) != hipSuccess) { (void)hipFree(d_new); return fail(c, RTO_E_HIP, std::string(fn) + ": out of device memory"); }
            (void)hipFree(c->d_iso); (void)hipFree(c->d_isoCell);
            c->d_iso = d_new; c->d_isoCell = d_newCell; c->isoCap = (int64_t)cap;
            c->isoTris = -1;                                 // the old list is gone: nothing is served until this one is complete
        }
        unsigned short* d_which = nullptr;
        RTO_HIP(c, scratch.alloc(&d_which, (size_t)total));
        RTO_HIP(c, events.record(3, s));
        if (total > 0) {
            hipLaunchKernelGGL(k_iso_place, dim3((unsigned)((activeRuns + kBlock / 32 - 1) / (kBlock / 32))), dim3(kBlock), 0, s, A, c->d_mcCases, d_cases,
                               d_activeRun, d_activeOff, (unsigned)activeRuns, c->d_isoCell, d_which, d_tally);
            hipLaunchKernelGGL(k_iso_emit, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, A, c->d_mcCases, d_which, c->d_isoCell,
                               (unsigned)total, c->d_iso, d_tally);
            RTO_HIP(c, hipGetLastError());
        }
        RTO_HIP(c, events.record(4, s));
        RTO_HIP(c, hipMemcpyAsync(slots.data(), d_tally, slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        RTO_HIP(c, hipStreamSynchronize(s));
        for (int k = 0; k < kIsoTallySlots; k++) { tally[0] += slots[2 * k]; tally[1] += slots[2 * k + 1]; }
        RTO_HIP(c, events.elapsed(0, 1, &ms[0]));
        RTO_HIP(c, events.elapsed(1, 2, &ms[1]));
        RTO_HIP(c, events.elapsed(3, 4, &ms[2]));
    }
    c->isoTris = (int64_t)total;
    std::memcpy(c->isoMs, ms, sizeof ms);
    if (summary) { summary->triangles = (int64_t)total; summary->active_cells = (int64_t)tally[0]; summary->degenerate = (int64_t)tally[1]; summary->reserved = 0; }
    return RTO_OK;
}

extern "C" {

int rto_extract_isosurface_device(rto_context* c, const rto_iso_params* params, const int32_t* d_volume, rto_iso_summary* summary) {
    if (!c) return RTO_E_INVALID;
    const char* fn = "rto_extract_isosurface_device";
    const int* volume = nullptr;
    const int rc = iso_check(c, fn, params, d_volume, &volume);
    if (rc != RTO_OK) return rc;
    RTO_HIP(c, hipSetDevice(c->device));
    return iso_extract(c, fn, params, volume, summary);
}

int rto_extract_isosurface_host(rto_context* c, const rto_iso_params* params, const int32_t* host_volume, rto_iso_summary* summary) {
    if (!c) return RTO_E_INVALID;
    const char* fn = "rto_extract_isosurface_host";
    const int* volume = nullptr;
    const int rc = iso_check(c, fn, params, host_volume, &volume);
    if (rc != RTO_OK) return rc;
    RTO_HIP(c, hipSetDevice(c->device));
    BuildScratch scratch(c->stream);
    if (host_volume) {                                               // RTO_FIELD_CALLER (iso_check)
        int32_t* d_volume = nullptr;
        RTO_HIP(c, scratch.alloc(&d_volume, (size_t)grid_voxels(c)));
        RTO_HIP(c, hipMemcpyAsync(d_volume, host_volume, (size_t)grid_voxels(c) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        volume = d_volume;
    }
    return iso_extract(c, fn, params, volume, summary);
}

int rto_isosurface_device(rto_context* c, void** d_tris, int32_t** d_tri_cell, int64_t* num_tris) {
    if (!c || !num_tris) return RTO_E_INVALID;
    if (c->isoTris < 0) return fail(c, RTO_E_INVALID, "rto_isosurface_device: no isosurface extracted");
    if (d_tris) *d_tris = c->d_iso;
    if (d_tri_cell) *d_tri_cell = c->d_isoCell;
    *num_tris = c->isoTris;
    return RTO_OK;
}

int rto_download_isosurface(rto_context* c, float* tris, int64_t capacity, int32_t* tri_cell, int64_t* num_tris) {
    if (!c || !num_tris) return RTO_E_INVALID;
    if (c->isoTris < 0) return fail(c, RTO_E_INVALID, "rto_download_isosurface: no isosurface extracted");
    *num_tris = c->isoTris;
    if (!tris && !tri_cell) return RTO_OK;
    if (capacity < c->isoTris) return fail(c, RTO_E_INVALID, "rto_download_isosurface: capacity too small");
    if (c->isoTris == 0) return RTO_OK;
    RTO_HIP(c, hipSetDevice(c->device));
    RTO_HIP(c, hipStreamSynchronize(c->stream));
    if (tris) RTO_HIP(c, hipMemcpy(tris, c->d_iso, (size_t)c->isoTris * 12 * sizeof(float), hipMemcpyDeviceToHost));
    if (tri_cell) RTO_HIP(c, hipMemcpy(tri_cell, c->d_isoCell, (size_t)c->isoTris * sizeof(int), hipMemcpyDeviceToHost));
    return RTO_OK;
}

int rto_last_isosurface_ms(const rto_context* c, float ms[3]) { return copy_last_ms(c, &rto_context::isoMs, ms); }

}  // extern "C"
