// rto_components.inc -- connected components of the resident grid (include/rto_hip.h, rto_label_components / rto_edit_components):
// labels the FILLED or the EMPTY voxels of the grid rto_build_octree keeps in HBM under 6- or 26-connectivity, keeps the label
// volume and the component table resident, and flips whole components (debris removal, cavity filling) with the voxel edits'
// rebuild.  Included at the end of rto_api.hip.
//
// Rule (DESIGN.md section 18).  Voxel (i, j, k) has linear index v = i + dimX (j + dimY k).  A component's root is its smallest
// linear index; components are numbered in ascending order of root; the label volume holds that number, -1 outside the set.
//
// Phases: (1) k_cc_local: one workgroup labels one 32 x 8 x 8 tile in LDS and writes a 32-bit parent per voxel (the global index
// of the tile-local root, kCcNone outside the set); (2) k_cc_merge unites the trees of every neighbour pair that straddles a tile
// face with agent-scope atomics, and runs again until a pass finds every such pair already joined; (3) k_cc_flatten points every
// voxel at its root and counts roots per chunk, k_scan_counts / k_cc_rank number the roots in index order, k_cc_label writes the
// volume; (4) k_cc_stats fills the table.  Every dependence between workgroups crosses a kernel boundary: no kernel waits for
// another workgroup.  Parents only ever decrease, so every find chain and every retry loop strictly descends.

namespace rto {

constexpr unsigned kCcNone = 0xffffffffu;
constexpr int kCcTileX = 32, kCcTileY = 8, kCcTileZ = 8;                 // one workgroup's tile: rows along x
constexpr int kCcTileVox = kCcTileX * kCcTileY * kCcTileZ;               // 2048 voxels, 8 per thread
constexpr int kCcSeg = kCcTileVox / kBlock;                              // a thread's x-run inside one tile row
constexpr int kCcVec = 16;                                               // bytes per wide load
constexpr int kCcPerThread = 16;                                         // voxels per thread of the streaming kernels
constexpr int kCcChunk = kBlock * kCcPerThread;                          // voxels per block there
constexpr int kCcMaxPasses = 32;
static_assert(kCcSeg == 8 && kCcTileX % kCcSeg == 0, "a thread owns 8 voxels of one tile row");

struct CcDims { int x, y, z; unsigned n; };

// The forward half of the neighbourhood: d > 0 in (z, y, x) order.  FACE uses entries 0, 1 and 4 (kCcFaceDirs).
__device__ constexpr signed char kCcDirs[13][3] = {
    { 1, 0, 0 }, { 0, 1, 0 }, { -1, 1, 0 }, { 1, 1, 0 }, { 0, 0, 1 },
    { -1, 0, 1 }, { 1, 0, 1 }, { 0, -1, 1 }, { -1, -1, 1 }, { 1, -1, 1 }, { 0, 1, 1 }, { -1, 1, 1 }, { 1, 1, 1 } };
__device__ constexpr int kCcFaceDirs[3] = { 0, 1, 4 };

// ---- phase 1: tile-local labelling in LDS
__device__ __forceinline__ unsigned cc_lds_find(const unsigned* L, unsigned a) {
    unsigned p = __hip_atomic_load(&L[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    while (p != a) { a = p; p = __hip_atomic_load(&L[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    return a;
}
__device__ __forceinline__ void cc_lds_unite(unsigned* L, unsigned a, unsigned b) {
    a = cc_lds_find(L, a); b = cc_lds_find(L, b);
    while (a != b) {
        if (a < b) { const unsigned t = a; a = b; b = t; }
        const unsigned old = __hip_atomic_fetch_min(&L[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == a) break;
        a = cc_lds_find(L, old); b = cc_lds_find(L, b);
    }
}

// Thread t owns the 8 voxels [8 (t % 4), 8 (t % 4) + 8) of tile row t / 4 (row = ly + 8 lz).  L[i]: the parent of local voxel
// i = lx + 32 row, kCcNone outside the set or the grid.  Local order is global order inside a tile, so the local root (smallest
// local index) is the voxel with the smallest global index.  A pair (v, v + d) with d off the x axis is skipped when (v - x,
// v - x + d) is a pair of the set inside the tile too: x-adjacency already joins them to it.
template <bool WIDE, bool FULL>
__global__ __launch_bounds__(kBlock) void k_cc_local(const uint8_t* __restrict__ vox, CcDims D, int tilesX, int tilesY, unsigned setValue,
                                                    unsigned* __restrict__ parent) {
    __shared__ unsigned L[kCcTileVox];
    const int t = (int)threadIdx.x;
    const int bid = (int)blockIdx.x;
    const int x0 = (bid % tilesX) * kCcTileX, y0 = ((bid / tilesX) % tilesY) * kCcTileY, z0 = (bid / (tilesX * tilesY)) * kCcTileZ;
    const int row = t / (kCcTileX / kCcSeg), seg = t % (kCcTileX / kCcSeg);
    const int lx0 = seg * kCcSeg, ly = row % kCcTileY, lz = row / kCcTileY;
    const int gx0 = x0 + lx0, gy = y0 + ly, gz = z0 + lz;
    const bool rowIn = gy < D.y && gz < D.z;
    const size_t rowBase = ((size_t)gz * D.y + gy) * (size_t)D.x;
    unsigned in = 0u;                                               // bit j: voxel gx0 + j belongs to the set
    if (rowIn) {
        if (WIDE) {                                                 // dimX % 16 == 0: a 16-byte chunk is wholly inside or outside
            const int c0 = gx0 & ~(kCcVec - 1);
            if (c0 < D.x) {
                const uint4 w = *reinterpret_cast<const uint4*>(vox + rowBase + c0);
                const unsigned lo = (gx0 & 8) ? w.z : w.x, hi = (gx0 & 8) ? w.w : w.y;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    in |= (((lo >> (8 * j)) & 0xffu) == setValue ? 1u : 0u) << j;
                    in |= (((hi >> (8 * j)) & 0xffu) == setValue ? 1u : 0u) << (4 + j);
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < kCcSeg; j++)
                if (gx0 + j < D.x) in |= ((unsigned)vox[rowBase + gx0 + j] == setValue ? 1u : 0u) << j;
        }
    }
    const int base = row * kCcTileX + lx0;
    {
        unsigned cur = kCcNone;
#pragma unroll
        for (int j = 0; j < kCcSeg; j++) {
            const bool s = (in >> j) & 1u;
            cur = s ? (cur == kCcNone ? (unsigned)(base + j) : cur) : kCcNone;
            L[base + j] = cur;
        }
    }
    __syncthreads();
    if (in) {
        if (lx0 > 0 && (in & 1u) && L[base - 1] != kCcNone) cc_lds_unite(L, (unsigned)base, (unsigned)(base - 1));
        constexpr int nd = FULL ? 13 : 3;
        for (int k = 1; k < nd; k++) {
            const int di = FULL ? k : kCcFaceDirs[k];
            const int dx = kCcDirs[di][0], dy = kCcDirs[di][1], dz = kCcDirs[di][2];
            const int ny = ly + dy, nz = lz + dz;
            if (ny < 0 || ny >= kCcTileY || nz >= kCcTileZ) continue;
            const int nrow = (nz * kCcTileY + ny) * kCcTileX;
            bool prev = false;                                      // the pair one step back along x was a pair of the set
            if (lx0 > 0 && lx0 - 1 + dx >= 0) prev = L[base - 1] != kCcNone && L[nrow + lx0 - 1 + dx] != kCcNone;
#pragma unroll
            for (int j = 0; j < kCcSeg; j++) {
                const int nx = lx0 + j + dx;
                bool both = false;
                if (nx >= 0 && nx < kCcTileX) both = ((in >> j) & 1u) && L[nrow + nx] != kCcNone;
                if (both && !prev) cc_lds_unite(L, (unsigned)(base + j), (unsigned)(nrow + nx));
                prev = both && nx >= 0;                             // nx - 1 + 1 must lie in the tile for the next step's shortcut
            }
        }
    }
    __syncthreads();
    if (rowIn) {
#pragma unroll
        for (int j = 0; j < kCcSeg; j++) {
            if (gx0 + j >= D.x) break;
            unsigned p = kCcNone;
            if ((in >> j) & 1u) {
                const unsigned r = cc_lds_find(L, (unsigned)(base + j));
                const int rx = (int)(r % kCcTileX), ry = (int)((r / kCcTileX) % kCcTileY), rz = (int)(r / (kCcTileX * kCcTileY));
                p = (unsigned)(((size_t)(z0 + rz) * D.y + (y0 + ry)) * (size_t)D.x + (x0 + rx));
            }
            parent[rowBase + gx0 + j] = p;
        }
    }
}

// ---- phase 2: merging across tile faces
__device__ __forceinline__ unsigned cc_load(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned cc_find(const unsigned* P, unsigned a) {
    unsigned p = cc_load(&P[a]);
    while (p != a) { a = p; p = cc_load(&P[a]); }       // p < a: strictly descending
    return a;
}
__device__ __forceinline__ void cc_unite(unsigned* P, unsigned a, unsigned b) {
    while (a != b) {
        if (a < b) { const unsigned t = a; a = b; b = t; }
        const unsigned old = __hip_atomic_fetch_min(&P[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) break;                              // a was a root and now hangs under b
        a = cc_find(P, old); b = cc_find(P, b);           // a's earlier parent must end up with b as well
    }
}

// One thread per voxel.  For every forward neighbour in another tile: both in the set and not yet under one root -> raise the
// flag and unite.  A pass that leaves the flag at 0 has written nothing, so it has read one consistent forest: the labelling is
// complete.  The x-shortcut of k_cc_local applies: the pair one step back along x is a pair of some tile or of this kernel.
template <bool FULL>
__global__ __launch_bounds__(kBlock) void k_cc_merge(unsigned* __restrict__ parent, CcDims D, int* __restrict__ flag) {
    const unsigned v = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    if (v >= D.n) return;
    const int x = (int)(v % (unsigned)D.x), y = (int)((v / (unsigned)D.x) % (unsigned)D.y), z = (int)(v / ((unsigned)D.x * (unsigned)D.y));
    const int lx = x % kCcTileX, ly = y % kCcTileY, lz = z % kCcTileZ;
    if (lx != 0 && lx != kCcTileX - 1 && ly != 0 && ly != kCcTileY - 1 && lz != kCcTileZ - 1) return;
    if (cc_load(&parent[v]) == kCcNone) return;
    constexpr int nd = FULL ? 13 : 3;
    for (int k = 0; k < nd; k++) {
        const int di = FULL ? k : kCcFaceDirs[k];
        const int dx = kCcDirs[di][0], dy = kCcDirs[di][1], dz = kCcDirs[di][2];
        const int nx = x + dx, ny = y + dy, nz = z + dz;
        if (nx < 0 || nx >= D.x || ny < 0 || ny >= D.y || nz >= D.z) continue;
        if (nx / kCcTileX == x / kCcTileX && ny / kCcTileY == y / kCcTileY && nz / kCcTileZ == z / kCcTileZ) continue;
        const unsigned w = (unsigned)(((size_t)nz * D.y + ny) * (size_t)D.x + nx);
        if (cc_load(&parent[w]) == kCcNone) continue;
        if ((dy != 0 || dz != 0) && x > 0 && nx > 0 && cc_load(&parent[v - 1]) != kCcNone && cc_load(&parent[w - 1]) != kCcNone) continue;
        const unsigned a = cc_find(parent, v), b = cc_find(parent, w);
        if (a != b) {
            __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            cc_unite(parent, a, b);
        }
    }
}

// ---- phase 3: flatten, rank, label.  A block owns kCcChunk consecutive voxels; thread t its voxels base + j * kBlock + t.
__global__ __launch_bounds__(kBlock) void k_cc_flatten(unsigned* __restrict__ parent, unsigned n, unsigned* __restrict__ blockCount) {
    const unsigned base = blockIdx.x * (unsigned)kCcChunk;
    int roots = 0;
#pragma unroll 4
    for (int j = 0; j < kCcPerThread; j++) {
        const unsigned v = base + (unsigned)j * kBlock + threadIdx.x;
        if (v < n) {
            const unsigned p = cc_load(&parent[v]);
            if (p != kCcNone) {
                const unsigned r = p == v ? v : cc_find(parent, p);
                if (r != p) __hip_atomic_store(&parent[v], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                roots += r == v ? 1 : 0;
            }
        }
    }
    roots = block_sum<kBlock>(roots);
    if (threadIdx.x == 0) blockCount[blockIdx.x] = (unsigned)roots;
}

struct CcComp {                    // rto_component's layout
    long long root, voxels;
    int lo[3], hi[3];
    int touches, reserved;
};
static_assert(sizeof(CcComp) == 48, "rto_component is 48 bytes");

// Roots in index order: the r-th root of the grid is component r.  Writes its number into the label volume at the root and
// starts its table entry.
__global__ __launch_bounds__(kBlock) void k_cc_rank(const unsigned* __restrict__ parent, unsigned n, const unsigned* __restrict__ blockBase,
                                                   int* __restrict__ labels, CcComp* __restrict__ comps) {
    const unsigned base = blockIdx.x * (unsigned)kCcChunk;
    unsigned rank = blockBase[blockIdx.x];
    for (int j = 0; j < kCcPerThread; j++) {
        const unsigned v = base + (unsigned)j * kBlock + threadIdx.x;
        const bool isRoot = v < n && parent[v] == v;
        int all;
        const int before = block_rank<kBlock>(isRoot, &all);             // roots of this row of the chunk before v
        if (isRoot) {
            const unsigned r = rank + (unsigned)before;
            labels[v] = (int)r;
            CcComp c;
            c.root = (long long)v; c.voxels = 0;
            c.lo[0] = c.lo[1] = c.lo[2] = 0x7fffffff; c.hi[0] = c.hi[1] = c.hi[2] = -1;
            c.touches = 0; c.reserved = 0;
            comps[r] = c;
        }
        rank += all;
        __syncthreads();
    }
}

// labels[v] = the number at v's root (written by the launch before), -1 outside the set.  A root rewrites its own value.
__global__ __launch_bounds__(kBlock) void k_cc_label(const unsigned* __restrict__ parent, unsigned n, int* __restrict__ labels) {
    const unsigned base = blockIdx.x * (unsigned)kCcChunk;
#pragma unroll 4
    for (int j = 0; j < kCcPerThread; j++) {
        const unsigned v = base + (unsigned)j * kBlock + threadIdx.x;
        if (v < n) {
            const unsigned p = parent[v];
            if (p == kCcNone) labels[v] = -1;
            else if (p != v) labels[v] = labels[p];
        }
    }
}

// ---- phase 4: statistics.  A thread folds its 32 consecutive voxels into one accumulator while the label stays the same and sends
// it off when the label changes; what is left at the end is combined over the wave when the whole wave holds one label (the huge component
// of a typical scene), then over the block's waves in LDS, so that such a component costs one set of atomics per block.
struct CcAcc { int label; unsigned count; int lo[3], hi[3]; };

__device__ __forceinline__ void cc_acc_send(CcComp* __restrict__ comps, const CcAcc& a) {
    CcComp* c = &comps[a.label];
    atomicAdd(reinterpret_cast<unsigned long long*>(&c->voxels), (unsigned long long)a.count);
#pragma unroll
    for (int k = 0; k < 3; k++) { atomicMin(&c->lo[k], a.lo[k]); atomicMax(&c->hi[k], a.hi[k]); }
}

constexpr int kCcStatPerThread = 32;
__global__ __launch_bounds__(kBlock) void k_cc_stats(const int* __restrict__ labels, CcDims D, CcComp* __restrict__ comps) {
    // thread t owns 32 consecutive voxels (one stretch of a row, or the end of one and the start of the next): labels change
    // along x only at run ends, so the accumulator is sent off about once per run, never once per voxel of a large component
    const unsigned v0 = (blockIdx.x * (unsigned)kBlock + threadIdx.x) * (unsigned)kCcStatPerThread;
    CcAcc a;
    a.label = -1; a.count = 0;
    if (v0 < D.n) {
        int x = (int)(v0 % (unsigned)D.x), y = (int)((v0 / (unsigned)D.x) % (unsigned)D.y), z = (int)(v0 / ((unsigned)D.x * (unsigned)D.y));
        const bool whole = v0 + (unsigned)kCcStatPerThread <= D.n;
        for (int q = 0; q < kCcStatPerThread / 4; q++) {
            int ls[4] = { -1, -1, -1, -1 };
            if (whole) {                                               // 16-byte aligned: v0 is a multiple of 32
                const int4 l4 = *reinterpret_cast<const int4*>(labels + v0 + 4 * q);
                ls[0] = l4.x; ls[1] = l4.y; ls[2] = l4.z; ls[3] = l4.w;
            } else {
                for (int j = 0; j < 4; j++) if (v0 + (unsigned)(4 * q + j) < D.n) ls[j] = labels[v0 + 4 * q + j];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int l = ls[j];
                if (l >= 0) {
                    if (l != a.label) {
                        if (a.label >= 0) cc_acc_send(comps, a);
                        a.label = l; a.count = 0;
                        a.lo[0] = a.hi[0] = x; a.lo[1] = a.hi[1] = y; a.lo[2] = a.hi[2] = z;
                    }
                    a.count++;
                    a.lo[0] = min(a.lo[0], x); a.hi[0] = max(a.hi[0], x);
                    a.lo[1] = min(a.lo[1], y); a.hi[1] = max(a.hi[1], y);
                    a.lo[2] = min(a.lo[2], z); a.hi[2] = max(a.hi[2], z);
                }
                if (++x == D.x) { x = 0; if (++y == D.y) { y = 0; z++; } }
            }
        }
    }
    // the wave: one label among the lanes that hold any -> one accumulator
    __shared__ CcAcc waveAcc[kBlock / kWave];
    const int lane = (int)threadIdx.x % kWave, wave = (int)threadIdx.x / kWave;
    const bool have = a.label >= 0;
    const unsigned long long holders = __ballot(have);
    int first = -1;
    bool uniform = false;
    if (holders) {
        first = __shfl(a.label, (int)__ffsll((long long)holders) - 1);
        uniform = __ballot(have && a.label != first) == 0ull;
    }
    if (uniform) {
        unsigned cnt = have ? a.count : 0u;
        int lo[3], hi[3];
#pragma unroll
        for (int k = 0; k < 3; k++) { lo[k] = have ? a.lo[k] : 0x7fffffff; hi[k] = have ? a.hi[k] : -1; }
        for (int off = kWave / 2; off > 0; off >>= 1) {
            cnt += __shfl_xor(cnt, off);
#pragma unroll
            for (int k = 0; k < 3; k++) { lo[k] = min(lo[k], __shfl_xor(lo[k], off)); hi[k] = max(hi[k], __shfl_xor(hi[k], off)); }
        }
        if (lane == 0) {
            CcAcc w;
            w.label = first; w.count = cnt;
            for (int k = 0; k < 3; k++) { w.lo[k] = lo[k]; w.hi[k] = hi[k]; }
            waveAcc[wave] = w;
        }
    } else {
        if (have) cc_acc_send(comps, a);
        if (lane == 0) waveAcc[wave].label = -1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 0; w < kBlock / kWave; w++) {
            CcAcc m = waveAcc[w];
            if (m.label < 0) continue;
            for (int u = w + 1; u < kBlock / kWave; u++) {
                if (waveAcc[u].label != m.label) continue;
                m.count += waveAcc[u].count;
                for (int k = 0; k < 3; k++) { m.lo[k] = min(m.lo[k], waveAcc[u].lo[k]); m.hi[k] = max(m.hi[k], waveAcc[u].hi[k]); }
                waveAcc[u].label = -1;
            }
            cc_acc_send(comps, m);
        }
    }
}

// touches from the finished boxes: a component has a voxel with index 0 on axis a exactly when lo[a] == 0.
__global__ __launch_bounds__(kBlock) void k_cc_touches(CcComp* __restrict__ comps, unsigned count, CcDims D) {
    const unsigned i = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    if (i >= count) return;
    const int dims[3] = { D.x, D.y, D.z };
    int bits = 0;
    for (int a = 0; a < 3; a++) bits |= (comps[i].lo[a] == 0 ? 1 << a : 0) | (comps[i].hi[a] == dims[a] - 1 ? 8 << a : 0);
    comps[i].touches = bits;
}

// ---- selection and flip (rto_edit_components)
// The component to keep under ALL_BUT_LARGEST: most voxels, ties to the smaller number (= the smaller root).  One workgroup.
__global__ __launch_bounds__(kBlock) void k_cc_largest(const CcComp* __restrict__ comps, unsigned count, int* __restrict__ keep) {
    __shared__ long long bestV[kBlock];
    __shared__ unsigned bestI[kBlock];
    long long bv = -1; unsigned bi = kCcNone;
    for (unsigned i = threadIdx.x; i < count; i += kBlock) {
        const long long n = comps[i].voxels;
        if (n > bv) { bv = n; bi = i; }                    // ascending i: the first of equals stays
    }
    bestV[threadIdx.x] = bv; bestI[threadIdx.x] = bi;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const long long ov = bestV[threadIdx.x + s]; const unsigned oi = bestI[threadIdx.x + s];
            if (ov > bestV[threadIdx.x] || (ov == bestV[threadIdx.x] && oi < bestI[threadIdx.x])) { bestV[threadIdx.x] = ov; bestI[threadIdx.x] = oi; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) keep[0] = (int)bestI[0];
}

// One select byte per component.  at: the label of the voxel the CONTAINING forms name (-1: not in the set -> nothing selected).
__global__ __launch_bounds__(kBlock) void k_cc_select(const CcComp* __restrict__ comps, unsigned count, int select, long long arg,
                                                     const int* __restrict__ labels, const int* __restrict__ keep, uint8_t* __restrict__ sel) {
    const unsigned i = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    if (i >= count) return;
    bool s = false;
    if (select == RTO_SELECT_SMALLER_THAN) s = comps[i].voxels < arg;
    else if (select == RTO_SELECT_ALL_BUT_LARGEST) s = (int)i != keep[0];
    else if (select == RTO_SELECT_ENCLOSED) s = comps[i].touches == 0;
    else {
        const int at = labels[arg];
        s = at >= 0 && (select == RTO_SELECT_CONTAINING ? (int)i == at : (int)i != at);
    }
    sel[i] = s ? 1 : 0;
}

// Every voxel of a selected component takes newValue.  A thread owns 16 consecutive voxels (WIDE: n % 16 == 0, one 16-byte
// store when anything changed).  The count: block_add_count.
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void k_cc_flip(uint8_t* __restrict__ vox, const int* __restrict__ labels, const uint8_t* __restrict__ sel,
                                                   unsigned n, unsigned newValue, unsigned long long* __restrict__ changed) {
    const unsigned v0 = (blockIdx.x * (unsigned)kBlock + threadIdx.x) * (unsigned)kCcVec;
    int count = 0;
    if (v0 < n) {
        if (WIDE) {
            unsigned hit = 0u;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int4 l = *reinterpret_cast<const int4*>(labels + v0 + 4 * q);
                const int ls[4] = { l.x, l.y, l.z, l.w };
#pragma unroll
                for (int j = 0; j < 4; j++) hit |= (ls[j] >= 0 && sel[ls[j]] ? 1u : 0u) << (4 * q + j);
            }
            if (hit) {
                const uint4 w = *reinterpret_cast<const uint4*>(vox + v0);
                unsigned words[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
                for (int j = 0; j < kCcVec; j++) {
                    const unsigned sh = 8u * (unsigned)(j & 3);
                    if ((hit >> j) & 1u) words[j >> 2] = (words[j >> 2] & ~(0xffu << sh)) | (newValue << sh);
                }
                *reinterpret_cast<uint4*>(vox + v0) = make_uint4(words[0], words[1], words[2], words[3]);
                count = __popc(hit);
            }
        } else {
            for (int j = 0; j < kCcVec && v0 + (unsigned)j < n; j++) {
                const int l = labels[v0 + j];
                if (l >= 0 && sel[l]) { vox[v0 + j] = (uint8_t)newValue; count++; }
            }
        }
    }
    block_add_count(count, changed);
}

}  // namespace rto

namespace {

// The kCcTileX x kCcTileY x kCcTileZ tiles that cover a grid: what every kernel that runs one workgroup per tile is launched over.
struct CcTiles {
    int x, y, z;
    explicit CcTiles(const int dim[3])
        : x((dim[0] + rto::kCcTileX - 1) / rto::kCcTileX), y((dim[1] + rto::kCcTileY - 1) / rto::kCcTileY), z((dim[2] + rto::kCcTileZ - 1) / rto::kCcTileZ) {}
    size_t count() const { return (size_t)x * y * z; }
};

// One labelling, owned by whoever holds it (the context, or rto_edit_components for the length of the call).
struct CcResult {
    int* d_labels = nullptr;
    rto::CcComp* d_comps = nullptr;
    int64_t count = 0;
    int passes = 0;
    float ms[4] = { -1.f, -1.f, -1.f, -1.f };
    void release() { (void)hipFree(d_labels); (void)hipFree(d_comps); d_labels = nullptr; d_comps = nullptr; count = 0; }
};

int cc_check_args(rto_context* c, const char* who, int set, int connectivity) {
    const std::string w(who);
    if (set != RTO_SET_SOLID && set != RTO_SET_EMPTY) return fail(c, RTO_E_INVALID, w + ": unknown set");
    if (connectivity != RTO_CONN_FACE && connectivity != RTO_CONN_FULL) return fail(c, RTO_E_INVALID, w + ": connectivity must be 6 or 26");
    return resident_grid_check(c, who, ": labels are 32-bit");
}

// Labels the resident grid into `out` (arguments already checked).  On any error `out` is released and the context is as it was.
int cc_label(rto_context* c, const char* who, int set, int connectivity, CcResult& out) {
    using namespace rto;
    const CcDims D{ c->voxDim[0], c->voxDim[1], c->voxDim[2], (unsigned)grid_voxels(c) };
    RTO_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    RTO_HIP(c, hipStreamSynchronize(s));
    StreamEvents<5> events;
    RTO_HIP(c, events.create());
    struct OutGuard { CcResult* r; bool keep = false; ~OutGuard() { if (!keep) r->release(); } } og{ &out };

    const CcTiles T(c->voxDim);
    const unsigned chunks = (D.n + kCcChunk - 1) / kCcChunk;
    const unsigned voxBlocks = (D.n + kBlock - 1) / kBlock;
    const bool full = connectivity == RTO_CONN_FULL;
    const unsigned setValue = set == RTO_SET_SOLID ? 1u : 0u;

    RTO_HIP(c, hipMalloc(&out.d_labels, (size_t)D.n * sizeof(int)));
    BuildScratch scratch(s);
    unsigned* d_parent = nullptr; unsigned* d_blockCount = nullptr; unsigned* d_total = nullptr; int* d_flags = nullptr;
    RTO_HIP(c, scratch.alloc(&d_parent, (size_t)D.n));
    RTO_HIP(c, scratch.alloc(&d_blockCount, (size_t)chunks));
    RTO_HIP(c, scratch.alloc(&d_total, 1));
    RTO_HIP(c, scratch.alloc(&d_flags, (size_t)kCcMaxPasses));
    RTO_HIP(c, hipMemsetAsync(d_flags, 0, kCcMaxPasses * sizeof(int), s));

    // (1) tiles
    RTO_HIP(c, events.record(0, s));
    {
        const dim3 g((unsigned)T.count()), b(kBlock);
        const bool wide = D.x % kCcVec == 0;
        if (wide && full) hipLaunchKernelGGL((k_cc_local<true, true>), g, b, 0, s, c->d_vox, D, T.x, T.y, setValue, d_parent);
        else if (wide) hipLaunchKernelGGL((k_cc_local<true, false>), g, b, 0, s, c->d_vox, D, T.x, T.y, setValue, d_parent);
        else if (full) hipLaunchKernelGGL((k_cc_local<false, true>), g, b, 0, s, c->d_vox, D, T.x, T.y, setValue, d_parent);
        else hipLaunchKernelGGL((k_cc_local<false, false>), g, b, 0, s, c->d_vox, D, T.x, T.y, setValue, d_parent);
        RTO_HIP(c, hipGetLastError());
    }
    RTO_HIP(c, events.record(1, s));
    // (2) merge until a pass is clean: the first two passes go out together (the expected case: one merge, one clean check)
    int passes = 0;
    bool clean = false;
    int flags[kCcMaxPasses];
    while (!clean && passes < kCcMaxPasses) {
        const int launch = passes == 0 ? 2 : 1;
        for (int i = 0; i < launch; i++) {
            if (full) hipLaunchKernelGGL(k_cc_merge<true>, dim3(voxBlocks), dim3(kBlock), 0, s, d_parent, D, d_flags + passes + i);
            else hipLaunchKernelGGL(k_cc_merge<false>, dim3(voxBlocks), dim3(kBlock), 0, s, d_parent, D, d_flags + passes + i);
            RTO_HIP(c, hipGetLastError());
        }
        passes += launch;
        RTO_HIP(c, hipMemcpyAsync(flags, d_flags, (size_t)passes * sizeof(int), hipMemcpyDeviceToHost, s));
        RTO_HIP(c, hipStreamSynchronize(s));
        clean = flags[passes - 1] == 0;
    }
    if (!clean) return fail(c, RTO_E_INTERNAL, std::string(who) + ": merging did not settle in 32 passes");
    RTO_HIP(c, events.record(2, s));
    // (3) flatten, rank, label
    hipLaunchKernelGGL(k_cc_flatten, dim3(chunks), dim3(kBlock), 0, s, d_parent, D.n, d_blockCount);
    RTO_HIP(c, hipGetLastError());
    hipLaunchKernelGGL((k_scan_counts<kBlock, unsigned, unsigned>), dim3(1), dim3(kBlock), 0, s, d_blockCount, (int)chunks, d_blockCount, d_total);
    RTO_HIP(c, hipGetLastError());
    unsigned total = 0;
    RTO_HIP(c, hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, s));
    RTO_HIP(c, hipStreamSynchronize(s));
    RTO_HIP(c, hipMalloc(&out.d_comps, (size_t)(total ? total : 1) * sizeof(CcComp)));
    hipLaunchKernelGGL(k_cc_rank, dim3(chunks), dim3(kBlock), 0, s, d_parent, D.n, d_blockCount, out.d_labels, out.d_comps);
    RTO_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(k_cc_label, dim3(chunks), dim3(kBlock), 0, s, d_parent, D.n, out.d_labels);
    RTO_HIP(c, hipGetLastError());
    RTO_HIP(c, events.record(3, s));
    // (4) statistics
    if (total) {
        const unsigned statBlocks = (D.n + kBlock * kCcStatPerThread - 1) / (kBlock * kCcStatPerThread);
        hipLaunchKernelGGL(k_cc_stats, dim3(statBlocks), dim3(kBlock), 0, s, out.d_labels, D, out.d_comps);
        RTO_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(k_cc_touches, dim3((total + kBlock - 1) / kBlock), dim3(kBlock), 0, s, out.d_comps, total, D);
        RTO_HIP(c, hipGetLastError());
    }
    RTO_HIP(c, events.record(4, s));
    RTO_HIP(c, hipStreamSynchronize(s));
    for (int i = 0; i < 4; i++) RTO_HIP(c, events.elapsed(i, i + 1, &out.ms[i]));
    out.count = (int64_t)total;
    out.passes = passes;
    og.keep = true;
    return RTO_OK;
}

}  // namespace

extern "C" {

int rto_label_components(rto_context* c, int set, int connectivity, int64_t* count) {
    if (!c) return RTO_E_INVALID;
    const int rcArgs = cc_check_args(c, "rto_label_components", set, connectivity);
    if (rcArgs != RTO_OK) return rcArgs;
    CcResult r;
    const int rc = cc_label(c, "rto_label_components", set, connectivity, r);
    if (rc != RTO_OK) return rc;
    free_components(c);
    c->d_ccLabels = r.d_labels; c->d_ccComps = r.d_comps; c->ccCount = r.count; c->ccPasses = r.passes;
    c->ccSet = set; c->ccConn = connectivity;
    for (int i = 0; i < 4; i++) c->ccMs[i] = r.ms[i];
    if (count) *count = r.count;
    return RTO_OK;
}

int rto_download_components(rto_context* c, rto_component* out, int64_t capacity, int64_t* count) {
    if (!c) return RTO_E_INVALID;
    if (!c->d_ccLabels) return fail(c, RTO_E_INVALID, "rto_download_components: no labels are resident (not labelled yet, or the grid has changed since)");
    if (count) *count = c->ccCount;
    if (!out) return RTO_OK;
    return download_resident(c, "rto_download_components", out, capacity, c->d_ccComps, c->ccCount, sizeof(rto_component));
}

int rto_download_labels(rto_context* c, int32_t* out, int64_t capacity) {
    if (!c) return RTO_E_INVALID;
    if (!c->d_ccLabels) return fail(c, RTO_E_INVALID, "rto_download_labels: no labels are resident (not labelled yet, or the grid has changed since)");
    return download_resident(c, "rto_download_labels", out, capacity, c->d_ccLabels, grid_voxels(c), sizeof(int32_t));
}

int rto_labels_device(rto_context* c, int32_t** d_labels, rto_component** d_components, int64_t* count) {
    if (!c) return RTO_E_INVALID;
    if (!c->d_ccLabels) return fail(c, RTO_E_INVALID, "rto_labels_device: no labels are resident (not labelled yet, or the grid has changed since)");
    if (d_labels) *d_labels = c->d_ccLabels;
    if (d_components) *d_components = reinterpret_cast<rto_component*>(c->d_ccComps);
    if (count) *count = c->ccCount;
    return RTO_OK;
}

int rto_last_components_ms(const rto_context* c, float ms[4]) { return copy_last_ms(c, &rto_context::ccMs, ms); }

int rto_debug_components_passes(const rto_context* c, int* passes) {
    if (!c || !passes) return RTO_E_INVALID;
    *passes = c->ccPasses;
    return RTO_OK;
}

int rto_edit_components(rto_context* c, int set, int connectivity, int select, int64_t arg, int64_t* changed) {
    using namespace rto;
    if (!c) return RTO_E_INVALID;
    if (changed) *changed = 0;
    if (select < RTO_SELECT_SMALLER_THAN || select > RTO_SELECT_NOT_CONTAINING) return fail(c, RTO_E_INVALID, "rto_edit_components: unknown selection");
    const int rcArgs = cc_check_args(c, "rto_edit_components", set, connectivity);
    if (rcArgs != RTO_OK) return rcArgs;
    const int64_t nvox = grid_voxels(c);
    const bool byVoxel = select == RTO_SELECT_CONTAINING || select == RTO_SELECT_NOT_CONTAINING;
    if ((byVoxel || select == RTO_SELECT_SMALLER_THAN) && arg < 0) return fail(c, RTO_E_INVALID, "rto_edit_components: arg is negative");
    if (byVoxel && arg >= nvox) return fail(c, RTO_E_INVALID, "rto_edit_components: arg is not a voxel of the grid");
    CcResult r;
    const int rc = cc_label(c, "rto_edit_components", set, connectivity, r);
    if (rc != RTO_OK) return rc;
    struct Release { CcResult* r; ~Release() { r->release(); } } rel{ &r };
    if (r.count == 0) return RTO_OK;
    hipStream_t s = c->stream;
    unsigned long long count = 0;
    {
        BuildScratch scratch(s);
        uint8_t* d_sel = nullptr; int* d_keep = nullptr;
        ChangedCount d_count;
        RTO_HIP(c, scratch.alloc(&d_sel, (size_t)r.count));
        RTO_HIP(c, scratch.alloc(&d_keep, 1));
        RTO_HIP(c, d_count.alloc(scratch));
        RTO_HIP(c, d_count.clear(s));
        if (select == RTO_SELECT_ALL_BUT_LARGEST) {
            hipLaunchKernelGGL(k_cc_largest, dim3(1), dim3(kBlock), 0, s, r.d_comps, (unsigned)r.count, d_keep);
            RTO_HIP(c, hipGetLastError());
        }
        hipLaunchKernelGGL(k_cc_select, dim3((unsigned)((r.count + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, r.d_comps, (unsigned)r.count, select,
                           (long long)(byVoxel || select == RTO_SELECT_SMALLER_THAN ? arg : 0), r.d_labels, d_keep, d_sel);
        RTO_HIP(c, hipGetLastError());
        const unsigned n = (unsigned)nvox;
        const unsigned blocks = (unsigned)(((nvox + kCcVec - 1) / kCcVec + kBlock - 1) / kBlock);
        const unsigned newValue = set == RTO_SET_SOLID ? 0u : 1u;
        if (n % kCcVec == 0) hipLaunchKernelGGL(k_cc_flip<true>, dim3(blocks), dim3(kBlock), 0, s, c->d_vox, r.d_labels, d_sel, n, newValue, d_count.d);
        else hipLaunchKernelGGL(k_cc_flip<false>, dim3(blocks), dim3(kBlock), 0, s, c->d_vox, r.d_labels, d_sel, n, newValue, d_count.d);
        RTO_HIP(c, hipGetLastError());
        RTO_HIP(c, d_count.read(s, &count));
    }
    if (changed) *changed = (int64_t)count;
    if (count == 0) return RTO_OK;           // nothing is dropped: rebuild_from_resident_grid's comment

    return rebuild_from_resident_grid(c, c->d_triOffset != nullptr, nullptr, nullptr);
}

}  // extern "C"
