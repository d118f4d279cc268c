// rto_geodesic.inc -- geodesic distance fields of the resident grid (include/rto_hip.h, rto_geodesic_field / rto_geodesic_paths /
// rto_edit_geodesic): the length of the shortest path that stays inside a medium (the EMPTY or the FILLED voxels) from a set of
// seed voxels to every voxel, kept resident as one int32 per voxel; the paths themselves, read back out of the field; and the
// flood edit that is a threshold on it, with the voxel edits' rebuild.  Included at the end of rto_api.hip, after rto_distance.inc.
//
// Rule (DESIGN.md section 20).  Voxel (i, j, k) has linear index v = i + dimX (j + dimY k).  A move joins two voxels of the medium
// that are neighbours under the connectivity: weight 1 for the 6 face moves of RTO_CONN_FACE; 3, 4, 5 for the 26 moves of
// RTO_CONN_FULL that change 1, 2, 3 coordinates.  g[v] = the smallest total weight of a path of moves from a seed of the medium to
// v; kDtNone outside the medium, out of reach of every seed, or beyond the limit.
//
// The field is the fixed point of g[v] = min(g[v], g[u] + w(u, v)) over the moves, reached by chaotic relaxation over tiles:
// (1) k_geo_fill / k_geo_seeds write kDtNone everywhere, 0 at the seeds of the medium, and mark the tiles that hold a seed or a
// neighbour of one;
// (2) k_geo_relax, one workgroup per marked 32 x 8 x 8 tile, loads the tile's values with a one-voxel halo into LDS, relaxes there
// until a sweep lowers nothing, writes back what it lowered and marks for the next launch every tile that holds a neighbour of a
// voxel it lowered; the host launches it until a launch finds no tile marked; (3) k_dt_summary (rto_distance.inc) reduces the
// volume.  Correctness without any synchronisation inside a launch: values only decrease; every value ever stored is the length
// of a real path, hence an upper bound of the answer; a 32-bit value is stored whole; so a halo value read while its owner lowers
// it is an older or a newer upper bound, and the owner marks the reader for the next launch, where the reader sees it.  A launch
// with no tile marked has therefore seen the unique fixed point.  No workgroup waits for another.

namespace rto {

constexpr int kGeoHaloX = kCcTileX + 2, kGeoHaloY = kCcTileY + 2, kGeoHaloZ = kCcTileZ + 2;   // 34 x 10 x 10
constexpr int kGeoHaloVox = kGeoHaloX * kGeoHaloY * kGeoHaloZ;                                // 3400 values, 13.3 KiB of LDS

__device__ __forceinline__ int geo_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void geo_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- init.  A thread owns 16 consecutive values.
__global__ __launch_bounds__(kBlock) void k_geo_fill(int* __restrict__ g, unsigned n) {
    const unsigned v0 = (blockIdx.x * (unsigned)kBlock + threadIdx.x) * (unsigned)kCcVec;
    if (v0 >= n) return;
    if (v0 + kCcVec <= n) {                                 // v0 is a multiple of 16 values: 16-byte stores are aligned
#pragma unroll
        for (int q = 0; q < 4; q++) *reinterpret_cast<int4*>(g + v0 + 4 * q) = make_int4(kDtNone, kDtNone, kDtNone, kDtNone);
    } else {
        for (int j = 0; j < kCcVec && v0 + (unsigned)j < n; j++) g[v0 + j] = kDtNone;
    }
}

// One thread per seed (all already known to be voxels of the grid): it holds 0 when it lies in the medium.  Its own tile and the
// tiles of its 26 neighbours are marked: a seed's 0 is lowered by no tile, so nobody else would tell the tile next door.
// Duplicates store the same words.
__global__ __launch_bounds__(kBlock) void k_geo_seeds(const uint8_t* __restrict__ vox, CcDims D, int tilesX, int tilesY, unsigned setValue,
                                                     const long long* __restrict__ seeds, unsigned count, int* __restrict__ g,
                                                     int* __restrict__ active) {
    const unsigned i = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    if (i >= count) return;
    const unsigned v = (unsigned)seeds[i];
    const int x = (int)(v % (unsigned)D.x), y = (int)((v / (unsigned)D.x) % (unsigned)D.y), z = (int)(v / ((unsigned)D.x * (unsigned)D.y));
    for (int dz = -1; dz <= 1; dz++)
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                const int nx = x + dx, ny = y + dy, nz = z + dz;
                if (nx < 0 || nx >= D.x || ny < 0 || ny >= D.y || nz < 0 || nz >= D.z) continue;
                geo_store(&active[(nz / kCcTileZ * tilesY + ny / kCcTileY) * tilesX + nx / kCcTileX], 1);
            }
    if ((unsigned)vox[v] == setValue) geo_store(&g[v], 0);
}

// ---- relaxation.  Workgroup b owns tile b and runs only when cur[b] is set (it clears the mark: the array is the next launch's
// `next`).  Thread t owns the 8 voxels [8 (t % 4), 8 (t % 4) + 8) of tile row t / 4, as in k_cc_local.  G: the tile's values with
// a one-voxel halo, kDtNone outside the grid.  Only voxels of the medium ever hold a finite value, so the halo needs no medium
// bits: a finite halo value is a voxel of the medium.  The sweeps run in place: a value read while its owner lowers it is an older
// or a newer upper bound.  Unsigned arithmetic: kDtNone + w stays above every finite value, so no test for kDtNone is needed.
// counters[0]: tiles run by this launch.
template <bool WIDE, bool FULL>
__global__ __launch_bounds__(kBlock) void k_geo_relax(const uint8_t* __restrict__ vox, CcDims D, int tilesX, int tilesY, int tilesZ,
                                                     unsigned setValue, unsigned limit, int* __restrict__ g, int* __restrict__ cur,
                                                     int* __restrict__ next, unsigned* __restrict__ counters) {
    __shared__ unsigned G[kGeoHaloVox];
    __shared__ unsigned marks;                                      // bit (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1): that neighbour tile is to run next
    __shared__ int on;
    const int t = (int)threadIdx.x;
    const int bid = (int)blockIdx.x;
    if (t == 0) { on = geo_load(&cur[bid]); marks = 0u; }
    __syncthreads();
    if (!on) return;                                                // the whole workgroup leaves: `on` is one LDS word
    if (t == 0) { geo_store(&cur[bid], 0); atomicAdd(counters, 1u); }
    const int tx = bid % tilesX, ty = (bid / tilesX) % tilesY, tz = bid / (tilesX * tilesY);
    const int x0 = tx * kCcTileX, y0 = ty * kCcTileY, z0 = tz * kCcTileZ;
    for (int i = t; i < kGeoHaloVox; i += kBlock) {                 // 14 rounds
        const int hx = i % kGeoHaloX, hy = (i / kGeoHaloX) % kGeoHaloY, hz = i / (kGeoHaloX * kGeoHaloY);
        const int gx = x0 + hx - 1, gy = y0 + hy - 1, gz = z0 + hz - 1;
        unsigned val = (unsigned)kDtNone;
        if (gx >= 0 && gx < D.x && gy >= 0 && gy < D.y && gz >= 0 && gz < D.z)
            val = (unsigned)geo_load(&g[((size_t)gz * D.y + gy) * (size_t)D.x + gx]);
        G[i] = val;
    }
    const int row = t / (kCcTileX / kCcSeg), seg = t % (kCcTileX / kCcSeg);
    const int lx0 = seg * kCcSeg, ly = row % kCcTileY, lz = row / kCcTileY;
    const int gx0 = x0 + lx0, gy = y0 + ly, gz = z0 + lz;
    const bool rowIn = gy < D.y && gz < D.z;
    const size_t rowBase = ((size_t)gz * D.y + gy) * (size_t)D.x;
    unsigned in = 0u;                                               // bit j: voxel gx0 + j belongs to the medium
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
    const int base = ((lz + 1) * kGeoHaloY + (ly + 1)) * kGeoHaloX + lx0 + 1;      // the thread's first voxel in G
    __syncthreads();
    unsigned orig[kCcSeg];
#pragma unroll
    for (int j = 0; j < kCcSeg; j++) orig[j] = G[base + j];
    // No barrier between the sweeps' reads and writes: every word of G only decreases and every value in it is a path length.  The
    // barrier of __syncthreads_or separates the rounds; a round that lowers nothing has read a fixed point.
    for (;;) {
        int lowered = 0;
        if (in) {
            for (int s = 0; s < 2 * kCcSeg; s++) {                  // along the run and back: a value crosses the run in one round
                const int j = s < kCcSeg ? s : 2 * kCcSeg - 1 - s;
                if (!((in >> j) & 1u)) continue;
                const int at = base + j;
                const unsigned was = G[at];
                unsigned best = was;
                if (FULL) {
#pragma unroll
                    for (int dz = -1; dz <= 1; dz++)
#pragma unroll
                        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                            for (int dx = -1; dx <= 1; dx++) {
                                if (dx == 0 && dy == 0 && dz == 0) continue;
                                const unsigned w = 2u + (unsigned)((dx != 0) + (dy != 0) + (dz != 0));
                                best = min(best, G[at + (dz * kGeoHaloY + dy) * kGeoHaloX + dx] + w);
                            }
                } else {
                    best = min(best, G[at - 1] + 1u);
                    best = min(best, G[at + 1] + 1u);
                    best = min(best, G[at - kGeoHaloX] + 1u);
                    best = min(best, G[at + kGeoHaloX] + 1u);
                    best = min(best, G[at - kGeoHaloX * kGeoHaloY] + 1u);
                    best = min(best, G[at + kGeoHaloX * kGeoHaloY] + 1u);
                }
                if (best < was && best <= limit) { G[at] = best; lowered = 1; }
            }
        }
        if (!__syncthreads_or(lowered)) break;
    }
    // write back what was lowered; which neighbour tiles hold a neighbour of a lowered voxel
    unsigned mine = 0u;
    if (in) {
#pragma unroll
        for (int j = 0; j < kCcSeg; j++) {
            const unsigned now = G[base + j];
            if (now >= orig[j]) continue;
            geo_store(&g[rowBase + gx0 + j], (int)now);
            const int lx = lx0 + j;
            // the neighbours at offset -1 / +1 along an axis lie in the tile before / after when the voxel is on that face
            const int ex = lx == 0 ? -1 : (lx == kCcTileX - 1 ? 1 : 0), ey = ly == 0 ? -1 : (ly == kCcTileY - 1 ? 1 : 0),
                      ez = lz == 0 ? -1 : (lz == kCcTileZ - 1 ? 1 : 0);
            if (FULL) {
#pragma unroll
                for (int az = 0; az < 2; az++)
#pragma unroll
                    for (int ay = 0; ay < 2; ay++)
#pragma unroll
                        for (int ax = 0; ax < 2; ax++) {
                            const int mx = ax ? ex : 0, my = ay ? ey : 0, mz = az ? ez : 0;
                            if (mx || my || mz) mine |= 1u << ((mz + 1) * 9 + (my + 1) * 3 + (mx + 1));
                        }
            } else {
                if (ex) mine |= 1u << (13 + ex);
                if (ey) mine |= 1u << (13 + 3 * ey);
                if (ez) mine |= 1u << (13 + 9 * ez);
            }
        }
    }
    if (mine) atomicOr(&marks, mine);
    __syncthreads();
    if (t < 27 && t != 13 && ((marks >> t) & 1u)) {
        const int nx = tx + t % 3 - 1, ny = ty + (t / 3) % 3 - 1, nz = tz + t / 9 - 1;
        if (nx >= 0 && nx < tilesX && ny >= 0 && ny < tilesY && nz >= 0 && nz < tilesZ) geo_store(&next[(nz * tilesY + ny) * tilesX + nx], 1);
    }
}

// ---- paths.  One thread per target walks downhill in the resident field: from p the next voxel is the smallest linear index
// among the neighbours u with g[u] finite and g[u] + w(u, p) == g[p] (the loops run in ascending index order, so the first match
// is the smallest).  g falls by at least 1 per step, so the walk ends.  row: maxLen voxels per target, -1 behind the path.
template <bool FULL>
__global__ __launch_bounds__(kBlock) void k_geo_paths(const int* __restrict__ g, CcDims D, const long long* __restrict__ targets, unsigned count,
                                                     long long maxLen, long long* __restrict__ rows, long long* __restrict__ lens) {
    const unsigned i = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    if (i >= count) return;
    long long* row = rows ? rows + (size_t)i * (size_t)maxLen : nullptr;
    unsigned p = (unsigned)targets[i];
    int gp = g[p];
    long long len = 0;
    if (gp == kDtNone) len = -1;
    else {
        for (;;) {
            if (len < maxLen) row[len] = (long long)p;
            len++;
            if (gp == 0) break;
            const int x = (int)(p % (unsigned)D.x), y = (int)((p / (unsigned)D.x) % (unsigned)D.y), z = (int)(p / ((unsigned)D.x * (unsigned)D.y));
            bool found = false;
            for (int dz = -1; dz <= 1 && !found; dz++)
                for (int dy = -1; dy <= 1 && !found; dy++)
                    for (int dx = -1; dx <= 1 && !found; dx++) {
                        const int c = (dx != 0) + (dy != 0) + (dz != 0);
                        if (c == 0 || (!FULL && c != 1)) continue;
                        const int nx = x + dx, ny = y + dy, nz = z + dz;
                        if (nx < 0 || nx >= D.x || ny < 0 || ny >= D.y || nz < 0 || nz >= D.z) continue;
                        const unsigned u = (unsigned)(((size_t)nz * D.y + ny) * (size_t)D.x + nx);
                        const int gu = g[u];
                        const int w = FULL ? 2 + c : 1;
                        if (gu != kDtNone && gu + w == gp) { p = u; gp = gu; found = true; }
                    }
            if (!found) break;                                      // not a field of this grid: cannot happen with a resident one
        }
    }
    for (long long k = len < 0 ? 0 : len; k < maxLen; k++) row[k] = -1;
    lens[i] = len;
}

}  // namespace rto

namespace {

struct GeoRun {
    float ms[2] = { -1.f, -1.f };      // init, relaxation
    int64_t passes = 0;                // relaxation launches up to and including the first that found no tile marked
    int64_t tilesRun = 0;              // tiles run, summed over those launches
};

// medium, connectivity, seeds, limit, then the grid: rto_label_components' order.  limitOut: the largest value kept.
int geo_check_args(rto_context* c, const char* who, int medium, int connectivity, const int64_t* seeds, int64_t n, int64_t limit,
                   unsigned* limitOut) {
    const std::string w(who);
    if (medium != RTO_SET_SOLID && medium != RTO_SET_EMPTY) return fail(c, RTO_E_INVALID, w + ": unknown medium");
    if (connectivity != RTO_CONN_FACE && connectivity != RTO_CONN_FULL) return fail(c, RTO_E_INVALID, w + ": connectivity must be 6 or 26");
    if (n < 1) return fail(c, RTO_E_INVALID, w + ": n is below 1");
    if (!seeds) return fail(c, RTO_E_INVALID, w + ": seeds is NULL");
    if (limit < 0) return fail(c, RTO_E_INVALID, w + ": limit is negative");
    const int rcGrid = resident_grid_check(c, who, ": the field is 32-bit");
    if (rcGrid != RTO_OK) return rcGrid;
    const int64_t wmax = connectivity == RTO_CONN_FULL ? 5 : 1;
    if (wmax * (grid_voxels(c) - 1) >= 0x7fffffffll) return fail(c, RTO_E_UNSUPPORTED, w + ": the longest possible path does not fit the 32-bit field");
    const int rcSeeds = voxel_list_check(c, who, "a seed", seeds, n);
    if (rcSeeds != RTO_OK) return rcSeeds;
    *limitOut = limit >= 0x7fffffffll ? (unsigned)rto::kDtNone - 1u : (unsigned)limit;
    return RTO_OK;
}

// The field into d_out (one int32 per voxel; arguments already checked).  The context is not touched, but for the stream.
int geo_relax(rto_context* c, const char* who, int medium, int connectivity, const int64_t* seeds, int64_t n, unsigned limit, int* d_out,
              GeoRun& run) {
    using namespace rto;
    const CcDims D{ c->voxDim[0], c->voxDim[1], c->voxDim[2], (unsigned)grid_voxels(c) };
    hipStream_t s = c->stream;
    StreamEvents<3> events;
    RTO_HIP(c, events.create());
    const CcTiles T(c->voxDim);
    const size_t tiles = T.count();
    const unsigned setValue = medium == RTO_SET_SOLID ? 1u : 0u;
    const bool full = connectivity == RTO_CONN_FULL, wide = D.x % kCcVec == 0;
    BuildScratch scratch(s);
    VoxelList d_seeds; int* d_active = nullptr; unsigned* d_counters = nullptr;
    RTO_HIP(c, d_seeds.upload(scratch, seeds, n, s));
    RTO_HIP(c, scratch.alloc(&d_active, 2 * tiles));
    RTO_HIP(c, scratch.alloc(&d_counters, (size_t)kMaxLook));
    RTO_HIP(c, events.record(0, s));
    RTO_HIP(c, hipMemsetAsync(d_active, 0, 2 * tiles * sizeof(int), s));
    hipLaunchKernelGGL(k_geo_fill, dim3((unsigned)((((int64_t)D.n + kCcVec - 1) / kCcVec + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, d_out, D.n);
    RTO_HIP(c, hipGetLastError());
    const int rcSeeds = d_seeds.in_parts(c, [&](const long long* part, unsigned count) {
        hipLaunchKernelGGL(k_geo_seeds, dim3((count + kBlock - 1) / kBlock), dim3(kBlock), 0, s, c->d_vox, D, T.x, T.y, setValue, part, count, d_out, d_active);
    });
    if (rcSeeds != RTO_OK) return rcSeeds;
    RTO_HIP(c, events.record(1, s));
    // launches until one finds no tile marked (its word: the tiles it ran); `look` of them between two looks (look_at_passes)
    const int64_t cap = (int64_t)D.n + 2;
    const int look = std::max(1, std::min(c->geoLook, kMaxLook));
    int64_t passes = 0, tilesRun = 0;
    bool settled = false;
    while (!settled && passes < cap) {
        const int launch = (int)std::min<int64_t>(look, cap - passes);
        const int rcLook = look_at_passes(c, d_counters, launch, [&](int i, unsigned* ran) -> int {
            int* cur = d_active + (size_t)((passes + i) & 1) * tiles;
            int* next = d_active + (size_t)((passes + i + 1) & 1) * tiles;
            const dim3 gr((unsigned)tiles), b(kBlock);
            if (wide && full) hipLaunchKernelGGL((k_geo_relax<true, true>), gr, b, 0, s, c->d_vox, D, T.x, T.y, T.z, setValue, limit, d_out, cur, next, ran);
            else if (wide) hipLaunchKernelGGL((k_geo_relax<true, false>), gr, b, 0, s, c->d_vox, D, T.x, T.y, T.z, setValue, limit, d_out, cur, next, ran);
            else if (full) hipLaunchKernelGGL((k_geo_relax<false, true>), gr, b, 0, s, c->d_vox, D, T.x, T.y, T.z, setValue, limit, d_out, cur, next, ran);
            else hipLaunchKernelGGL((k_geo_relax<false, false>), gr, b, 0, s, c->d_vox, D, T.x, T.y, T.z, setValue, limit, d_out, cur, next, ran);
            RTO_HIP(c, hipGetLastError());
            return RTO_OK;
        }, passes, tilesRun, settled);
        if (rcLook != RTO_OK) return rcLook;
    }
    if (!settled) return fail(c, RTO_E_INTERNAL, std::string(who) + ": the relaxation did not settle within voxels + 2 passes");
    RTO_HIP(c, events.record(2, s));
    RTO_HIP(c, hipStreamSynchronize(s));
    for (int i = 0; i < 2; i++) RTO_HIP(c, events.elapsed(i, i + 1, &run.ms[i]));
    run.passes = passes;
    run.tilesRun = tilesRun;
    return RTO_OK;
}

// A grid edit that is a flip by a field of the call's own (rto_edit_geodesic, and rto_edit_skeleton in rto_skeleton.inc; arguments
// already checked): compute(d_field) makes the field in the call's scratch, flip(d_field, nvox, blocks, d_count) enqueues the
// kernel that flips the voxels the field selects, one thread per kCcVec voxels, and counts them; then the voxel edits' rebuild.
// editMs: field and flip, octree rebuild, triangle rebuild.
template <class Compute, class Flip>
int edit_by_field(rto_context* c, float (&editMs)[3], int64_t* changed, Compute compute, Flip flip) {
    RTO_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    RTO_HIP(c, hipStreamSynchronize(s));
    const unsigned nvox = (unsigned)grid_voxels(c);
    float ms[3] = { -1.f, -1.f, -1.f };
    unsigned long long count = 0;
    {
        StreamEvents<2> events;
        RTO_HIP(c, events.create());
        BuildScratch scratch(s);
        int* d_field = nullptr;
        ChangedCount d_count;
        RTO_HIP(c, scratch.alloc(&d_field, (size_t)nvox));
        RTO_HIP(c, d_count.alloc(scratch));
        RTO_HIP(c, events.record(0, s));
        const int rc = compute(d_field);
        if (rc != RTO_OK) return rc;                                    // the grid has not been written yet
        RTO_HIP(c, d_count.clear(s));
        flip(d_field, nvox, (unsigned)((((int64_t)nvox + rto::kCcVec - 1) / rto::kCcVec + kBlock - 1) / kBlock), d_count.d);
        RTO_HIP(c, hipGetLastError());
        RTO_HIP(c, events.record(1, s));
        RTO_HIP(c, d_count.read(s, &count));
        RTO_HIP(c, events.elapsed(0, 1, &ms[0]));
    }
    for (int i = 0; i < 3; i++) editMs[i] = ms[i];
    if (changed) *changed = (int64_t)count;
    if (count == 0) return RTO_OK;           // nothing is dropped: rebuild_from_resident_grid's comment

    return rebuild_from_resident_grid(c, c->d_triOffset != nullptr, &editMs[1], &editMs[2]);
}


}  // namespace

extern "C" {

int rto_geodesic_field(rto_context* c, int medium, int connectivity, const int64_t* seeds, int64_t n, int64_t limit, rto_geo_summary* summary) {
    using namespace rto;
    if (!c) return RTO_E_INVALID;
    unsigned lim = 0u;
    const int rcArgs = geo_check_args(c, "rto_geodesic_field", medium, connectivity, seeds, n, limit, &lim);
    if (rcArgs != RTO_OK) return rcArgs;
    FieldDraft draft(c, kFieldGeodesic);
    const int rcDraft = draft.begin();
    if (rcDraft != RTO_OK) return rcDraft;
    GeoRun run;
    const int rc = geo_relax(c, "rto_geodesic_field", medium, connectivity, seeds, n, lim, draft.d, run);
    if (rc != RTO_OK) return rc;
    float summaryMs = -1.f;
    if (summary) {
        DtSummary sum;
        const int rcSum = dt_summary(c, draft.d, (unsigned)grid_voxels(c), sum);
        if (rcSum != RTO_OK) return rcSum;
        summaryMs = sum.ms;
        summary->reached = sum.finite;
        summary->max_g = sum.max;
        summary->argmax = sum.argmax;
        summary->reserved = 0;
    }
    draft.publish();
    c->geoMedium = medium; c->geoConn = connectivity;
    c->geoPasses = run.passes; c->geoTilesRun = run.tilesRun;
    c->geoMs[0] = run.ms[0]; c->geoMs[1] = run.ms[1]; c->geoMs[2] = summaryMs;
    return RTO_OK;
}

int rto_download_geodesic(rto_context* c, int32_t* out, int64_t capacity) { return download_field(c, "rto_download_geodesic", kFieldGeodesic, out, capacity); }

int rto_geodesic_device(rto_context* c, int32_t** d_g) { return field_device(c, "rto_geodesic_device", kFieldGeodesic, d_g); }

int rto_geodesic_paths(rto_context* c, const int64_t* targets, int64_t n, int64_t max_len, int64_t* out_voxels, int64_t* out_len) {
    using namespace rto;
    if (!c) return RTO_E_INVALID;
    if (n < 1) return fail(c, RTO_E_INVALID, "rto_geodesic_paths: n is below 1");
    if (!targets || !out_len) return fail(c, RTO_E_INVALID, "rto_geodesic_paths: targets or out_len is NULL");
    if (max_len < 0) return fail(c, RTO_E_INVALID, "rto_geodesic_paths: max_len is negative");
    if (max_len > 0 && !out_voxels) return fail(c, RTO_E_INVALID, "rto_geodesic_paths: out_voxels is NULL");
    const int rcField = resident_field_check(c, "rto_geodesic_paths", kFieldGeodesic);
    if (rcField != RTO_OK) return rcField;
    const int rcTargets = voxel_list_check(c, "rto_geodesic_paths", "a target", targets, n);
    if (rcTargets != RTO_OK) return rcTargets;
    if (n > 0x40000000ll || (max_len > 0 && n > (int64_t)(0x7fffffffffffffffll / 8) / max_len))
        return fail(c, RTO_E_INVALID, "rto_geodesic_paths: n x max_len is beyond what one call serves");
    const CcDims D{ c->voxDim[0], c->voxDim[1], c->voxDim[2], (unsigned)grid_voxels(c) };
    RTO_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    RTO_HIP(c, hipStreamSynchronize(s));
    BuildScratch scratch(s);
    long long* d_targets = nullptr; long long* d_rows = nullptr; long long* d_lens = nullptr;
    RTO_HIP(c, scratch.alloc(&d_targets, (size_t)n));
    RTO_HIP(c, scratch.alloc(&d_lens, (size_t)n));
    if (max_len > 0) RTO_HIP(c, scratch.alloc(&d_rows, (size_t)n * (size_t)max_len));
    RTO_HIP(c, hipMemcpyAsync(d_targets, targets, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, s));
    const dim3 gr((unsigned)((n + kBlock - 1) / kBlock)), b(kBlock);
    if (c->geoConn == RTO_CONN_FULL) hipLaunchKernelGGL(k_geo_paths<true>, gr, b, 0, s, c->d_field[kFieldGeodesic], D, d_targets, (unsigned)n, (long long)max_len, d_rows, d_lens);
    else hipLaunchKernelGGL(k_geo_paths<false>, gr, b, 0, s, c->d_field[kFieldGeodesic], D, d_targets, (unsigned)n, (long long)max_len, d_rows, d_lens);
    RTO_HIP(c, hipGetLastError());
    RTO_HIP(c, hipMemcpyAsync(out_len, d_lens, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (max_len > 0) RTO_HIP(c, hipMemcpyAsync(out_voxels, d_rows, (size_t)n * (size_t)max_len * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    RTO_HIP(c, hipStreamSynchronize(s));
    return RTO_OK;
}

int rto_last_geodesic_ms(const rto_context* c, float ms[3]) { return copy_last_ms(c, &rto_context::geoMs, ms); }

int rto_debug_geodesic_passes(const rto_context* c, int64_t* passes, int64_t* tiles_run) {
    if (!c || !passes) return RTO_E_INVALID;
    *passes = c->geoPasses;
    if (tiles_run) *tiles_run = c->geoTilesRun;
    return RTO_OK;
}

int rto_debug_set_geodesic_look(rto_context* c, int passes_per_look) {
    if (!c) return RTO_E_INVALID;
    if (passes_per_look < 1 || passes_per_look > kMaxLook) return fail(c, RTO_E_INVALID, "rto_debug_set_geodesic_look: 1 to 64 passes per look");
    c->geoLook = passes_per_look;
    return RTO_OK;
}

int rto_edit_geodesic(rto_context* c, int medium, int connectivity, const int64_t* seeds, int64_t n, int64_t limit, int64_t* changed) {
    using namespace rto;
    if (!c) return RTO_E_INVALID;
    if (changed) *changed = 0;
    unsigned lim = 0u;
    const int rcArgs = geo_check_args(c, "rto_edit_geodesic", medium, connectivity, seeds, n, limit, &lim);
    if (rcArgs != RTO_OK) return rcArgs;
    const unsigned from = medium == RTO_SET_SOLID ? 1u : 0u, to = medium == RTO_SET_SOLID ? 0u : 1u;
    return edit_by_field(
        c, c->geoEditMs, changed,
        [&](int* d_field) {
            GeoRun run;
            return geo_relax(c, "rto_edit_geodesic", medium, connectivity, seeds, n, lim, d_field, run);
        },
        // only voxels of the medium hold a finite value, so the threshold of rto_edit_morphology is the flood's flip as well
        [&](const int* d_field, unsigned nvox, unsigned blocks, unsigned long long* d_count) {
            if (nvox % kCcVec == 0) hipLaunchKernelGGL(k_morph_flip<true>, dim3(blocks), dim3(kBlock), 0, c->stream, c->d_vox, d_field, (const uint8_t*)nullptr, nvox, from, to, d_count);
            else hipLaunchKernelGGL(k_morph_flip<false>, dim3(blocks), dim3(kBlock), 0, c->stream, c->d_vox, d_field, (const uint8_t*)nullptr, nvox, from, to, d_count);
        });
}

int rto_last_geodesic_edit_ms(const rto_context* c, float ms[3]) { return copy_last_ms(c, &rto_context::geoEditMs, ms); }

}  // extern "C"
