// rto_parts.inc -- part segmentation of the resident grid (include/rto_hip.h, rto_segment_parts / rto_edit_parts): the watershed of
// the squared distance field of a set, basins merged across wide necks, the label volume and the part and neck tables kept resident,
// and the edit that cuts the grid at the necks.  Included at the end of rto_api.hip, after rto_components.inc and rto_distance.inc,
// whose kernels it reuses unchanged.
//
// Rule (DESIGN.md section 26).  h[v] = the uncapped d2 from v to the voxels outside the set S (0 off S, kDtNone on S when S is the
// whole grid); key(v) = (h[v], -v), a strict total order; up(v) = the neighbour in S with the largest key if that exceeds key(v),
// else v, a peak; a basin is what ends at one peak, numbered in ascending order of the peak.  Basin edges carry the highest pass
// between two basins; the host merges them in descending order of pass height under the ratio test and numbers the clusters in
// ascending order of their smallest voxel.
//
// Phases: (1) dt_transform of the other set into h; (2) k_part_ascend writes parent = up, k_part_flatten doubles the pointers until
// a launch changes nothing; (3) k_cc_flatten / k_scan_counts / k_cc_rank / k_cc_label number the peaks and write the basin volume,
// k_cc_stats / k_cc_touches fill the basin table, k_part_basin_min adds the smallest voxel and the peak height; (4) k_part_edges
// folds every crossing pair into an open-addressing table, k_part_compact lists its occupied slots; (5) the host merges and
// k_part_relabel maps basin numbers to part numbers.  Every dependence between workgroups crosses a kernel boundary.
//
// Why stale reads are harmless in (2): the forest is the ascent forest, keys strictly ascend along every chain, and a launch only
// ever replaces parent[v] by an ancestor of v (an ancestor's parent is an ancestor).  Whatever mix of old and new values a thread
// reads under relaxed agent-scope loads is therefore an ancestor, no cycle can form, and a launch that raises no flag has written
// nothing, so it has read one consistent forest in which every parent is a fixed point.

namespace rto {

constexpr int kPartMaxRounds = 32;                       // pointer-doubling launches: covers chains of 2^32 voxels
constexpr int kPartRoundsPerLook = 4;                    // launches between two looks at the flags
constexpr int kPartMaxGrowths = 8;                       // doublings of the edge table
constexpr unsigned long long kPartEmpty = ~0ull;         // no basin pair: A < 2^31

struct PartEdge { unsigned long long key, val, pairs; }; // (A << 32 | B), (s << 32 | ~at), voxel pairs
static_assert(sizeof(PartEdge) == 24, "three words a basin edge");

// ---- phase 2: the ascent.  One workgroup per 32 x 8 x 8 tile, thread t the column (t % 32, t / 32) of it, one voxel per z step;
// h is read straight from global memory: the 6 or 26 neighbours of a wave's row are three rows that the rows before and after load
// again, so all but the first touch hits L1 / L2, and the kernel keeps no LDS and no barrier.
template <bool FULL>
__global__ __launch_bounds__(kBlock) void k_part_ascend(const int* __restrict__ h, CcDims D, int tilesX, int tilesY, unsigned* __restrict__ parent) {
    const int t = (int)threadIdx.x;
    const int bid = (int)blockIdx.x;
    const int x = (bid % tilesX) * kCcTileX + t % kCcTileX, y = ((bid / tilesX) % tilesY) * kCcTileY + t / kCcTileX;
    const int z0 = (bid / (tilesX * tilesY)) * kCcTileZ;
    if (x >= D.x || y >= D.y) return;
    const unsigned strideY = (unsigned)D.x, strideZ = (unsigned)D.x * (unsigned)D.y;
    for (int lz = 0; lz < kCcTileZ; lz++) {
        const int z = z0 + lz;
        if (z >= D.z) break;
        const unsigned v = (unsigned)z * strideZ + (unsigned)y * strideY + (unsigned)x;
        const int hv = h[v];
        unsigned best = kCcNone;
        if (hv > 0) {
            int bh = hv;
            best = v;
#pragma unroll
            for (int dz = -1; dz <= 1; dz++) {
#pragma unroll
                for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
                    for (int dx = -1; dx <= 1; dx++) {
                        const int k = (dx != 0) + (dy != 0) + (dz != 0);
                        if (k == 0 || (!FULL && k != 1)) continue;
                        const int nx = x + dx, ny = y + dy, nz = z + dz;
                        if (nx < 0 || nx >= D.x || ny < 0 || ny >= D.y || nz < 0 || nz >= D.z) continue;
                        const unsigned u = (unsigned)nz * strideZ + (unsigned)ny * strideY + (unsigned)nx;
                        const int hu = h[u];
                        if (hu > bh || (hu == bh && u < best)) { bh = hu; best = u; }      // hu == bh >= 1: u is in S
                    }
                }
            }
        }
        parent[v] = best;
    }
}

// parent[v] <- parent[parent[v]].  One thread per voxel.  The flag is one word that every workgroup of every XCD would write: a
// wave that changed something sends one store, and only while it still reads 0 there (a stale 0 costs a store, nothing else), so
// that a round in which every voxel moves does not queue two million stores on one address.
__global__ __launch_bounds__(kBlock) void k_part_flatten(unsigned* __restrict__ parent, unsigned n, int* __restrict__ flag) {
    const unsigned v = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    bool changed = false;
    if (v < n) {
        const unsigned p = cc_load(&parent[v]);
        if (p != kCcNone && p != v) {
            const unsigned g = cc_load(&parent[p]);
            if (g != p) {
                __hip_atomic_store(&parent[v], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                changed = true;
            }
        }
    }
    const unsigned long long movers = __ballot(changed);
    if (movers && (int)(threadIdx.x % kWave) == (int)__ffsll((long long)movers) - 1 &&
        __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
        __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- phase 3: what the component kernels do not give.  minVox[b] = the smallest voxel of basin b: one atomic per workgroup when
// all its voxels of S lie in one basin (the huge basins of a typical scene: block_reduce over the label range and the minimum),
// else one per wave that holds one basin, else one per lane; and none at all when the slot, read first, already holds a value no
// larger than the candidate (a stale larger value costs an atomic that changes nothing): the workgroups of a huge basin do not
// queue on its one word.  peakH[b] = h at the peak.  One thread per voxel; no thread leaves before the collectives.
__device__ __forceinline__ void part_min_send(unsigned* slot, unsigned v) {
    if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v) atomicMin(slot, v);
}
struct PartSpan { int lo, hi; unsigned first; };         // the labels held (lo > hi: none) and the smallest voxel that holds one
__global__ __launch_bounds__(kBlock) void k_part_basin_min(const int* __restrict__ basin, const unsigned* __restrict__ parent, const int* __restrict__ h,
                                                          unsigned n, unsigned* __restrict__ minVox, int* __restrict__ peakH) {
    const unsigned v = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    const int b = v < n ? basin[v] : -1;
    const bool have = b >= 0;
    const PartSpan all = block_reduce<kBlock>(PartSpan{ have ? b : 0x7fffffff, have ? b : -1, have ? v : kCcNone }, [](PartSpan x, const PartSpan& y) {
        x.lo = min(x.lo, y.lo); x.hi = max(x.hi, y.hi); x.first = min(x.first, y.first);
        return x;
    });
    if (all.lo == all.hi) {                              // one basin in the whole workgroup
        if (threadIdx.x == 0) part_min_send(&minVox[all.lo], all.first);
    } else if (all.lo < all.hi) {
        int first;
        if (wave_uniform_label(have, b, first)) {
            const unsigned m = wave_min(have ? v : kCcNone);
            if (threadIdx.x % kWave == 0) part_min_send(&minVox[first], m);
        } else if (have) part_min_send(&minVox[b], v);
    }
    if (have && parent[v] == v) peakH[b] = h[v];
}

// ---- phase 4: basin edges.  One thread per voxel, the forward half of the neighbourhood: every unordered pair once, and its pass
// index min(a, b) is the thread's own voxel.  A slot is claimed by a compare-and-swap on its key; the largest (s, ~at) is the highest
// pass and, among equals, the smallest index.  A table without a free slot raises *full and the pair is dropped: the caller
// then discards the table and runs again with twice the capacity.
__device__ __forceinline__ void part_edge_insert(unsigned long long* keys, unsigned long long* vals, unsigned long long* pairs, unsigned cap, int shift,
                                                 unsigned long long key, unsigned long long val, int* full) {
    unsigned slot = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> shift);
    for (unsigned probe = 0; probe < cap; probe++, slot = (slot + 1u) & (cap - 1u)) {
        unsigned long long cur = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kPartEmpty) {
            cur = atomicCAS(&keys[slot], kPartEmpty, key);
            if (cur == kPartEmpty) cur = key;
        }
        if (cur == key) {
            atomicMax(&vals[slot], val);
            atomicAdd(&pairs[slot], 1ull);
            return;
        }
    }
    __hip_atomic_store(full, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool FULL>
__global__ __launch_bounds__(kBlock) void k_part_edges(const int* __restrict__ basin, const int* __restrict__ h, CcDims D, unsigned long long* __restrict__ keys,
                                                      unsigned long long* __restrict__ vals, unsigned long long* __restrict__ pairs, unsigned cap, int shift,
                                                      int* __restrict__ full) {
    const unsigned v = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    if (v >= D.n) return;
    const int a = basin[v];
    if (a < 0) return;
    const int x = (int)(v % (unsigned)D.x), y = (int)((v / (unsigned)D.x) % (unsigned)D.y), z = (int)(v / ((unsigned)D.x * (unsigned)D.y));
    const int hv = h[v];
    constexpr int nd = FULL ? 13 : 3;
    for (int k = 0; k < nd; k++) {
        const int di = FULL ? k : kCcFaceDirs[k];
        const int nx = x + kCcDirs[di][0], ny = y + kCcDirs[di][1], nz = z + kCcDirs[di][2];
        if (nx < 0 || nx >= D.x || ny < 0 || ny >= D.y || nz >= D.z) continue;
        const unsigned w = (unsigned)(((size_t)nz * D.y + ny) * (size_t)D.x + nx);
        const int b = basin[w];
        if (b < 0 || b == a) continue;
        const unsigned A = (unsigned)min(a, b), B = (unsigned)max(a, b);
        const unsigned s = (unsigned)min(hv, h[w]);
        part_edge_insert(keys, vals, pairs, cap, shift, ((unsigned long long)A << 32) | B, ((unsigned long long)s << 32) | (unsigned long long)(~v), full);
    }
}

// The occupied slots as a list, one atomic per wave (wave_append); every lane reaches the collective.
__global__ __launch_bounds__(kBlock) void k_part_compact(const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ vals,
                                                        const unsigned long long* __restrict__ pairs, unsigned cap, PartEdge* __restrict__ out,
                                                        unsigned* __restrict__ count) {
    const unsigned i = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    const unsigned long long key = i < cap ? keys[i] : kPartEmpty;
    const bool occupied = key != kPartEmpty;
    const unsigned at = wave_append<unsigned>(occupied ? 1u : 0u, count);
    if (occupied) out[at] = PartEdge{ key, vals[i], pairs[i] };
}

// ---- phase 5: labels[v] = map[basin[v]], in place; -1 stays.
__global__ __launch_bounds__(kBlock) void k_part_relabel(int* __restrict__ labels, unsigned n, const int* __restrict__ map) {
    const unsigned base = blockIdx.x * (unsigned)kCcChunk;
#pragma unroll 4
    for (int j = 0; j < kCcPerThread; j++) {
        const unsigned v = base + (unsigned)j * kBlock + threadIdx.x;
        if (v < n) {
            const int b = labels[v];
            if (b >= 0) labels[v] = map[b];
        }
    }
}

// ---- the edit's flip: a voxel of S with a neighbour of a larger part number takes newValue.  The decision reads the labels alone,
// so the order in which voxels flip does not matter.  One thread per voxel; the count: block_add_count.
template <bool FULL>
__global__ __launch_bounds__(kBlock) void k_part_cut(uint8_t* __restrict__ vox, const int* __restrict__ labels, CcDims D, unsigned newValue,
                                                    unsigned long long* __restrict__ changed) {
    const unsigned v = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    int count = 0;
    if (v < D.n) {
        const int l = labels[v];
        if (l >= 0) {
            const int x = (int)(v % (unsigned)D.x), y = (int)((v / (unsigned)D.x) % (unsigned)D.y), z = (int)(v / ((unsigned)D.x * (unsigned)D.y));
            bool hit = false;
#pragma unroll
            for (int dz = -1; dz <= 1; dz++) {
#pragma unroll
                for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
                    for (int dx = -1; dx <= 1; dx++) {
                        const int k = (dx != 0) + (dy != 0) + (dz != 0);
                        if (k == 0 || (!FULL && k != 1)) continue;
                        const int nx = x + dx, ny = y + dy, nz = z + dz;
                        if (nx < 0 || nx >= D.x || ny < 0 || ny >= D.y || nz < 0 || nz >= D.z) continue;
                        hit = hit || labels[((size_t)nz * D.y + ny) * (size_t)D.x + nx] > l;
                    }
                }
            }
            if (hit) { vox[v] = (uint8_t)newValue; count = 1; }
        }
    }
    block_add_count(count, changed);
}

}  // namespace rto

namespace {

static_assert(sizeof(rto_part) == 64 && sizeof(rto_neck) == 32 && sizeof(rto_parts_summary) == 32, "the part records of include/rto_hip.h");

// One segmentation: the tables, owned by whoever holds it (the context, or rto_edit_parts for the length of the call).  The label
// volume is the caller's buffer.
struct PartsResult {
    rto_part* d_parts = nullptr;
    rto_neck* d_necks = nullptr;
    rto_parts_summary sum = { 0, 0, 0, 0 };
    int64_t edges = 0, tableCap = 0;
    int rounds = 0;
    float ms[5] = { -1.f, -1.f, -1.f, -1.f, -1.f };
    void release() { (void)hipFree(d_parts); (void)hipFree(d_necks); d_parts = nullptr; d_necks = nullptr; }
};

int parts_check_args(rto_context* c, const char* who, int set, int connectivity, int ratio) {
    const std::string w(who);
    if (set != RTO_SET_SOLID && set != RTO_SET_EMPTY) return fail(c, RTO_E_INVALID, w + ": unknown set");
    if (connectivity != RTO_CONN_FACE && connectivity != RTO_CONN_FULL) return fail(c, RTO_E_INVALID, w + ": connectivity must be 6 or 26");
    if (ratio < 0 || ratio > RTO_PARTS_RATIO_MAX) return fail(c, RTO_E_INVALID, w + ": ratio must lie in [0, 1001]");
    const int rcGrid = resident_grid_check(c, who, ": labels are 32-bit");
    if (rcGrid != RTO_OK) return rcGrid;
    return dt_check_grid(c, who);
}

// What the host needs of a basin.
struct PartBasin { rto::CcComp box; unsigned minVox; int peakH; };

// Rule 5 to rule 9 over the basin table and the downloaded basin edges: the basin -> part map and the two tables.
void parts_merge(const std::vector<PartBasin>& basins, std::vector<rto::PartEdge>& edges, int ratio, std::vector<int>& map, std::vector<rto_part>& parts,
                 std::vector<rto_neck>& necks, rto_parts_summary& sum) {
    const int nb = (int)basins.size();
    auto passOf = [](const rto::PartEdge& e) { return (int64_t)(e.val >> 32); };
    auto atOf = [](const rto::PartEdge& e) { return (int64_t)(~(unsigned)(e.val & 0xffffffffull)); };
    std::sort(edges.begin(), edges.end(), [&](const rto::PartEdge& a, const rto::PartEdge& b) {
        if (passOf(a) != passOf(b)) return passOf(a) > passOf(b);
        return a.key < b.key;
    });
    std::vector<int> up(nb), P(nb);
    for (int i = 0; i < nb; i++) { up[i] = i; P[i] = basins[i].peakH; }
    auto find = [&](int a) { while (up[a] != a) { up[a] = up[up[a]]; a = up[a]; } return a; };
    const int64_t r2 = (int64_t)ratio * ratio;
    for (const rto::PartEdge& e : edges) {
        const int a = find((int)(e.key >> 32)), b = find((int)(e.key & 0xffffffffull));
        if (a == b) continue;
        if (1000000ll * passOf(e) >= r2 * (int64_t)std::min(P[a], P[b])) { up[b] = a; P[a] = std::max(P[a], P[b]); }
    }
    // clusters in ascending order of their smallest voxel
    std::vector<unsigned> first(nb, 0xffffffffu);
    for (int i = 0; i < nb; i++) { const int r = find(i); first[r] = std::min(first[r], basins[i].minVox); }
    std::vector<int> roots;
    for (int i = 0; i < nb; i++) if (up[i] == i) roots.push_back(i);
    std::sort(roots.begin(), roots.end(), [&](int a, int b) { return first[a] < first[b]; });
    std::vector<int> number(nb, -1);
    for (size_t i = 0; i < roots.size(); i++) number[roots[i]] = (int)i;
    map.resize(nb);
    parts.assign(roots.size(), rto_part{});
    for (size_t i = 0; i < roots.size(); i++) {
        rto_part& p = parts[i];
        p.root = (int64_t)first[roots[i]];
        for (int a = 0; a < 3; a++) { p.lo[a] = 0x7fffffff; p.hi[a] = -1; }
        p.peak = -1; p.peak_h = 0;
    }
    for (int i = 0; i < nb; i++) {
        const int n = number[find(i)];
        map[i] = n;
        rto_part& p = parts[n];
        const rto::CcComp& b = basins[i].box;
        p.voxels += b.voxels;
        for (int a = 0; a < 3; a++) { p.lo[a] = std::min(p.lo[a], b.lo[a]); p.hi[a] = std::max(p.hi[a], b.hi[a]); }
        p.touches |= b.touches;
        p.basins++;
        if (p.peak < 0 || basins[i].peakH > p.peak_h || (basins[i].peakH == p.peak_h && b.root < p.peak)) { p.peak = b.root; p.peak_h = basins[i].peakH; }
    }
    // necks: the surviving edges by (part_lo, part_hi), the highest pass first and among equals the smallest index
    struct Cross { int lo, hi; int64_t s, at, pairs; };
    std::vector<Cross> cross;
    for (const rto::PartEdge& e : edges) {
        const int a = map[e.key >> 32], b = map[e.key & 0xffffffffull];
        if (a != b) cross.push_back(Cross{ std::min(a, b), std::max(a, b), passOf(e), atOf(e), (int64_t)e.pairs });
    }
    std::sort(cross.begin(), cross.end(), [](const Cross& a, const Cross& b) {
        if (a.lo != b.lo) return a.lo < b.lo;
        if (a.hi != b.hi) return a.hi < b.hi;
        if (a.s != b.s) return a.s > b.s;
        return a.at < b.at;
    });
    necks.clear();
    int64_t pairs = 0;
    for (const Cross& x : cross) {
        if (necks.empty() || necks.back().part_lo != x.lo || necks.back().part_hi != x.hi) necks.push_back(rto_neck{ x.lo, x.hi, (int32_t)x.s, 0, x.at, 0 });
        necks.back().pairs += x.pairs;
        pairs += x.pairs;
    }
    sum.parts = (int64_t)parts.size(); sum.basins = nb; sum.necks = (int64_t)necks.size(); sum.pairs = pairs;
}

// Segments the resident grid: part numbers into d_labels (one int32 per voxel, the caller's), the tables into `out` (arguments
// already checked; the device is set and the stream drained).  On any error `out` is released and the context is as it was.
int parts_segment(rto_context* c, const char* who, int set, int connectivity, int ratio, int* d_labels, PartsResult& out) {
    using namespace rto;
    const std::string w(who);
    const CcDims D{ c->voxDim[0], c->voxDim[1], c->voxDim[2], (unsigned)grid_voxels(c) };
    hipStream_t s = c->stream;
    StreamEvents<4> events;
    RTO_HIP(c, events.create());
    struct OutGuard { PartsResult* r; bool keep = false; ~OutGuard() { if (!keep) r->release(); } } og{ &out };

    const CcTiles T(c->voxDim);
    const unsigned chunks = (D.n + kCcChunk - 1) / kCcChunk;
    const unsigned voxBlocks = (D.n + kBlock - 1) / kBlock;
    const bool full = connectivity == RTO_CONN_FULL;

    BuildScratch scratch(s);
    int* d_h = nullptr; unsigned* d_parent = nullptr; unsigned* d_blockCount = nullptr; unsigned* d_total = nullptr; int* d_flags = nullptr;
    RTO_HIP(c, scratch.alloc(&d_h, (size_t)D.n));
    RTO_HIP(c, scratch.alloc(&d_parent, (size_t)D.n));
    RTO_HIP(c, scratch.alloc(&d_blockCount, (size_t)chunks));
    RTO_HIP(c, scratch.alloc(&d_total, 1));
    RTO_HIP(c, scratch.alloc(&d_flags, (size_t)kPartMaxRounds + 1));
    RTO_HIP(c, hipMemsetAsync(d_flags, 0, (kPartMaxRounds + 1) * sizeof(int), s));

    // (1) the height: the transform of the other set, uncapped
    {
        float ms[3];
        const int rc = dt_transform(c, set == RTO_SET_SOLID ? RTO_SET_EMPTY : RTO_SET_SOLID, kDtNone - 1, d_h, ms);
        if (rc != RTO_OK) return rc;
        out.ms[0] = ms[0] + ms[1] + ms[2];
    }
    // (2) ascent, then pointer doubling until a launch changes nothing
    RTO_HIP(c, events.record(0, s));
    if (full) hipLaunchKernelGGL(k_part_ascend<true>, dim3((unsigned)T.count()), dim3(kBlock), 0, s, d_h, D, T.x, T.y, d_parent);
    else hipLaunchKernelGGL(k_part_ascend<false>, dim3((unsigned)T.count()), dim3(kBlock), 0, s, d_h, D, T.x, T.y, d_parent);
    RTO_HIP(c, hipGetLastError());
    int launched = 0, rounds = 0;
    int flags[kPartMaxRounds];
    while (rounds == 0 && launched < kPartMaxRounds) {
        for (int i = 0; i < kPartRoundsPerLook; i++) {
            hipLaunchKernelGGL(k_part_flatten, dim3(voxBlocks), dim3(kBlock), 0, s, d_parent, D.n, d_flags + launched + i);
            RTO_HIP(c, hipGetLastError());
        }
        RTO_HIP(c, hipMemcpyAsync(flags + launched, d_flags + launched, kPartRoundsPerLook * sizeof(int), hipMemcpyDeviceToHost, s));
        RTO_HIP(c, hipStreamSynchronize(s));
        for (int i = 0; i < kPartRoundsPerLook && rounds == 0; i++) if (flags[launched + i] == 0) rounds = launched + i + 1;      // the first clean launch
        launched += kPartRoundsPerLook;
    }
    if (rounds == 0) return fail(c, RTO_E_INTERNAL, w + ": the ascent did not flatten in 32 rounds");
    RTO_HIP(c, events.record(1, s));
    // (3) peaks in index order are the basins; the basin volume goes into d_labels
    hipLaunchKernelGGL(k_cc_flatten, dim3(chunks), dim3(kBlock), 0, s, d_parent, D.n, d_blockCount);
    RTO_HIP(c, hipGetLastError());
    hipLaunchKernelGGL((k_scan_counts<kBlock, unsigned, unsigned>), dim3(1), dim3(kBlock), 0, s, d_blockCount, (int)chunks, d_blockCount, d_total);
    RTO_HIP(c, hipGetLastError());
    unsigned total = 0;
    RTO_HIP(c, hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, s));
    RTO_HIP(c, hipStreamSynchronize(s));
    CcComp* d_basins = nullptr; unsigned* d_minVox = nullptr; int* d_peakH = nullptr;
    RTO_HIP(c, scratch.alloc(&d_basins, (size_t)total));
    RTO_HIP(c, scratch.alloc(&d_minVox, (size_t)total));
    RTO_HIP(c, scratch.alloc(&d_peakH, (size_t)total));
    hipLaunchKernelGGL(k_cc_rank, dim3(chunks), dim3(kBlock), 0, s, d_parent, D.n, d_blockCount, d_labels, d_basins);
    RTO_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(k_cc_label, dim3(chunks), dim3(kBlock), 0, s, d_parent, D.n, d_labels);
    RTO_HIP(c, hipGetLastError());
    std::vector<PartBasin> basins(total);
    if (total) {
        const unsigned statBlocks = (D.n + kBlock * kCcStatPerThread - 1) / (kBlock * kCcStatPerThread);
        hipLaunchKernelGGL(k_cc_stats, dim3(statBlocks), dim3(kBlock), 0, s, d_labels, D, d_basins);
        RTO_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(k_cc_touches, dim3((total + kBlock - 1) / kBlock), dim3(kBlock), 0, s, d_basins, total, D);
        RTO_HIP(c, hipGetLastError());
        RTO_HIP(c, hipMemsetAsync(d_minVox, 0xff, (size_t)total * sizeof(unsigned), s));
        hipLaunchKernelGGL(k_part_basin_min, dim3(voxBlocks), dim3(kBlock), 0, s, d_labels, d_parent, d_h, D.n, d_minVox, d_peakH);
        RTO_HIP(c, hipGetLastError());
    }
    RTO_HIP(c, events.record(2, s));
    // (4) basin edges: one record per edge comes down
    std::vector<PartEdge> edges;
    int64_t tableCap = 0;
    if (total > 1) {
        uint64_t want = c->partsFirstCap > 0 ? (uint64_t)c->partsFirstCap : std::max<uint64_t>(1024, 16ull * total);
        uint64_t cap = 2;
        while (cap < want) cap <<= 1;
        bool done = false;
        for (int attempt = 0; attempt <= kPartMaxGrowths && !done; attempt++, cap <<= 1) {
            if (cap > (1ull << 31)) break;
            int shift = 64;
            for (uint64_t q = cap; q > 1; q >>= 1) shift--;
            BuildScratch table(s);
            unsigned long long* d_keys = nullptr; unsigned long long* d_vals = nullptr; unsigned long long* d_pairs = nullptr;
            PartEdge* d_list = nullptr; unsigned* d_count = nullptr;
            RTO_HIP(c, table.alloc(&d_keys, (size_t)cap));
            RTO_HIP(c, table.alloc(&d_vals, (size_t)cap));
            RTO_HIP(c, table.alloc(&d_pairs, (size_t)cap));
            RTO_HIP(c, table.alloc(&d_count, 1));
            RTO_HIP(c, hipMemsetAsync(d_keys, 0xff, (size_t)cap * sizeof(unsigned long long), s));
            RTO_HIP(c, hipMemsetAsync(d_vals, 0, (size_t)cap * sizeof(unsigned long long), s));
            RTO_HIP(c, hipMemsetAsync(d_pairs, 0, (size_t)cap * sizeof(unsigned long long), s));
            RTO_HIP(c, hipMemsetAsync(d_count, 0, sizeof(unsigned), s));
            int* d_full = d_flags + kPartMaxRounds;
            RTO_HIP(c, hipMemsetAsync(d_full, 0, sizeof(int), s));
            if (full) hipLaunchKernelGGL(k_part_edges<true>, dim3(voxBlocks), dim3(kBlock), 0, s, d_labels, d_h, D, d_keys, d_vals, d_pairs, (unsigned)cap, shift, d_full);
            else hipLaunchKernelGGL(k_part_edges<false>, dim3(voxBlocks), dim3(kBlock), 0, s, d_labels, d_h, D, d_keys, d_vals, d_pairs, (unsigned)cap, shift, d_full);
            RTO_HIP(c, hipGetLastError());
            int isFull = 0;
            RTO_HIP(c, hipMemcpyAsync(&isFull, d_full, sizeof isFull, hipMemcpyDeviceToHost, s));
            RTO_HIP(c, hipStreamSynchronize(s));
            if (isFull) continue;
            RTO_HIP(c, table.alloc(&d_list, (size_t)cap));
            hipLaunchKernelGGL(k_part_compact, dim3((unsigned)((cap + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, d_keys, d_vals, d_pairs, (unsigned)cap, d_list, d_count);
            RTO_HIP(c, hipGetLastError());
            unsigned count = 0;
            RTO_HIP(c, hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, s));
            RTO_HIP(c, hipStreamSynchronize(s));
            edges.resize(count);
            if (count) RTO_HIP(c, hipMemcpyAsync(edges.data(), d_list, (size_t)count * sizeof(PartEdge), hipMemcpyDeviceToHost, s));
            RTO_HIP(c, hipStreamSynchronize(s));
            tableCap = (int64_t)cap;
            done = true;
        }
        if (!done) return fail(c, RTO_E_INTERNAL, w + ": the basin-edge table was still full after 8 doublings");
    }
    RTO_HIP(c, events.record(3, s));
    // (5) the host's merge over basins, then basin numbers become part numbers
    const auto t0 = std::chrono::steady_clock::now();
    if (total) {
        std::vector<CcComp> boxes(total);
        std::vector<unsigned> minVox(total);
        std::vector<int> peakH(total);
        RTO_HIP(c, hipMemcpyAsync(boxes.data(), d_basins, (size_t)total * sizeof(CcComp), hipMemcpyDeviceToHost, s));
        RTO_HIP(c, hipMemcpyAsync(minVox.data(), d_minVox, (size_t)total * sizeof(unsigned), hipMemcpyDeviceToHost, s));
        RTO_HIP(c, hipMemcpyAsync(peakH.data(), d_peakH, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, s));
        RTO_HIP(c, hipStreamSynchronize(s));
        for (unsigned i = 0; i < total; i++) basins[i] = PartBasin{ boxes[i], minVox[i], peakH[i] };
    }
    std::vector<int> map;
    std::vector<rto_part> parts;
    std::vector<rto_neck> necks;
    parts_merge(basins, edges, ratio, map, parts, necks, out.sum);
    RTO_HIP(c, fallible_malloc(reinterpret_cast<void**>(&out.d_parts), (parts.empty() ? 1 : parts.size()) * sizeof(rto_part)));
    RTO_HIP(c, fallible_malloc(reinterpret_cast<void**>(&out.d_necks), (necks.empty() ? 1 : necks.size()) * sizeof(rto_neck)));
    if (total) {
        int* d_map = nullptr;
        RTO_HIP(c, scratch.alloc(&d_map, (size_t)total));
        RTO_HIP(c, hipMemcpyAsync(d_map, map.data(), (size_t)total * sizeof(int), hipMemcpyHostToDevice, s));
        RTO_HIP(c, hipMemcpyAsync(out.d_parts, parts.data(), parts.size() * sizeof(rto_part), hipMemcpyHostToDevice, s));
        if (!necks.empty()) RTO_HIP(c, hipMemcpyAsync(out.d_necks, necks.data(), necks.size() * sizeof(rto_neck), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_part_relabel, dim3(chunks), dim3(kBlock), 0, s, d_labels, D.n, d_map);
        RTO_HIP(c, hipGetLastError());
    }
    RTO_HIP(c, hipStreamSynchronize(s));                                // the uploads read host vectors of this scope
    out.ms[4] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (int i = 0; i < 3; i++) RTO_HIP(c, events.elapsed(i, i + 1, &out.ms[1 + i]));
    out.edges = (int64_t)edges.size();
    out.tableCap = tableCap;
    out.rounds = rounds;
    og.keep = true;
    return RTO_OK;
}

int parts_resident_check(rto_context* c, const char* who) { return resident_field_check(c, who, kFieldParts); }

}  // namespace

extern "C" {

int rto_segment_parts(rto_context* c, int set, int connectivity, int ratio, rto_parts_summary* summary) {
    if (!c) return RTO_E_INVALID;
    const int rcArgs = parts_check_args(c, "rto_segment_parts", set, connectivity, ratio);
    if (rcArgs != RTO_OK) return rcArgs;
    FieldDraft draft(c, kFieldParts);
    const int rcDraft = draft.begin();
    if (rcDraft != RTO_OK) return rcDraft;
    PartsResult r;
    const int rc = parts_segment(c, "rto_segment_parts", set, connectivity, ratio, draft.d, r);
    if (rc != RTO_OK) return rc;
    free_parts(c);
    draft.publish();
    c->d_partTab = r.d_parts; c->d_neckTab = r.d_necks; c->partsSum = r.sum;
    c->partsEdges = r.edges; c->partsTableCap = r.tableCap; c->partsRounds = r.rounds;
    for (int i = 0; i < 5; i++) c->partsMs[i] = r.ms[i];
    if (summary) *summary = r.sum;
    return RTO_OK;
}

int rto_download_part_labels(rto_context* c, int32_t* out, int64_t capacity) { return download_field(c, "rto_download_part_labels", kFieldParts, out, capacity); }

int rto_download_parts(rto_context* c, rto_part* out, int64_t capacity, int64_t* count) {
    if (!c) return RTO_E_INVALID;
    const int rc = parts_resident_check(c, "rto_download_parts");
    if (rc != RTO_OK) return rc;
    if (count) *count = c->partsSum.parts;
    if (!out) return RTO_OK;
    return download_resident(c, "rto_download_parts", out, capacity, c->d_partTab, c->partsSum.parts, sizeof(rto_part));
}

int rto_download_necks(rto_context* c, rto_neck* out, int64_t capacity, int64_t* count) {
    if (!c) return RTO_E_INVALID;
    const int rc = parts_resident_check(c, "rto_download_necks");
    if (rc != RTO_OK) return rc;
    if (count) *count = c->partsSum.necks;
    if (!out) return RTO_OK;
    return download_resident(c, "rto_download_necks", out, capacity, c->d_neckTab, c->partsSum.necks, sizeof(rto_neck));
}

int rto_parts_device(rto_context* c, int32_t** d_labels, rto_part** d_parts, int64_t* parts, rto_neck** d_necks, int64_t* necks) {
    if (!c) return RTO_E_INVALID;
    const int rc = parts_resident_check(c, "rto_parts_device");
    if (rc != RTO_OK) return rc;
    if (d_labels) *d_labels = c->d_field[kFieldParts];
    if (d_parts) *d_parts = c->d_partTab;
    if (parts) *parts = c->partsSum.parts;
    if (d_necks) *d_necks = c->d_neckTab;
    if (necks) *necks = c->partsSum.necks;
    return RTO_OK;
}

int rto_last_parts_ms(const rto_context* c, float ms[5]) { return copy_last_ms(c, &rto_context::partsMs, ms); }

int rto_debug_parts(const rto_context* c, int64_t* basins, int64_t* edges, int* rounds, int64_t* capacity) {
    if (!c) return RTO_E_INVALID;
    if (basins) *basins = c->partsSum.basins;
    if (edges) *edges = c->partsEdges;
    if (rounds) *rounds = c->partsRounds;
    if (capacity) *capacity = c->partsTableCap;
    return RTO_OK;
}

int rto_debug_parts_capacity(rto_context* c, int64_t first_capacity) {
    if (!c) return RTO_E_INVALID;
    if (first_capacity < 0 || first_capacity > (1ll << 31)) return fail(c, RTO_E_INVALID, "rto_debug_parts_capacity: the capacity must lie in [0, 2^31]");
    c->partsFirstCap = first_capacity;
    return RTO_OK;
}

int rto_edit_parts(rto_context* c, int set, int connectivity, int ratio, int64_t* changed) {
    using namespace rto;
    if (!c) return RTO_E_INVALID;
    if (changed) *changed = 0;
    const int rcArgs = parts_check_args(c, "rto_edit_parts", set, connectivity, ratio);
    if (rcArgs != RTO_OK) return rcArgs;
    RTO_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    RTO_HIP(c, hipStreamSynchronize(s));
    unsigned long long count = 0;
    {
        BuildScratch scratch(s);
        int* d_labels = nullptr;
        ChangedCount d_count;
        const CcDims D{ c->voxDim[0], c->voxDim[1], c->voxDim[2], (unsigned)grid_voxels(c) };
        RTO_HIP(c, scratch.alloc(&d_labels, (size_t)D.n));
        RTO_HIP(c, d_count.alloc(scratch));
        PartsResult r;
        const int rc = parts_segment(c, "rto_edit_parts", set, connectivity, ratio, d_labels, r);
        if (rc != RTO_OK) return rc;
        struct Release { PartsResult* r; ~Release() { r->release(); } } rel{ &r };
        if (r.sum.necks == 0) return RTO_OK;                             // no two parts touch: nothing to cut
        RTO_HIP(c, d_count.clear(s));
        const unsigned blocks = (D.n + kBlock - 1) / kBlock;
        const unsigned newValue = set == RTO_SET_SOLID ? 0u : 1u;
        if (connectivity == RTO_CONN_FULL) hipLaunchKernelGGL(k_part_cut<true>, dim3(blocks), dim3(kBlock), 0, s, c->d_vox, d_labels, D, newValue, d_count.d);
        else hipLaunchKernelGGL(k_part_cut<false>, dim3(blocks), dim3(kBlock), 0, s, c->d_vox, d_labels, D, newValue, d_count.d);
        RTO_HIP(c, hipGetLastError());
        RTO_HIP(c, d_count.read(s, &count));
    }
    if (changed) *changed = (int64_t)count;
    if (count == 0) return RTO_OK;           // nothing is dropped: rebuild_from_resident_grid's comment

    return rebuild_from_resident_grid(c, c->d_triOffset != nullptr, nullptr, nullptr);
}

}  // extern "C"
