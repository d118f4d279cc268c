// rto_skeleton.inc -- skeletons of the resident grid (include/rto_hip.h, rto_skeleton_field / rto_edit_skeleton): topology-preserving
// thinning of a set (the FILLED or the EMPTY voxels) in passes of one mark and eight subfield sub-steps, kept resident as one int32
// per voxel (-1 outside the set, 0 the skeleton, p the pass that removed the voxel); and the edit that replaces the set by its
// skeleton, with the voxel edits' rebuild.  Included at the end of rto_api.hip, after rto_measure.inc.
//
// Rule (DESIGN.md section 23).  A voxel beyond the grid is not in the set.  Pass p: M = the voxels of X with a neighbour (6 under
// FULL, 26 under FACE) not in X; then for s = 0 .. 7 every voxel of subfield (i & 1) + 2 (j & 1) + 4 (k & 1) == s that is in M, no
// anchor, not kept by the mode and simple leaves X.  The first pass that removes nothing ends the thinning.
//
// State: X, M and the anchors A as bit rows, one 32-bit word per 32 voxels of a grid row (word wx of row (y, z) holds x = 32 wx ..
// 32 wx + 31; bits beyond dimX are 0).  A 32 x 8 x 8 tile (k_cc_local's) is 64 words, written by the tile's own workgroup only.
// (1) k_skel_init makes X and writes k = -1 / 0; k_skel_anchors sets A.
// (2) per pass: k_skel_mark makes M & ~A for EVERY word from the X of the pass's start (a tile that is woken in the middle of a pass
// must not take its newly exposed voxels for marked ones, so M is never derived from the current X); then one launch of k_skel_step
// per sub-step, one workgroup per tile.  The workgroup stages the X rows of its tile and a halo of one voxel (10 x 10 rows of 34
// bits) in LDS; in sub-step s a tile holds 16 x 4 x 4 = 256 voxels of subfield s, one per thread; a thread whose voxel is marked
// gathers the 27-bit block from 9 rows by shifts and floods inside it in registers (sk_simple).
// No synchronisation inside a launch: in sub-step s a verdict depends on the 26 neighbours of a subfield-s voxel, none of which is of
// subfield s (a neighbour differs in the parity of a coordinate), and only subfield-s voxels change in that launch.  The subfield-s
// bits a workgroup may read from a neighbour's word while the owner clears them are bits it never uses; a 32-bit word is stored whole.
// Worklist: stamp[tile] = the last pass in which a voxel of the tile or of its halo was removed (whoever removes a voxel raises the
// stamp of its own tile and of the up to 26 tiles that hold a neighbour of it).  A tile skips sub-step (P, s) when its stamp is below
// P - 1: nothing in the tile and its halo has changed since the start of pass P - 1, so M, the blocks and every verdict are those of
// pass P - 1, which removed nothing there.  (A window of 8 sub-steps would be too short: a removal at (P - 1, s' < s) first marks its
// neighbour at pass P.)  A stamp read while a neighbour raises it in the same launch is older or newer; the removal behind it is of
// subfield s and changes no verdict of this launch.  The host sends `look` passes between two looks at the per-pass "removed something" flags;
// passes behind the fixed point remove nothing.
// (3) k_skel_summary counts the volume.

namespace rto {

constexpr int kSkRowsY = kCcTileY + 2, kSkRowsZ = kCcTileZ + 2;          // halo rows
constexpr int kSkRows = kSkRowsY * kSkRowsZ;                             // 100 row windows, 800 bytes of LDS
constexpr int kSkTileRows = kCcTileY * kCcTileZ;                         // 64 words of a tile
static_assert(kCcTileX == 32, "a tile row is one word");
static_assert(kBlock == (kCcTileX / 2) * (kCcTileY / 2) * (kCcTileZ / 2), "one thread per voxel of a subfield");
static_assert(kSkRows <= kBlock && kSkTileRows <= kWave, "one thread per row window; one wave for the tile's words");

// Cells of the 3 x 3 x 3 block, bit (dx + 1) + 3 (dy + 1) + 9 (dz + 1).
constexpr unsigned sk_where(int axis, int value) {
    unsigned m = 0u;
    for (int b = 0; b < 27; b++) {
        const int d[3] = { b % 3 - 1, (b / 3) % 3 - 1, b / 9 - 1 };
        if (d[axis] == value) m |= 1u << b;
    }
    return m;
}
constexpr unsigned sk_within(int lo, int hi) {                           // the cells that differ from the centre on lo .. hi axes
    unsigned m = 0u;
    for (int b = 0; b < 27; b++) {
        const int c = (b % 3 != 1) + ((b / 3) % 3 != 1) + (b / 9 != 1);
        if (c >= lo && c <= hi) m |= 1u << b;
    }
    return m;
}
constexpr unsigned kSkAll = (1u << 27) - 1u, kSkN26 = sk_within(1, 3), kSkN18 = sk_within(1, 2), kSkN6 = sk_within(1, 1);
constexpr unsigned kSkNotX0 = kSkAll & ~sk_where(0, -1), kSkNotX2 = kSkAll & ~sk_where(0, 1);
constexpr unsigned kSkNotY0 = kSkAll & ~sk_where(1, -1), kSkNotY2 = kSkAll & ~sk_where(1, 1);

struct SkDims { int x, y, z, wordsX; unsigned words; };

// Words that another workgroup may write in the same launch are read and written whole (relaxed atomics), at WORKGROUP scope: nothing
// a launch reads needs what another workgroup writes in that launch (the argument above), only what earlier launches wrote, and
// that the launch boundary makes visible.  Agent scope would send every one of a tile's 300 window loads past the caches to the
// cross-die fabric: measured on the 512^3 sphere, the thinning then took 109.6 ms instead of 26.0.
__device__ __forceinline__ unsigned sk_load(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void sk_store(unsigned* p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// One step of growth along an axis inside the block.  Every shift is masked back to the block's 27 bits and to the columns or rows
// that do not wrap: bit 24 shifted by 3 is bit 27, and from there a further shift would bring it back in as bit 18.
__device__ __forceinline__ unsigned sk_grow_x(unsigned m) { return m | ((m << 1) & kSkNotX0) | ((m >> 1) & kSkNotX2); }
__device__ __forceinline__ unsigned sk_grow_y(unsigned m) { return m | ((m << 3) & kSkNotY0) | ((m >> 3) & kSkNotY2); }
__device__ __forceinline__ unsigned sk_grow_z(unsigned m) { return m | ((m << 9) & kSkAll) | (m >> 9); }

// What of `inside` the lowest bit of `from` reaches, by 26 (the three growths composed) or by 6 (their union).
template <bool BY26>
__device__ __forceinline__ unsigned sk_flood(unsigned from, unsigned inside) {
    unsigned f = from & (0u - from);
    for (;;) {
        const unsigned g = (BY26 ? sk_grow_z(sk_grow_y(sk_grow_x(f))) : (sk_grow_x(f) | sk_grow_y(f) | sk_grow_z(f))) & inside;
        if (g == f) return f;
        f = g;
    }
}

// Is the centre a simple point under FULL of the set whose voxels are n's ones?  (FACE: the caller complements n.)
__device__ __forceinline__ bool sk_simple(unsigned n) {
    n &= kSkN26;
    if (!n || sk_flood<true>(n, n) != n) return false;
    const unsigned b = ~n & kSkN18, b6 = b & kSkN6;
    return b6 && (sk_flood<false>(b6, b) & b6) == b6;
}

// The X bits of x = 32 wx - 1 .. 32 wx + 32 of row (y, z) as bits 0 .. 33; beyond the grid: 0.
__device__ __forceinline__ unsigned long long sk_window(const unsigned* X, const SkDims& D, int wx, int y, int z) {
    if (y < 0 || y >= D.y || z < 0 || z >= D.z) return 0ull;
    const unsigned* r = X + ((size_t)z * D.y + y) * (size_t)D.wordsX;
    unsigned long long w = (unsigned long long)sk_load(r + wx) << 1;
    if (wx > 0) w |= (unsigned long long)(sk_load(r + wx - 1) >> 31);
    if (wx + 1 < D.wordsX) w |= (unsigned long long)(sk_load(r + wx + 1) & 1u) << 33;
    return w;
}

// ---- init.  One thread per word: X from the grid, k = 0 in the set and -1 outside.  WIDE: dimX % 32 == 0, so a word's 32 bytes
// and 32 values are whole and aligned.
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void k_skel_init(const uint8_t* __restrict__ vox, SkDims D, unsigned setValue, unsigned* __restrict__ X,
                                                     int* __restrict__ k) {
    const unsigned w = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    if (w >= D.words) return;
    const unsigned wx = w % (unsigned)D.wordsX, row = w / (unsigned)D.wordsX;
    const size_t base = (size_t)row * (size_t)D.x + (size_t)wx * 32u;
    unsigned bits = 0u;
    if (WIDE) {
        const uint4 a = *reinterpret_cast<const uint4*>(vox + base), b = *reinterpret_cast<const uint4*>(vox + base + 16);
        const unsigned q[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
#pragma unroll
        for (int j = 0; j < 32; j++) bits |= (((q[j >> 2] >> (8 * (j & 3))) & 0xffu) == setValue ? 1u : 0u) << j;
#pragma unroll
        for (int j = 0; j < 32; j += 4)
            *reinterpret_cast<int4*>(k + base + j) = make_int4((int)((bits >> j) & 1u) - 1, (int)((bits >> (j + 1)) & 1u) - 1,
                                                               (int)((bits >> (j + 2)) & 1u) - 1, (int)((bits >> (j + 3)) & 1u) - 1);
    } else {
        const int cnt = min(32, D.x - (int)wx * 32);
        for (int j = 0; j < cnt; j++) {
            const unsigned in = (unsigned)vox[base + j] == setValue ? 1u : 0u;
            bits |= in << j;
            k[base + j] = (int)in - 1;
        }
    }
    X[w] = bits;
}

// One thread per anchor (all already known to be voxels of the grid).  A is zero before the launch; duplicates set the same bit.
__global__ __launch_bounds__(kBlock) void k_skel_anchors(const long long* __restrict__ anchors, unsigned count, SkDims D, unsigned* __restrict__ A) {
    const unsigned i = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    if (i >= count) return;
    const unsigned v = (unsigned)anchors[i];
    const unsigned x = v % (unsigned)D.x, row = v / (unsigned)D.x;
    atomicOr(&A[(size_t)row * (size_t)D.wordsX + x / 32u], 1u << (x & 31u));
}

// ---- mark.  One thread per word: M = X & ~A & ~(all the neighbours are in X), from the X of the pass's start.
template <bool FULL>
__global__ __launch_bounds__(kBlock) void k_skel_mark(const unsigned* __restrict__ X, const unsigned* __restrict__ A, SkDims D, unsigned* __restrict__ M) {
    const unsigned w = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    if (w >= D.words) return;
    const unsigned own = X[w] & ~A[w];
    unsigned m = 0u;
    if (own) {
        const int wx = (int)(w % (unsigned)D.wordsX), row = (int)(w / (unsigned)D.wordsX);
        const int y = row % D.y, z = row / D.y;
        unsigned long long all;
        if (FULL) {
            const unsigned long long c = sk_window(X, D, wx, y, z);
            all = c & (c >> 2) & (sk_window(X, D, wx, y - 1, z) >> 1) & (sk_window(X, D, wx, y + 1, z) >> 1) & (sk_window(X, D, wx, y, z - 1) >> 1) &
                  (sk_window(X, D, wx, y, z + 1) >> 1);
        } else {
            all = ~0ull;
#pragma unroll
            for (int dz = -1; dz <= 1; dz++)
#pragma unroll
                for (int dy = -1; dy <= 1; dy++) {
                    const unsigned long long c = sk_window(X, D, wx, y + dy, z + dz);
                    all &= c & (c >> 1) & (c >> 2);
                }
        }
        m = own & ~(unsigned)all;
    }
    M[w] = m;
}

// ---- sub-step s of pass `pass`.  Workgroup b owns tile b.  Thread t owns the voxel of subfield s at (2 (t % 16), 2 (t / 16 % 4),
// 2 (t / 64)) + the subfield's parities; tiles start on even coordinates, so local and global parities agree.  *removed: set when
// the pass removes a voxel (every writer stores the same 1); runs[b]: the sub-steps tile b has run, its own word.  Neither is one
// address that every running tile adds to.
template <bool FULL, bool CURVE>
__global__ __launch_bounds__(kBlock) void k_skel_step(unsigned* X, const unsigned* __restrict__ M, int* __restrict__ k, int* stamp, SkDims D, int tilesX,
                                                     int tilesY, int tilesZ, int pass, int s, unsigned* __restrict__ removed, unsigned* __restrict__ runs) {
    __shared__ unsigned long long rows[kSkRows];
    __shared__ unsigned rem[kSkTileRows];                           // the bits this sub-step removes from the tile's words
    __shared__ unsigned marks;                                      // bit (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1): that tile's stamp is to rise
    __shared__ int on;
    const int t = (int)threadIdx.x;
    const int bid = (int)blockIdx.x;
    if (t == 0) { on = __hip_atomic_load(&stamp[bid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= pass - 1 ? 1 : 0; marks = 0u; }
    __syncthreads();
    if (!on) return;                                                // the whole workgroup leaves: `on` is one LDS word
    const int tx = bid % tilesX, ty = (bid / tilesX) % tilesY, tz = bid / (tilesX * tilesY);
    const int x0 = tx * kCcTileX, y0 = ty * kCcTileY, z0 = tz * kCcTileZ;
    if (t < kSkTileRows) rem[t] = 0u;
    if (t < kSkRows) rows[t] = sk_window(X, D, tx, y0 + t % kSkRowsY - 1, z0 + t / kSkRowsY - 1);
    const int lx = 2 * (t % 16) + (s & 1), ly = 2 * ((t / 16) % 4) + ((s >> 1) & 1), lz = 2 * (t / 64) + ((s >> 2) & 1);
    const int gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
    const bool inGrid = gx < D.x && gy < D.y && gz < D.z;
    // a marked voxel of subfield s is still in X: it can have left in this sub-step of this pass only
    const bool cand = inGrid && ((M[((size_t)gz * D.y + gy) * (size_t)D.wordsX + tx] >> lx) & 1u);
    __syncthreads();
    bool go = false;
    if (cand) {
        unsigned m = 0u;
#pragma unroll
        for (int dz = 0; dz < 3; dz++)
#pragma unroll
            for (int dy = 0; dy < 3; dy++) m |= ((unsigned)(rows[(lz + dz) * kSkRowsY + (ly + dy)] >> lx) & 7u) << (3 * dy + 9 * dz);
        const unsigned n = m & kSkN26;
        if (CURVE && __popc(n) == 1) go = false;                    // a curve's end stays
        else go = sk_simple(FULL ? n : ~n & kSkN26);
    }
    if (go) {
        atomicOr(&rem[lz * kCcTileY + ly], 1u << lx);
        k[((size_t)gz * D.y + gy) * (size_t)D.x + gx] = pass;
        // the neighbours at offset -1 / +1 along an axis lie in the tile before / after when the voxel is on that face
        const int ex = lx == 0 ? -1 : (lx == kCcTileX - 1 ? 1 : 0), ey = ly == 0 ? -1 : (ly == kCcTileY - 1 ? 1 : 0),
                  ez = lz == 0 ? -1 : (lz == kCcTileZ - 1 ? 1 : 0);
        unsigned mine = 0u;
#pragma unroll
        for (int az = 0; az < 2; az++)
#pragma unroll
            for (int ay = 0; ay < 2; ay++)
#pragma unroll
                for (int ax = 0; ax < 2; ax++) mine |= 1u << (((az ? ez : 0) + 1) * 9 + ((ay ? ey : 0) + 1) * 3 + ((ax ? ex : 0) + 1));
        atomicOr(&marks, mine);
    }
    __syncthreads();
    if (t < kWave) {                                                // the tile's words: only this workgroup writes them
        const unsigned r = t < kSkTileRows ? rem[t] : 0u;
        if (r) {
            unsigned* word = X + ((size_t)(z0 + t / kCcTileY) * D.y + (y0 + t % kCcTileY)) * (size_t)D.wordsX + tx;
            sk_store(word, sk_load(word) & ~r);
        }
        const unsigned long long any = __ballot(r != 0u);
        if (t == 0) {
            if (any) sk_store(removed, 1u);
            runs[bid] += 1u;
        }
    }
    if (t < 27 && ((marks >> t) & 1u)) {
        const int nx = tx + t % 3 - 1, ny = ty + (t / 3) % 3 - 1, nz = tz + t / 9 - 1;
        if (nx >= 0 && nx < tilesX && ny >= 0 && ny < tilesY && nz >= 0 && nz < tilesZ)
            __hip_atomic_store(&stamp[(nz * tilesY + ny) * tilesX + nx], pass, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// ---- summary.  out[0]: voxels with k == 0; out[1]: with k > 0; out[2]: the largest k (zero before the launch).
__global__ __launch_bounds__(kBlock) void k_skel_summary(const int* __restrict__ k, unsigned n, unsigned long long* __restrict__ out) {
    struct SkelSums { unsigned kept, gone, top; } s = { 0u, 0u, 0u };
    for (unsigned v = blockIdx.x * (unsigned)kBlock + threadIdx.x; v < n; v += gridDim.x * (unsigned)kBlock) {
        const int q = k[v];
        s.kept += q == 0 ? 1u : 0u;
        s.gone += q > 0 ? 1u : 0u;
        s.top = max(s.top, (unsigned)max(q, 0));
    }
    s = block_reduce<kBlock>(s, [](SkelSums a, const SkelSums& b) {
        a.kept += b.kept; a.gone += b.gone; a.top = max(a.top, b.top);
        return a;
    });
    if (threadIdx.x == 0) {
        if (s.kept) atomicAdd(&out[0], (unsigned long long)s.kept);
        if (s.gone) atomicAdd(&out[1], (unsigned long long)s.gone);
        if (s.top) atomicMax(&out[2], (unsigned long long)s.top);
    }
}

// ---- the edit's flip.  Every voxel with k > 0 takes `to`; a thread owns 16 consecutive voxels.  The count: block_add_count.
__global__ __launch_bounds__(kBlock) void k_skel_flip(uint8_t* __restrict__ vox, const int* __restrict__ k, unsigned n, unsigned to,
                                                     unsigned long long* __restrict__ changed) {
    const unsigned v0 = (blockIdx.x * (unsigned)kBlock + threadIdx.x) * (unsigned)kCcVec;
    int count = 0;
    for (int j = 0; j < kCcVec; j++) {
        const unsigned v = v0 + (unsigned)j;
        if (v0 < n && v < n && k[v] > 0) { vox[v] = (uint8_t)to; count++; }
    }
    block_add_count(count, changed);
}

}  // namespace rto

namespace {

struct SkelRun {
    float ms[2] = { -1.f, -1.f };      // init, thinning
    int64_t launches = 0;              // mark and sub-step launches sent
    int64_t tilesRun = 0;              // tiles run, summed over the sub-steps
};

// set, connectivity, mode, anchors, max_passes, then the grid: rto_geodesic_field's order.
int skel_check_args(rto_context* c, const char* who, int set, int connectivity, int mode, const int64_t* anchors, int64_t n, int64_t max_passes) {
    const std::string w(who);
    if (set != RTO_SET_SOLID && set != RTO_SET_EMPTY) return fail(c, RTO_E_INVALID, w + ": unknown set");
    if (connectivity != RTO_CONN_FACE && connectivity != RTO_CONN_FULL) return fail(c, RTO_E_INVALID, w + ": connectivity must be 6 or 26");
    if (mode != RTO_SKEL_TOPOLOGY && mode != RTO_SKEL_CURVE) return fail(c, RTO_E_INVALID, w + ": unknown mode");
    if (mode == RTO_SKEL_CURVE && connectivity != RTO_CONN_FULL) return fail(c, RTO_E_INVALID, w + ": RTO_SKEL_CURVE needs RTO_CONN_FULL");
    if (n < 0) return fail(c, RTO_E_INVALID, w + ": n is negative");
    if (n > 0 && !anchors) return fail(c, RTO_E_INVALID, w + ": anchors is NULL");
    if (max_passes < 1) return fail(c, RTO_E_INVALID, w + ": max_passes is below 1");
    const int rcGrid = resident_grid_check(c, who, ": the field is 32-bit");
    if (rcGrid != RTO_OK) return rcGrid;
    return voxel_list_check(c, who, "an anchor", anchors, n);
}

// The field into d_out (one int32 per voxel; arguments already checked).  The context is not touched, but for the stream.
int skel_thin(rto_context* c, const char* who, int set, int connectivity, int mode, const int64_t* anchors, int64_t n, int64_t max_passes,
              int* d_out, SkelRun& run) {
    using namespace rto;
    const int64_t nvox = grid_voxels(c);
    const int wordsX = (c->voxDim[0] + 31) / 32;
    const SkDims D{ c->voxDim[0], c->voxDim[1], c->voxDim[2], wordsX, (unsigned)((int64_t)wordsX * c->voxDim[1] * c->voxDim[2]) };
    hipStream_t s = c->stream;
    StreamEvents<3> events;
    RTO_HIP(c, events.create());
    const CcTiles T(c->voxDim);
    const size_t tiles = T.count();
    const unsigned setValue = set == RTO_SET_SOLID ? 1u : 0u;
    const bool full = connectivity == RTO_CONN_FULL, curve = mode == RTO_SKEL_CURVE;
    BuildScratch scratch(s);
    VoxelList d_anchors; unsigned* d_bits = nullptr; int* d_stamp = nullptr; unsigned* d_removed = nullptr; unsigned* d_runs = nullptr;
    RTO_HIP(c, d_anchors.upload(scratch, anchors, n, s));
    RTO_HIP(c, scratch.alloc(&d_bits, 3 * (size_t)D.words));            // X, M, A
    RTO_HIP(c, scratch.alloc(&d_stamp, tiles));
    RTO_HIP(c, scratch.alloc(&d_removed, (size_t)kMaxLook));
    RTO_HIP(c, scratch.alloc(&d_runs, tiles));
    unsigned* d_X = d_bits; unsigned* d_M = d_bits + D.words; unsigned* d_A = d_bits + 2 * (size_t)D.words;
    RTO_HIP(c, events.record(0, s));
    RTO_HIP(c, hipMemsetAsync(d_A, 0, (size_t)D.words * sizeof(unsigned), s));
    RTO_HIP(c, hipMemsetAsync(d_stamp, 0, tiles * sizeof(int), s));
    RTO_HIP(c, hipMemsetAsync(d_runs, 0, tiles * sizeof(unsigned), s));
    const dim3 b(kBlock), perWord((D.words + kBlock - 1) / kBlock);
    if (D.x % 32 == 0) hipLaunchKernelGGL(k_skel_init<true>, perWord, b, 0, s, c->d_vox, D, setValue, d_X, d_out);
    else hipLaunchKernelGGL(k_skel_init<false>, perWord, b, 0, s, c->d_vox, D, setValue, d_X, d_out);
    RTO_HIP(c, hipGetLastError());
    const int rcAnchors = d_anchors.in_parts(c, [&](const long long* part, unsigned count) {
        hipLaunchKernelGGL(k_skel_anchors, dim3((count + kBlock - 1) / kBlock), b, 0, s, part, count, D, d_A);
    });
    if (rcAnchors != RTO_OK) return rcAnchors;
    RTO_HIP(c, events.record(1, s));
    // passes until one removes nothing (its word: did it remove a voxel); `look` of them between two looks (look_at_passes).
    // Every pass but the last removes a voxel: voxels + 1 passes at most.
    const int64_t cap = nvox + 1;
    const int64_t most = std::min<int64_t>(max_passes, cap);
    const int look = std::max(1, std::min(c->skelLook, kMaxLook));
    int64_t passes = 0, launches = 0, tilesRun = 0, flagSum = 0;        // flagSum: the words' sum, of no use for flags
    bool settled = false;
    while (!settled && passes < most) {
        const int launch = (int)std::min<int64_t>(look, most - passes);
        const int rcLook = look_at_passes(c, d_removed, launch, [&](int i, unsigned* cnt) -> int {
            const int pass = (int)(passes + i + 1);
            if (full) hipLaunchKernelGGL(k_skel_mark<true>, perWord, b, 0, s, d_X, d_A, D, d_M);
            else hipLaunchKernelGGL(k_skel_mark<false>, perWord, b, 0, s, d_X, d_A, D, d_M);
            RTO_HIP(c, hipGetLastError());
            for (int sub = 0; sub < 8; sub++) {
                const dim3 gr((unsigned)tiles);
                if (curve) hipLaunchKernelGGL((k_skel_step<true, true>), gr, b, 0, s, d_X, d_M, d_out, d_stamp, D, T.x, T.y, T.z, pass, sub, cnt, d_runs);
                else if (full) hipLaunchKernelGGL((k_skel_step<true, false>), gr, b, 0, s, d_X, d_M, d_out, d_stamp, D, T.x, T.y, T.z, pass, sub, cnt, d_runs);
                else hipLaunchKernelGGL((k_skel_step<false, false>), gr, b, 0, s, d_X, d_M, d_out, d_stamp, D, T.x, T.y, T.z, pass, sub, cnt, d_runs);
                RTO_HIP(c, hipGetLastError());
            }
            return RTO_OK;
        }, passes, flagSum, settled);
        if (rcLook != RTO_OK) return rcLook;
        launches += 9 * (int64_t)launch;
    }
    if (!settled && passes >= cap) return fail(c, RTO_E_INTERNAL, std::string(who) + ": the thinning did not end within voxels + 1 passes");
    RTO_HIP(c, events.record(2, s));
    RTO_HIP(c, hipStreamSynchronize(s));
    for (int i = 0; i < 2; i++) RTO_HIP(c, events.elapsed(i, i + 1, &run.ms[i]));
    {
        std::vector<unsigned> perTile(tiles);
        RTO_HIP(c, hipMemcpyAsync(perTile.data(), d_runs, tiles * sizeof(unsigned), hipMemcpyDeviceToHost, s));
        RTO_HIP(c, hipStreamSynchronize(s));
        for (const unsigned r : perTile) tilesRun += r;
    }
    run.launches = launches;
    run.tilesRun = tilesRun;
    return RTO_OK;
}

}  // namespace

extern "C" {

int rto_skeleton_field(rto_context* c, int set, int connectivity, int mode, const int64_t* anchors, int64_t n, int64_t max_passes,
                       rto_skel_summary* summary) {
    using namespace rto;
    if (!c) return RTO_E_INVALID;
    const int rcArgs = skel_check_args(c, "rto_skeleton_field", set, connectivity, mode, anchors, n, max_passes);
    if (rcArgs != RTO_OK) return rcArgs;
    FieldDraft draft(c, kFieldSkeleton);
    const int rcDraft = draft.begin();
    if (rcDraft != RTO_OK) return rcDraft;
    SkelRun run;
    const int rc = skel_thin(c, "rto_skeleton_field", set, connectivity, mode, anchors, n, max_passes, draft.d, run);
    if (rc != RTO_OK) return rc;
    float summaryMs = -1.f;
    if (summary) {
        const unsigned nvox = (unsigned)grid_voxels(c);
        unsigned long long red[3] = { 0ull, 0ull, 0ull };
        const int rcSum = reduce_words(c, [&](unsigned long long* d_red) {
            const unsigned blocks = std::min<unsigned>((nvox + kBlock - 1) / kBlock, 4096u);
            hipLaunchKernelGGL(k_skel_summary, dim3(blocks), dim3(kBlock), 0, c->stream, draft.d, nvox, d_red);
        }, red, &summaryMs);
        if (rcSum != RTO_OK) return rcSum;
        summary->kept = (int64_t)red[0];
        summary->removed = (int64_t)red[1];
        summary->passes = (int64_t)red[2];
        summary->reserved = 0;
    }
    draft.publish();
    c->skelSet = set; c->skelConn = connectivity; c->skelMode = mode;
    c->skelLaunches = run.launches; c->skelTilesRun = run.tilesRun;
    c->skelMs[0] = run.ms[0]; c->skelMs[1] = run.ms[1]; c->skelMs[2] = summaryMs;
    return RTO_OK;
}

int rto_download_skeleton(rto_context* c, int32_t* out, int64_t capacity) { return download_field(c, "rto_download_skeleton", kFieldSkeleton, out, capacity); }

int rto_skeleton_device(rto_context* c, int32_t** d_k) { return field_device(c, "rto_skeleton_device", kFieldSkeleton, d_k); }

int rto_last_skeleton_ms(const rto_context* c, float ms[3]) { return copy_last_ms(c, &rto_context::skelMs, ms); }

int rto_debug_skeleton_passes(const rto_context* c, int64_t* launches, int64_t* tiles_run) {
    if (!c || !launches) return RTO_E_INVALID;
    *launches = c->skelLaunches;
    if (tiles_run) *tiles_run = c->skelTilesRun;
    return RTO_OK;
}

int rto_debug_set_skeleton_look(rto_context* c, int passes_per_look) {
    if (!c) return RTO_E_INVALID;
    if (passes_per_look < 1 || passes_per_look > kMaxLook) return fail(c, RTO_E_INVALID, "rto_debug_set_skeleton_look: 1 to 64 passes per look");
    c->skelLook = passes_per_look;
    return RTO_OK;
}

int rto_edit_skeleton(rto_context* c, int set, int connectivity, int mode, const int64_t* anchors, int64_t n, int64_t max_passes, int64_t* changed) {
    using namespace rto;
    if (!c) return RTO_E_INVALID;
    if (changed) *changed = 0;
    const int rcArgs = skel_check_args(c, "rto_edit_skeleton", set, connectivity, mode, anchors, n, max_passes);
    if (rcArgs != RTO_OK) return rcArgs;
    return edit_by_field(
        c, c->skelEditMs, changed,
        [&](int* d_field) {
            SkelRun run;
            return skel_thin(c, "rto_edit_skeleton", set, connectivity, mode, anchors, n, max_passes, d_field, run);
        },
        [&](const int* d_field, unsigned nvox, unsigned blocks, unsigned long long* d_count) {
            hipLaunchKernelGGL(k_skel_flip, dim3(blocks), dim3(kBlock), 0, c->stream, c->d_vox, d_field, nvox, set == RTO_SET_SOLID ? 0u : 1u, d_count);
        });
}

int rto_last_skeleton_edit_ms(const rto_context* c, float ms[3]) { return copy_last_ms(c, &rto_context::skelEditMs, ms); }

}  // extern "C"
