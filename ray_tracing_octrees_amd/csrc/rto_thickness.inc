// rto_thickness.inc -- local thickness fields of the resident grid (include/rto_hip.h, rto_thickness_field): at every voxel of a
// medium (the FILLED or the EMPTY voxels) the squared radius of the largest ball that fits inside the medium and contains the
// voxel, for balls of squared radius up to c <= 64, kept resident as one int32 per voxel with its histogram.  Included at the end
// of rto_api.hip, after rto_distance.inc, whose transform it runs.
//
// Rule (DESIGN.md section 21).  Voxel (i, j, k) has linear index v = i + dimX (j + dimY k).  D[q] = min(d2 from q to the nearest
// voxel of the other set, c), 0 outside the medium; t2[p] = max{ D[q] : (p - q)^2 < D[q] } for p in the medium, 0 elsewhere.
//
// (1) dt_transform (rto_distance.inc) makes a private field with set = the complement of the medium and cap = c; (2) k_thick_gather,
// one workgroup per 32 x 8 x 8 tile, takes the maximum over the balls that cover each voxel from a copy of D in LDS, as bytes;
// (3) k_thick_summary makes the histogram and the arg-min.  Kernel boundaries are the only synchronisation between workgroups; no
// lane reads what another lane of the same launch writes, except through LDS across a __syncthreads().

namespace rto {

constexpr int kThickMaxC = RTO_THICK_MAX_C;               // c <= 64: D fits a byte
constexpr int kThickMaxHalo = 7;                         // isqrt(kThickMaxC - 1): how far a ball that covers a voxel can be centred
constexpr int kThickLds = (kCcTileX + 2 * kThickMaxHalo) * (kCcTileY + 2 * kThickMaxHalo) * (kCcTileZ + 2 * kThickMaxHalo);   // 46 x 22 x 22
constexpr int kThickPerThread = kCcTileVox / kBlock;     // a thread's voxels: a column of the tile along z
constexpr int kThickTabHead = 68;                        // ints in front of the offsets: first[0 .. c], then padding to a 16-byte boundary
static_assert(kThickMaxHalo * kThickMaxHalo < kThickMaxC && (kThickMaxHalo + 1) * (kThickMaxHalo + 1) >= kThickMaxC, "the halo is isqrt(c - 1)");
static_assert(kThickPerThread == kCcTileZ && kBlock == kCcTileX * kCcTileY, "thread t owns column (t % 32, t / 32) of the tile");
static_assert(kThickTabHead % 4 == 0 && kThickTabHead >= kThickMaxC + 1, "the offsets start on a 16-byte boundary behind first[]");

// ---- the gather.  Thread t owns the 8 voxels (t % 32, t / 32, 0 .. 7) of the tile: the 32 lanes of a half-wave read 32
// consecutive bytes of one LDS row at every step (at most 9 words, each on a bank of its own), and a wave writes two rows of 32
// consecutive int32.  A tile whose own voxels all hold 0 or c is written straight out, before the halo is even loaded.
// tab: first[s], s = 0 .. c, in units of four offsets, then from tab + kThickTabHead the LDS byte offsets (dz sy + dy) sx + dx of
// the grid offsets o with o^2 = s, shell after shell, every shell padded to a multiple of four with the offset 0 (which tests the
// voxel's own D again and so changes nothing).  Every index into tab is wave-uniform.
__global__ __launch_bounds__(kBlock) void k_thick_gather(const int* __restrict__ d2, CcDims D, int tilesX, int tilesY, int c, int h,
                                                        const int* __restrict__ tab, int* __restrict__ out) {
    __shared__ uint8_t B[kThickLds];                      // min(d2, c) of the tile and its halo of h voxels; 0 outside the grid
    const int t = (int)threadIdx.x;
    const unsigned bid = blockIdx.x;
    const int x0 = (int)(bid % (unsigned)tilesX) * kCcTileX, y0 = (int)((bid / (unsigned)tilesX) % (unsigned)tilesY) * kCcTileY,
              z0 = (int)(bid / ((unsigned)tilesX * (unsigned)tilesY)) * kCcTileZ;
    const int lx = t % kCcTileX, ly = t / kCcTileX;
    const int gx = x0 + lx, gy = y0 + ly;
    const bool inXY = gx < D.x && gy < D.y;
    const size_t plane = (size_t)D.x * (size_t)D.y;
    const size_t col = (size_t)gy * (size_t)D.x + (size_t)gx;
    int own[kThickPerThread];
    bool work = false;
#pragma unroll
    for (int j = 0; j < kThickPerThread; j++) {
        own[j] = 0;
        if (inXY && z0 + j < D.z) own[j] = min(d2[(size_t)(z0 + j) * plane + col], c);
        work = work || (own[j] > 0 && own[j] < c);
    }
    if (!__syncthreads_or(work ? 1 : 0)) {                              // nothing to look for: every voxel holds 0 or c
#pragma unroll
        for (int j = 0; j < kThickPerThread; j++)
            if (inXY && z0 + j < D.z) out[(size_t)(z0 + j) * plane + col] = own[j];
        return;
    }
    const int sx = kCcTileX + 2 * h, sy = kCcTileY + 2 * h, sz = kCcTileZ + 2 * h;     // h <= kThickMaxHalo: sx sy sz <= kThickLds
    const int slab = sx * sy, total = slab * sz;
    int m = 0;
    for (int i = t; i < total; i += kBlock) {
        const int bz = i / slab, r = i - bz * slab, by = r / sx, bx = r - by * sx;
        const int x = x0 - h + bx, y = y0 - h + by, z = z0 - h + bz;
        int v = 0;
        if (x >= 0 && x < D.x && y >= 0 && y < D.y && z >= 0 && z < D.z) v = min(d2[(size_t)z * plane + (size_t)y * (size_t)D.x + (size_t)x], c);
        B[i] = (uint8_t)v;
        m = max(m, v);
    }
    // the largest D of the block: no ball in reach is larger (the barrier of the maximum is also the one after which B is read)
    const int M = __builtin_amdgcn_readfirstlane(block_max<kBlock>(m));
    const int lim = min(c, M);                                          // an offset with o^2 >= M is inside no ball
    int at[kThickPerThread], best[kThickPerThread];
#pragma unroll
    for (int j = 0; j < kThickPerThread; j++) {
        at[j] = ((j + h) * sy + (ly + h)) * sx + lx + h;
        best[j] = own[j];
    }
    const int4* __restrict__ offs = reinterpret_cast<const int4*>(tab + kThickTabHead);
    for (int s = 0; s < lim; s++) {                                     // shells of offsets in ascending o^2 = s: at most c of them
        bool pending = false;
#pragma unroll
        for (int j = 0; j < kThickPerThread; j++) pending = pending || (own[j] > 0 && own[j] < c && best[j] < M);
        if (!__any(pending ? 1 : 0)) break;                             // every voxel of this wave has its answer
        const int e1 = tab[s + 1];
        for (int e = tab[s]; e < e1; e++) {
            const int4 q = offs[e];
            const int o[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
            for (int k = 0; k < 4; k++) {
#pragma unroll
                for (int j = 0; j < kThickPerThread; j++) {
                    const int v = (int)B[at[j] + o[k]];                 // inside the block: |dx|, |dy|, |dz| <= h
                    best[j] = max(best[j], v > s ? v : 0);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kThickPerThread; j++)
        if (inXY && z0 + j < D.z) out[(size_t)(z0 + j) * plane + col] = own[j] > 0 ? best[j] : 0;
}

// ---- summary: the histogram of the values 1 .. c (LDS atomics; the value c, which nearly every voxel of a thick part holds, is
// counted in a register and added once per wave; then one global atomic per non-empty bin per workgroup) and the smallest value
// with the smallest voxel that holds it, as one min over the key (t2 << 32) | v: k_dt_summary's packing, turned round.
__global__ __launch_bounds__(kBlock) void k_thick_summary(const int* __restrict__ t2, unsigned n, int c, unsigned long long* __restrict__ bins,
                                                         unsigned long long* __restrict__ key) {
    __shared__ unsigned hist[kThickMaxC + 1];
    __shared__ unsigned long long waveBest[kBlock / kWave];
    if (threadIdx.x <= (unsigned)kThickMaxC) hist[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned base = blockIdx.x * (unsigned)kDtChunk;
    unsigned long long best = ~0ull;
    unsigned full = 0u;
#pragma unroll 4
    for (int j = 0; j < kDtPerThread; j++) {
        const unsigned v = base + (unsigned)j * kBlock + threadIdx.x;
        if (v < n) {
            const int d = t2[v];
            if (d > 0 && d <= c) {
                const unsigned long long k = ((unsigned long long)(unsigned)d << 32) | (unsigned long long)v;
                best = k < best ? k : best;
                if (d == c) full++;
                else atomicAdd(&hist[d], 1u);
            }
        }
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off);
        best = o < best ? o : best;
        full += __shfl_xor(full, off);
    }
    if ((threadIdx.x % kWave) == 0) {
        waveBest[threadIdx.x / kWave] = best;
        if (full) atomicAdd(&hist[c], full);
    }
    __syncthreads();
    if (threadIdx.x <= (unsigned)c && hist[threadIdx.x]) atomicAdd(&bins[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
    if (threadIdx.x == 0) {
        unsigned long long b = ~0ull;
        for (int w = 0; w < kBlock / kWave; w++) b = waveBest[w] < b ? waveBest[w] : b;
        if (b != ~0ull) atomicMin(key, b);
    }
}

}  // namespace rto

namespace {

// The gather's table for cap c (halo h, LDS strides sx, sy): k_thick_gather's comment.
std::vector<int> thick_table(int c, int h, int sx, int sy) {
    std::vector<std::vector<int>> shells((size_t)c);
    for (int dz = -h; dz <= h; dz++)
        for (int dy = -h; dy <= h; dy++)
            for (int dx = -h; dx <= h; dx++) {
                const int s = dx * dx + dy * dy + dz * dz;
                if (s < c) shells[(size_t)s].push_back((dz * sy + dy) * sx + dx);
            }
    std::vector<int> tab((size_t)rto::kThickTabHead, 0);
    for (int s = 0; s < c; s++) {
        tab[(size_t)s] = (int)((tab.size() - (size_t)rto::kThickTabHead) / 4);
        tab.insert(tab.end(), shells[(size_t)s].begin(), shells[(size_t)s].end());
        while ((tab.size() - (size_t)rto::kThickTabHead) % 4) tab.push_back(0);
    }
    tab[(size_t)c] = (int)((tab.size() - (size_t)rto::kThickTabHead) / 4);
    return tab;
}

}  // namespace

extern "C" {

int rto_thickness_field(rto_context* c, int medium, float max_radius, rto_thick_summary* summary) {
    using namespace rto;
    if (!c) return RTO_E_INVALID;
    if (medium != RTO_SET_SOLID && medium != RTO_SET_EMPTY) return fail(c, RTO_E_INVALID, "rto_thickness_field: unknown medium");
    if (std::isnan(max_radius) || max_radius < 0.0f) return fail(c, RTO_E_INVALID, "rto_thickness_field: max_radius is NaN or negative");
    long long mq = 0;
    int cap = 1;
    if (c->numNodes > 0) {                                              // without an octree there is no voxelSize to measure in
        if (!dt_quantize(max_radius, c->voxelSize, mq, cap))
            return fail(c, RTO_E_INVALID, "rto_thickness_field: max_radius is beyond 2^28 quanta of voxelSize / 64");
        if (cap == 0) return fail(c, RTO_E_INVALID, "rto_thickness_field: max_radius is under one voxel");
        if (cap > kThickMaxC) return fail(c, RTO_E_UNSUPPORTED, "rto_thickness_field: max_radius is above 8 voxels");
    }
    const int rcGrid = dt_check_grid(c, "rto_thickness_field");
    if (rcGrid != RTO_OK) return rcGrid;
    FieldDraft draft(c, kFieldThickness);
    const int rcDraft = draft.begin();
    if (rcDraft != RTO_OK) return rcDraft;
    hipStream_t s = c->stream;
    const CcDims D{ c->voxDim[0], c->voxDim[1], c->voxDim[2], (unsigned)grid_voxels(c) };
    const unsigned n = D.n;
    int h = 0;
    while ((h + 1) * (h + 1) < cap) h++;                                // isqrt(cap - 1)
    const CcTiles T(c->voxDim);
    // The offset table depends on c alone: the context keeps the one of the last c, and a call at the same c uploads nothing.
    // A new one is the call's own until the call has succeeded, like the field.
    struct TabGuard { int* p; ~TabGuard() { (void)hipFree(p); } } newTab{ nullptr };
    if (c->thickTabCap != cap) {
        const std::vector<int> tab = thick_table(cap, h, kCcTileX + 2 * h, kCcTileY + 2 * h);
        RTO_HIP(c, hipMalloc(&newTab.p, tab.size() * sizeof(int)));
        RTO_HIP(c, hipMemcpy(newTab.p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    const int* d_tab = newTab.p ? newTab.p : c->d_thickTab;
    float ms[3] = { -1.f, -1.f, -1.f };
    unsigned long long red[kThickMaxC + 2];
    {
        StreamEvents<3> events;
        RTO_HIP(c, events.create());
        BuildScratch scratch(s);
        int* d_D = nullptr;
        unsigned long long* d_red = nullptr;                            // the bins, then the key
        RTO_HIP(c, scratch.alloc(&d_D, (size_t)n));
        RTO_HIP(c, scratch.alloc(&d_red, (size_t)kThickMaxC + 2));
        float pass[3];
        const int rc = dt_transform(c, medium == RTO_SET_SOLID ? RTO_SET_EMPTY : RTO_SET_SOLID, cap, d_D, pass);
        if (rc != RTO_OK) return rc;
        ms[0] = pass[0] + pass[1] + pass[2];
        RTO_HIP(c, hipMemsetAsync(d_red, 0, ((size_t)kThickMaxC + 1) * sizeof(unsigned long long), s));
        RTO_HIP(c, hipMemsetAsync(d_red + kThickMaxC + 1, 0xff, sizeof(unsigned long long), s));
        RTO_HIP(c, events.record(0, s));
        hipLaunchKernelGGL(k_thick_gather, dim3((unsigned)T.count()), dim3(kBlock), 0, s, d_D, D, T.x, T.y, cap, h, d_tab, draft.d);
        RTO_HIP(c, hipGetLastError());
        RTO_HIP(c, events.record(1, s));
        hipLaunchKernelGGL(k_thick_summary, dim3((n + kDtChunk - 1) / kDtChunk), dim3(kBlock), 0, s, draft.d, n, cap, d_red, d_red + kThickMaxC + 1);
        RTO_HIP(c, hipGetLastError());
        RTO_HIP(c, events.record(2, s));
        RTO_HIP(c, hipMemcpyAsync(red, d_red, sizeof red, hipMemcpyDeviceToHost, s));
        RTO_HIP(c, hipStreamSynchronize(s));
        RTO_HIP(c, events.elapsed(0, 1, &ms[1]));
        RTO_HIP(c, events.elapsed(1, 2, &ms[2]));
    }
    int64_t mediumCount = 0, thin = 0;
    for (int t = 0; t <= cap; t++) { mediumCount += (int64_t)red[t]; if (t < cap) thin += (int64_t)red[t]; }
    if (summary) {
        const unsigned long long key = red[kThickMaxC + 1];
        summary->min_t2 = mediumCount ? (int64_t)(key >> 32) : -1;
        summary->argmin = mediumCount ? (int64_t)(key & 0xffffffffull) : -1;
        summary->thin = thin;
        summary->medium = mediumCount;
    }
    draft.publish();
    if (newTab.p) {
        (void)hipFree(c->d_thickTab);
        c->d_thickTab = newTab.p; c->thickTabCap = cap;
        c->thickTabBuilds++;
        newTab.p = nullptr;
    }
    c->thickMedium = medium; c->thickCap = cap;
    for (int t = 0; t <= kThickMaxC; t++) c->thickBins[t] = t <= cap ? (int64_t)red[t] : 0;
    for (int i = 0; i < 3; i++) c->thickMs[i] = ms[i];
    return RTO_OK;
}

int rto_download_thickness(rto_context* c, int32_t* out, int64_t capacity) { return download_field(c, "rto_download_thickness", kFieldThickness, out, capacity); }

int rto_thickness_device(rto_context* c, int32_t** d_t2) { return field_device(c, "rto_thickness_device", kFieldThickness, d_t2); }

int rto_thickness_histogram(rto_context* c, int64_t* out, int64_t capacity, int64_t* bins) {
    if (!c) return RTO_E_INVALID;
    const int rcField = resident_field_check(c, "rto_thickness_histogram", kFieldThickness);
    if (rcField != RTO_OK) return rcField;
    if (out && capacity < (int64_t)c->thickCap + 1) return fail(c, RTO_E_INVALID, "rto_thickness_histogram: capacity is below c + 1");
    if (bins) *bins = (int64_t)c->thickCap + 1;
    if (out) for (int t = 0; t <= c->thickCap; t++) out[t] = c->thickBins[t];
    return RTO_OK;
}

int rto_debug_thickness_table(const rto_context* c, int* table_c, int64_t* built) {
    if (!c) return RTO_E_INVALID;
    if (table_c) *table_c = c->thickTabCap;
    if (built) *built = c->thickTabBuilds;
    return RTO_OK;
}

int rto_last_thickness_ms(const rto_context* c, float ms[3]) { return copy_last_ms(c, &rto_context::thickMs, ms); }

}  // extern "C"
