// rto_distance.inc -- distance fields of the resident grid (include/rto_hip.h, rto_distance_field / rto_edit_morphology): the exact
// squared Euclidean distance, in voxel-index units, from every voxel to the nearest voxel of a set (the FILLED or the EMPTY voxels),
// kept resident as one int32 per voxel, and the morphology that is a threshold on it: dilate, erode, open, close, with the voxel
// edits' rebuild.  Included at the end of rto_api.hip.
//
// Rule (DESIGN.md section 19).  Voxel (i, j, k) has linear index v = i + dimX (j + dimY k).  d2[v] = min over the voxels u of the
// set of (i_v - i_u)^2 + (j_v - j_u)^2 + (k_v - k_u)^2; kDtNone where the set is empty or the voxel is out of reach of the cap.
//
// The transform is separable: a min over x, then over y, then over z of f[j] + (i - j)^2 is exact in integers.  (1) k_dt_x turns
// every row into occupancy bit masks in LDS and takes each voxel's nearest set bit to the left and to the right from the mask
// words; (2, 3) k_dt_axis<1> and k_dt_axis<2> run the lower envelope of parabolas (Meijster) down every y and every z column, one
// lane per column, in place; (4) k_dt_summary reduces the volume.
// A value beyond the cap is replaced by kDtNone after every pass: the passes only ever add non-negative terms, so such a value can
// take part in no sum that is in reach.  Kernel boundaries are the only synchronisation between workgroups; no lane reads what
// another lane of the same launch writes, except through LDS across a __syncthreads() in k_dt_x.

namespace rto {

constexpr int kDtNone = 0x7fffffff;                      // RTO_DIST_NONE
constexpr int kDtMaxDim = 46341;                         // (dim - 1)^2 < 2^31 - 1: the largest dimension rto_distance_field accepts
constexpr int kDtMaskWords = 2048;                       // LDS mask words of one k_dt_x workgroup: its rows' bits
constexpr int kDtRowVox = 2048;                          // voxels one k_dt_x workgroup owns at most, unless a single row is longer
constexpr unsigned kDtNoBit = 0xffffu;                   // "no set bit on this side": positions are below 46341
constexpr int kDtPerThread = 16;                         // voxels per thread of the streaming kernels
constexpr int kDtChunk = kBlock * kDtPerThread;
static_assert((kDtMaxDim + 31) / 32 <= kDtMaskWords, "one row's mask fits the LDS array");
static_assert(kDtMaxDim < (int)kDtNoBit, "positions fit 16 bits");

// ---- pass 1: rows.  A workgroup owns `rowsPerBlock` consecutive rows (a contiguous stretch of the volume): rowsPerBlock * rowWords
// <= kDtMaskWords.  WIDE: dimX % 16 == 0, so every row starts on a 16-byte boundary: 16-byte loads, and four voxels of one mask
// word per thread with one 16-byte store.
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void k_dt_x(const uint8_t* __restrict__ vox, CcDims D, int rowsPerBlock, int rowWords, unsigned numRows,
                                                unsigned setValue, int cap, int* __restrict__ out) {
    __shared__ unsigned mask[kDtMaskWords];                 // bit b of word w of row r: voxel 32 w + b of that row is in the set
    __shared__ unsigned short leftOf[kDtMaskWords];         // the nearest set bit of the row before word w, kDtNoBit: none
    __shared__ unsigned short rightOf[kDtMaskWords];        // the nearest one after it
    const unsigned row0 = blockIdx.x * (unsigned)rowsPerBlock;
    const int rows = (int)min((unsigned)rowsPerBlock, numRows - row0);
    const int words = rows * rowWords;
    const size_t base = (size_t)row0 * (size_t)D.x;
    for (int i = (int)threadIdx.x; i < words; i += kBlock) {           // at most kDtMaskWords / kBlock rounds
        const int r = i / rowWords, w = i - r * rowWords;
        const int x0 = 32 * w;
        const uint8_t* p = vox + base + (size_t)r * (size_t)D.x + x0;
        unsigned m = 0u;
        if (WIDE) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                if (x0 + 16 * h < D.x) {                                // a 16-byte piece is wholly inside the row or outside
                    const uint4 q = *reinterpret_cast<const uint4*>(p + 16 * h);
                    const unsigned ws[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
                    for (int j = 0; j < 16; j++) m |= (((ws[j >> 2] >> (8 * (j & 3))) & 0xffu) == setValue ? 1u : 0u) << (16 * h + j);
                }
            }
        } else {
#pragma unroll 8
            for (int j = 0; j < 32; j++)
                if (x0 + j < D.x) m |= ((unsigned)p[j] == setValue ? 1u : 0u) << j;
        }
        mask[i] = m;
    }
    __syncthreads();
    for (int r = (int)threadIdx.x; r < rows; r += kBlock) {            // one thread per row: two sweeps of rowWords steps
        unsigned last = kDtNoBit;
        for (int w = 0; w < rowWords; w++) {
            leftOf[r * rowWords + w] = (unsigned short)last;
            const unsigned m = mask[r * rowWords + w];
            if (m) last = (unsigned)(32 * w + 31 - __clz((int)m));
        }
        last = kDtNoBit;
        for (int w = rowWords - 1; w >= 0; w--) {
            rightOf[r * rowWords + w] = (unsigned short)last;
            const unsigned m = mask[r * rowWords + w];
            if (m) last = (unsigned)(32 * w + __ffs((int)m) - 1);
        }
    }
    __syncthreads();
    constexpr int V = WIDE ? 4 : 1;
    const int count = rows * D.x / V;                                   // rows * dimX <= max(kDtRowVox, kDtMaxDim)
    for (int e = (int)threadIdx.x; e < count; e += kBlock) {
        const int r = (e * V) / D.x, x = e * V - r * D.x;
        const int w = x >> 5, wi = r * rowWords + w;
        const unsigned m = mask[wi];
        const unsigned lo = leftOf[wi], ro = rightOf[wi];
        int vals[V];
#pragma unroll
        for (int j = 0; j < V; j++) {
            const int xx = x + j, b = xx & 31;
            const unsigned ml = m & (0xffffffffu >> (31 - b)), mr = m & (0xffffffffu << b);
            const unsigned pl = ml ? (unsigned)(32 * w + 31 - __clz((int)ml)) : lo;
            const unsigned pr = mr ? (unsigned)(32 * w + __ffs((int)mr) - 1) : ro;
            const unsigned dl = pl == kDtNoBit ? kDtNoBit : (unsigned)xx - pl, dr = pr == kDtNoBit ? kDtNoBit : pr - (unsigned)xx;
            const unsigned d = min(dl, dr);                            // < 46341, or kDtNoBit
            vals[j] = d != kDtNoBit && d * d <= (unsigned)cap ? (int)(d * d) : kDtNone;
        }
        int* dst = out + base + (size_t)e * V;
        if (WIDE) *reinterpret_cast<int4*>(dst) = make_int4(vals[0], vals[V > 1 ? 1 : 0], vals[V > 2 ? 2 : 0], vals[V > 3 ? 3 : 0]);
        else dst[0] = vals[0];
    }
}

// ---- passes 2 and 3: columns, the general form.  One lane per column: AXIS 1 walks y (stride dimX; the columns are the (x, z)
// pairs), AXIS 2 walks z (stride dimX dimY; the columns are the (x, y) pairs), x fastest across lanes, so every lane of a wave
// reads and writes the same step of neighbouring columns.  The lower envelope of the parabolas f[s] + (u - s)^2, Meijster's form:
// a stack of (s, t, f[s]) where parabola s is the lowest from u = t on.  The top of the stack lives in registers; the entries below
// it live in the scratch volumes stPos / stVal at the column's own addresses (entry q where voxel q of the column is): at most n
// entries, because a step pushes at most one.  kDtNone entries are never pushed.  The forward sweep takes n steps and pops at most
// what it pushed (<= 2 n steps), the backward sweep n steps and at most n pops.  The volume is transformed in place: the forward
// sweep has read all of the column before the backward sweep writes any of it.
template <int AXIS>
__global__ __launch_bounds__(kBlock) void k_dt_axis(int* __restrict__ f, CcDims D, unsigned cols, int cap, unsigned* __restrict__ stPos,
                                                   int* __restrict__ stVal) {
    const unsigned c = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    if (c >= cols) return;
    const int n = AXIS == 1 ? D.y : D.z;
    const size_t stride = AXIS == 1 ? (size_t)D.x : (size_t)D.x * (size_t)D.y;
    const size_t base = AXIS == 1 ? (size_t)(c % (unsigned)D.x) + (size_t)(c / (unsigned)D.x) * (size_t)D.x * (size_t)D.y : (size_t)c;
    int depth = 0;                    // entries on the stack, the top included
    int tp = 0, tb = 0, tv = 0;       // the top: position, the step from which it is the lowest, its value
    for (int u = 0; u < n; u++) {
        const int g = f[base + (size_t)u * stride];
        if (g == kDtNone) continue;
        while (depth > 0) {                                            // at most `depth` <= u rounds: every round pops
            const long long a = (long long)(tb - tp) * (tb - tp) + tv, b = (long long)(tb - u) * (tb - u) + g;
            if (a <= b) break;
            depth--;
            if (depth > 0) {
                const size_t at = base + (size_t)(depth - 1) * stride;
                const unsigned pb = stPos[at];
                tp = (int)(pb & 0xffffu); tb = (int)(pb >> 16); tv = stVal[at];
            }
        }
        if (depth == 0) { tp = u; tb = 0; tv = g; depth = 1; }
        else {
            // the first step at which u is lower than the top: 1 + floor((u^2 - tp^2 + g - tv) / (2 (u - tp))); the quotient is at
            // least tb >= 0 (the top survived the loop above), so the numerator is not negative and truncation is the floor
            const long long num = (long long)u * u - (long long)tp * tp + (long long)g - (long long)tv;
            const long long w = 1 + num / (long long)(2 * (u - tp));
            if (w < (long long)n) {
                const size_t at = base + (size_t)(depth - 1) * stride;
                stPos[at] = (unsigned)tp | ((unsigned)tb << 16); stVal[at] = tv;
                tp = u; tb = (int)w; tv = g; depth++;
            }
        }
    }
    for (int u = n - 1; u >= 0; u--) {
        int val = kDtNone;
        if (depth > 0) {
            const long long d = (long long)(u - tp) * (u - tp) + tv;
            if (d <= (long long)cap) val = (int)d;
            if (u == tb) {
                depth--;
                if (depth > 0) {
                    const size_t at = base + (size_t)(depth - 1) * stride;
                    const unsigned pb = stPos[at];
                    tp = (int)(pb & 0xffffu); tb = (int)(pb >> 16); tv = stVal[at];
                }
            }
        }
        f[base + (size_t)u * stride] = val;
    }
}

// ---- summary: the largest finite value and the smallest voxel that holds it, as one max over the key (d2 << 32) | ~v (a smaller
// v is a larger key; every real key is above 0 because v < 2^31), and the number of finite values: one 64-bit atomic max and one
// 64-bit atomic add per workgroup.
__global__ __launch_bounds__(kBlock) void k_dt_summary(const int* __restrict__ d2, unsigned n, unsigned long long* __restrict__ key,
                                                      unsigned long long* __restrict__ finite) {
    const unsigned base = blockIdx.x * (unsigned)kDtChunk;
    unsigned long long best = 0ull;
    unsigned count = 0u;
#pragma unroll 4
    for (int j = 0; j < kDtPerThread; j++) {
        const unsigned v = base + (unsigned)j * kBlock + threadIdx.x;
        if (v < n) {
            const int d = d2[v];
            if (d != kDtNone) {
                const unsigned long long k = ((unsigned long long)(unsigned)d << 32) | (unsigned long long)(~v);
                best = k > best ? k : best;
                count++;
            }
        }
    }
    struct __attribute__((packed, aligned(4))) DtBest { unsigned long long key; unsigned count; };      // 12 bytes: three words a wave in LDS
    const DtBest all = block_reduce<kBlock>(DtBest{ best, count }, [](DtBest a, const DtBest& b) {
        a.key = b.key > a.key ? b.key : a.key; a.count += b.count;
        return a;
    });
    if (threadIdx.x == 0 && all.count) { atomicMax(key, all.key); atomicAdd(finite, (unsigned long long)all.count); }
}

// ---- morphology: the threshold.  Every voxel equal to `from` whose field value is finite (in reach of the cap the field was made
// with) takes `to`.  A thread owns 16 consecutive voxels (WIDE: n % 16 == 0, one 16-byte store when anything changed).  The count
// is of voxels whose value now differs from `orig` (the grid before the call; nullptr: the grid before this launch):
// block_add_count.
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void k_morph_flip(uint8_t* __restrict__ vox, const int* __restrict__ d2, const uint8_t* __restrict__ orig,
                                                      unsigned n, unsigned from, unsigned to, unsigned long long* __restrict__ changed) {
    const unsigned v0 = (blockIdx.x * (unsigned)kBlock + threadIdx.x) * (unsigned)kCcVec;
    int count = 0;
    if (v0 < n) {
        if (WIDE) {
            unsigned hit = 0u;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int4 d = *reinterpret_cast<const int4*>(d2 + v0 + 4 * q);
                const int ds[4] = { d.x, d.y, d.z, d.w };
#pragma unroll
                for (int j = 0; j < 4; j++) hit |= (ds[j] != kDtNone ? 1u : 0u) << (4 * q + j);
            }
            if (hit || orig) {
                const uint4 w = *reinterpret_cast<const uint4*>(vox + v0);
                unsigned words[4] = { w.x, w.y, w.z, w.w };
                unsigned was[4] = { w.x, w.y, w.z, w.w };
                if (orig) {
                    const uint4 o = *reinterpret_cast<const uint4*>(orig + v0);
                    was[0] = o.x; was[1] = o.y; was[2] = o.z; was[3] = o.w;
                }
                bool wrote = false;
#pragma unroll
                for (int j = 0; j < kCcVec; j++) {
                    const unsigned sh = 8u * (unsigned)(j & 3);
                    if (((hit >> j) & 1u) && ((words[j >> 2] >> sh) & 0xffu) == from) {
                        words[j >> 2] = (words[j >> 2] & ~(0xffu << sh)) | (to << sh);
                        wrote = true;
                    }
                    count += ((words[j >> 2] >> sh) & 0xffu) != ((was[j >> 2] >> sh) & 0xffu) ? 1 : 0;
                }
                if (wrote) *reinterpret_cast<uint4*>(vox + v0) = make_uint4(words[0], words[1], words[2], words[3]);
            }
        } else {
            for (int j = 0; j < kCcVec && v0 + (unsigned)j < n; j++) {
                unsigned cur = vox[v0 + j];
                const unsigned was = orig ? (unsigned)orig[v0 + j] : cur;
                if (d2[v0 + j] != kDtNone && cur == from) { cur = to; vox[v0 + j] = (uint8_t)to; }
                count += cur != was ? 1 : 0;
            }
        }
    }
    block_add_count(count, changed);
}

}  // namespace rto

namespace {

constexpr double kDtQuantLimit = 268435456.0;            // 2^28: mq and rq, as section 17's max_dist

// The cap as the largest squared distance in reach: 4096 d2 <= mq^2 exactly when d2 <= floor(mq^2 / 4096).  +inf: no cap.
// false: NaN, negative, or beyond 2^28 quanta.
bool dt_quantize(float dist, float voxelSize, long long& mq, int& cap) {
    if (std::isinf(dist) && dist > 0.0f) { mq = -1; cap = rto::kDtNone - 1; return true; }
    const double a = (double)dist / (double)voxelSize;
    const double b = a * 64.0;
    const double f = std::floor(b + 0.5);
    if (!(f <= kDtQuantLimit && dist >= 0.0f)) return false;            // NaN fails both
    mq = (long long)f;
    const long long d2 = mq * mq / 4096;
    cap = (int)std::min<long long>(d2, (long long)rto::kDtNone - 1);
    return true;
}

int dt_check_grid(rto_context* c, const char* who) {
    const std::string w(who);
    const int rcGrid = resident_grid_check(c, who, "");
    if (rcGrid != RTO_OK) return rcGrid;
    int64_t diag = 0;
    for (int a = 0; a < 3; a++) diag += (int64_t)(c->voxDim[a] - 1) * (c->voxDim[a] - 1);
    if (diag >= 0x7fffffffll) return fail(c, RTO_E_UNSUPPORTED, w + ": the grid's diagonal squared does not fit the 32-bit field");
    return RTO_OK;
}

// The three passes into d_out (one int32 per voxel; arguments already checked).  ms: x, y, z pass.  The context is not touched.
int dt_transform(rto_context* c, int set, int cap, int* d_out, float ms[3]) {
    using namespace rto;
    const CcDims D{ c->voxDim[0], c->voxDim[1], c->voxDim[2], (unsigned)grid_voxels(c) };
    hipStream_t s = c->stream;
    StreamEvents<4> events;
    RTO_HIP(c, events.create());
    BuildScratch scratch(s);
    unsigned* d_stPos = nullptr; int* d_stVal = nullptr;
    RTO_HIP(c, scratch.alloc(&d_stPos, (size_t)D.n));
    RTO_HIP(c, scratch.alloc(&d_stVal, (size_t)D.n));
    const unsigned setValue = set == RTO_SET_SOLID ? 1u : 0u;
    RTO_HIP(c, events.record(0, s));
    {
        const int rowWords = (D.x + 31) / 32;
        const int rowsPerBlock = std::max(1, kDtRowVox / D.x);          // rowsPerBlock * rowWords <= kDtMaskWords (rowWords <= dimX)
        const unsigned numRows = (unsigned)D.y * (unsigned)D.z;
        const unsigned blocks = (numRows + (unsigned)rowsPerBlock - 1) / (unsigned)rowsPerBlock;
        if (D.x % kCcVec == 0) hipLaunchKernelGGL(k_dt_x<true>, dim3(blocks), dim3(kBlock), 0, s, c->d_vox, D, rowsPerBlock, rowWords, numRows, setValue, cap, d_out);
        else hipLaunchKernelGGL(k_dt_x<false>, dim3(blocks), dim3(kBlock), 0, s, c->d_vox, D, rowsPerBlock, rowWords, numRows, setValue, cap, d_out);
        RTO_HIP(c, hipGetLastError());
    }
    RTO_HIP(c, events.record(1, s));
    {
        const unsigned colsY = (unsigned)D.x * (unsigned)D.z, colsZ = (unsigned)D.x * (unsigned)D.y;
        hipLaunchKernelGGL(k_dt_axis<1>, dim3((colsY + kBlock - 1) / kBlock), dim3(kBlock), 0, s, d_out, D, colsY, cap, d_stPos, d_stVal);
        RTO_HIP(c, hipGetLastError());
        RTO_HIP(c, events.record(2, s));
        hipLaunchKernelGGL(k_dt_axis<2>, dim3((colsZ + kBlock - 1) / kBlock), dim3(kBlock), 0, s, d_out, D, colsZ, cap, d_stPos, d_stVal);
        RTO_HIP(c, hipGetLastError());
    }
    RTO_HIP(c, events.record(3, s));
    RTO_HIP(c, hipStreamSynchronize(s));
    for (int i = 0; i < 3; i++) RTO_HIP(c, events.elapsed(i, i + 1, &ms[i]));
    return RTO_OK;
}

// The summary of a distance-like field (one int32 per voxel, kDtNone where there is no value): k_dt_summary over it, decoded.
struct DtSummary {
    int64_t finite = 0;                // voxels that hold a value
    int64_t max = -1, argmax = -1;     // the largest value and the smallest voxel that holds it; -1: no voxel holds a value
    float ms = -1.f;                   // device time of the launch
};
int dt_summary(rto_context* c, const int* d_field, unsigned n, DtSummary& out) {
    using namespace rto;
    unsigned long long red[2] = { 0ull, 0ull };                         // the key, the count
    const int rc = reduce_words(c, [&](unsigned long long* d_red) {
        hipLaunchKernelGGL(k_dt_summary, dim3((n + kDtChunk - 1) / kDtChunk), dim3(kBlock), 0, c->stream, d_field, n, d_red, d_red + 1);
    }, red, &out.ms);
    if (rc != RTO_OK) return rc;
    out.finite = (int64_t)red[1];
    out.max = red[1] ? (int64_t)(red[0] >> 32) : -1;
    out.argmax = red[1] ? (int64_t)(~(unsigned)(red[0] & 0xffffffffull)) : -1;
    return RTO_OK;
}

}  // namespace

extern "C" {

int rto_distance_field(rto_context* c, int set, float max_dist, rto_dist_summary* summary) {
    using namespace rto;
    if (!c) return RTO_E_INVALID;
    if (set != RTO_SET_SOLID && set != RTO_SET_EMPTY) return fail(c, RTO_E_INVALID, "rto_distance_field: unknown set");
    if (std::isnan(max_dist) || max_dist < 0.0f) return fail(c, RTO_E_INVALID, "rto_distance_field: max_dist is NaN or negative");
    long long mq = 0;
    int cap = 0;
    if (c->numNodes > 0 && !dt_quantize(max_dist, c->voxelSize, mq, cap))           // without an octree there is no voxelSize to measure in
        return fail(c, RTO_E_INVALID, "rto_distance_field: max_dist is beyond 2^28 quanta of voxelSize / 64");
    const int rcGrid = dt_check_grid(c, "rto_distance_field");
    if (rcGrid != RTO_OK) return rcGrid;
    FieldDraft draft(c, kFieldDistance);
    const int rcDraft = draft.begin();
    if (rcDraft != RTO_OK) return rcDraft;
    float ms[4] = { -1.f, -1.f, -1.f, -1.f };
    const int rc = dt_transform(c, set, cap, draft.d, ms);
    if (rc != RTO_OK) return rc;
    if (summary) {
        DtSummary sum;
        const int rcSum = dt_summary(c, draft.d, (unsigned)grid_voxels(c), sum);
        if (rcSum != RTO_OK) return rcSum;
        ms[3] = sum.ms;
        summary->finite = sum.finite;
        summary->max_d2 = sum.max;
        summary->argmax = sum.argmax;
        summary->reserved = 0;
    }
    draft.publish();
    for (int i = 0; i < 4; i++) c->distMs[i] = ms[i];
    return RTO_OK;
}

int rto_download_distance(rto_context* c, int32_t* out, int64_t capacity) { return download_field(c, "rto_download_distance", kFieldDistance, out, capacity); }

int rto_distance_device(rto_context* c, int32_t** d_d2) { return field_device(c, "rto_distance_device", kFieldDistance, d_d2); }

int rto_last_distance_ms(const rto_context* c, float ms[4]) { return copy_last_ms(c, &rto_context::distMs, ms); }

int rto_edit_morphology(rto_context* c, int op, float radius, int64_t* changed) {
    using namespace rto;
    if (!c) return RTO_E_INVALID;
    if (changed) *changed = 0;
    if (op < RTO_MORPH_DILATE || op > RTO_MORPH_CLOSE) return fail(c, RTO_E_INVALID, "rto_edit_morphology: unknown op");
    if (std::isnan(radius) || radius < 0.0f) return fail(c, RTO_E_INVALID, "rto_edit_morphology: radius is NaN or negative");
    long long rq = 0;
    int cap = 0;
    if (c->numNodes > 0 && !dt_quantize(radius, c->voxelSize, rq, cap))
        return fail(c, RTO_E_INVALID, "rto_edit_morphology: radius is beyond 2^28 quanta of voxelSize / 64");
    const int rcGrid = dt_check_grid(c, "rto_edit_morphology");
    if (rcGrid != RTO_OK) return rcGrid;
    c->morphMs[0] = c->morphMs[1] = c->morphMs[2] = -1.f;
    if (rq == 0) return RTO_OK;                                         // nothing but the set itself is in reach
    RTO_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    RTO_HIP(c, hipStreamSynchronize(s));
    const unsigned n = (unsigned)grid_voxels(c);
    // DILATE grows the SOLID set into the EMPTY voxels in reach; ERODE grows the EMPTY set into the FILLED ones
    const int first = (op == RTO_MORPH_DILATE || op == RTO_MORPH_CLOSE) ? RTO_SET_SOLID : RTO_SET_EMPTY;
    const int steps = (op == RTO_MORPH_OPEN || op == RTO_MORPH_CLOSE) ? 2 : 1;
    unsigned long long count = 0;
    {
        StreamEvents<2> events;
        RTO_HIP(c, events.create());
        BuildScratch scratch(s);
        int* d_field = nullptr; uint8_t* d_orig = nullptr;
        ChangedCount d_count;
        RTO_HIP(c, scratch.alloc(&d_field, (size_t)n));
        RTO_HIP(c, d_count.alloc(scratch));
        RTO_HIP(c, events.record(0, s));
        RTO_HIP(c, scratch.alloc(&d_orig, (size_t)n));               // the grid before the call: what OPEN and CLOSE count against, and what an error restores
        RTO_HIP(c, hipMemcpyAsync(d_orig, c->d_vox, (size_t)n, hipMemcpyDeviceToDevice, s));
        const unsigned blocks = (unsigned)((((int64_t)n + kCcVec - 1) / kCcVec + kBlock - 1) / kBlock);
        for (int step = 0; step < steps; step++) {
            const int set = step == 0 ? first : (first == RTO_SET_SOLID ? RTO_SET_EMPTY : RTO_SET_SOLID);
            float ms[3];
            int rc = dt_transform(c, set, cap, d_field, ms);
            if (rc == RTO_OK) {
                const unsigned from = set == RTO_SET_SOLID ? 0u : 1u, to = set == RTO_SET_SOLID ? 1u : 0u;
                const uint8_t* orig = step == 0 ? nullptr : d_orig;
                hipError_t e = d_count.clear(s);
                if (e == hipSuccess) {
                    if (n % kCcVec == 0) hipLaunchKernelGGL(k_morph_flip<true>, dim3(blocks), dim3(kBlock), 0, s, c->d_vox, d_field, orig, n, from, to, d_count.d);
                    else hipLaunchKernelGGL(k_morph_flip<false>, dim3(blocks), dim3(kBlock), 0, s, c->d_vox, d_field, orig, n, from, to, d_count.d);
                    e = hipGetLastError();
                }
                if (e == hipSuccess) e = d_count.read(s, &count);
                if (e != hipSuccess) rc = fail(c, RTO_E_HIP, std::string("rto_edit_morphology: ") + hipGetErrorString(e));
            }
            if (rc != RTO_OK) {                                         // give the grid back as it was before the first step
                (void)hipMemcpyAsync(c->d_vox, d_orig, (size_t)n, hipMemcpyDeviceToDevice, s);
                (void)hipStreamSynchronize(s);
                return rc;
            }
        }
        RTO_HIP(c, events.record(1, s));
        RTO_HIP(c, hipStreamSynchronize(s));
        RTO_HIP(c, events.elapsed(0, 1, &c->morphMs[0]));
    }
    if (changed) *changed = (int64_t)count;
    if (count == 0) return RTO_OK;           // nothing is dropped: rebuild_from_resident_grid's comment

    return rebuild_from_resident_grid(c, c->d_triOffset != nullptr, &c->morphMs[1], &c->morphMs[2]);
}

int rto_last_morphology_ms(const rto_context* c, float ms[3]) { return copy_last_ms(c, &rto_context::morphMs, ms); }

}  // extern "C"
