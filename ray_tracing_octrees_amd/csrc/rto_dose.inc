// rto_dose.inc -- dose fields of the resident grid (include/rto_hip.h, rto_dose_field): for every evaluated EMPTY voxel the sum over
// point sources of the source's weight, attenuated by a table indexed with the number of SOLID voxels that the straight segment
// from the voxel's centre to the source's crosses and, if asked for, divided by the squared distance; kept resident as one int32
// per voxel (-1 for a voxel that is not evaluated) with one int64 per source that counts the voxels with a clear view of it.
// Included by rto_api.hip after rto_exposure.inc, whose bit rows, selection, ExDims and crossing rule this file uses as they are.
//
// Rule (DESIGN.md section 31).  d = s - p.  The planes of axis a are crossed at t = (2 m + 1) / (2 |d_a|), m = 0 .. |d_a| - 1; equal
// times of several axes are ONE step that moves on all of them (a segment through an edge or a corner enters neither cube it only
// touches); the last step arrives at s, which is not counted.  With d not primitive these are periods 0 .. g - 1 of section 25's
// template of d / g, without the last entry.  Both ends lie in the grid and every axis only moves from p towards s, so every voxel
// visited lies in the box the two span: no bounds test.
//
// (1) k_expo_bits and k_expo_select (rto_exposure.inc) make the SOLID bit rows and the list of evaluated voxels; e is filled with -1.
// (2) k_dose_march: one thread per listed voxel.  The loop over sources is wave-uniform and a source's record is read through a
// wave-uniform address; the transmission table sits in LDS.  Per pair each lane runs its own three-axis integer DDA: the next
// crossing time of every axis is kept over the COMMON denominator 2 a' b' c' (a' = max(|d_a|, 1)) as the 32-bit numerator
// (2 m + 1) b' c' <= 2,047 x 1,023^2 < 2^31, which is why the reach ends at 1,023; an axis with d_a = 0 holds 2^32 - 1 and never
// steps; an axis that has arrived holds (2 |d_a| + 1) b' c', above every time still to come.  After each source one ballot counts
// the wave's clear lanes and one lane adds them to covered[s].  e[v] is written once; a voxel that saw a source sets the top bit of
// its list entry (an index is below 2^31 - 1), which is all that k_dose_summary needs beside e.
// (3) k_dose_summary: total, dark, seen and the peak with its smallest index over the list.

namespace rto {

struct DoseArgs { int n, m, stop, falloff, reach; };               // stop: the k at which a pair may leave early (below)

constexpr unsigned kDoseSeenBit = 0x80000000u;

// ---- march.  One thread per listed voxel.  src[s] is the same for all lanes of a wave.
__global__ __launch_bounds__(kBlock) void k_dose_march(const unsigned* __restrict__ S, ExDims D, unsigned* __restrict__ list, unsigned count,
                                                      const int4* __restrict__ src, const unsigned* __restrict__ transmit, DoseArgs A,
                                                      unsigned long long* __restrict__ covered, int* __restrict__ e) {
    __shared__ unsigned T[RTO_DOSE_MAX_TABLE];
    if (threadIdx.x < RTO_DOSE_MAX_TABLE) T[threadIdx.x] = (int)threadIdx.x < A.m ? transmit[threadIdx.x] : 0u;
    __syncthreads();
    const unsigned i = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    const bool mine = i < count;
    const unsigned v = mine ? list[i] : 0u;
    const unsigned line = v / (unsigned)D.x;
    const int x = (int)(v % (unsigned)D.x), y = (int)(line % (unsigned)D.y), z = (int)(line / (unsigned)D.y);
    const unsigned wordsX = (unsigned)D.wordsX, plane = wordsX * (unsigned)D.y;
    const unsigned row0 = ((unsigned)z * (unsigned)D.y + (unsigned)y) * wordsX;
    unsigned sum = 0u;
    bool seen = false;
    for (int si = 0; si < A.n; si++) {
        const int4 q = src[si];
        const int dx = q.x - x, dy = q.y - y, dz = q.z - z;
        const int ax = abs(dx), ay = abs(dy), az = abs(dz);
        const int far = max(ax, max(ay, az));
        const bool in = mine && far <= A.reach;
        int k = 0;
        if (in && far > 0) {
            const unsigned bx = (unsigned)max(ax, 1), by = (unsigned)max(ay, 1), bz = (unsigned)max(az, 1);
            const unsigned ix = 2u * by * bz, iy = 2u * bx * bz, iz = 2u * bx * by;
            unsigned tx = ax ? by * bz : ~0u, ty = ay ? bx * bz : ~0u, tz = az ? bx * by : ~0u;
            const int sx = dx < 0 ? -1 : 1;
            const unsigned ry = dy < 0 ? 0u - wordsX : wordsX, rz = dz < 0 ? 0u - plane : plane;
            const unsigned rowS = ((unsigned)q.z * (unsigned)D.y + (unsigned)q.y) * wordsX;
            int cx = x;
            unsigned row = row0;
            for (;;) {
                const unsigned t = min(tx, min(ty, tz));
                if (tx == t) { cx += sx; tx += ix; }
                if (ty == t) { row += ry; ty += iy; }
                if (tz == t) { row += rz; tz += iz; }
                if (cx == q.x && row == rowS) break;                    // arrived: s itself is not counted
                if ((S[row + ((unsigned)cx >> 5)] >> (cx & 31)) & 1u) {
                    if (++k >= A.stop) break;                           // every T from here on is zero, and the view is not clear
                }
            }
        }
        if (in) {
            unsigned c = (unsigned)(((unsigned long long)(unsigned)q.w * (unsigned long long)(k < A.m ? T[k] : 0u)) >> 16);
            if (A.falloff == RTO_DOSE_FALLOFF_INVERSE_SQUARE) c /= (unsigned)max(1, ax * ax + ay * ay + az * az);
            sum += c;
        }
        const bool clear = in && k == 0;
        seen = seen || clear;
        const unsigned long long lanes = __ballot(clear);
#if !defined(RTO_DOSE_AB_NO_COVERAGE_ATOMIC)                                // A/B builds only (tools/build_variants.sh): what the atomics cost
        if (lanes && threadIdx.x % kWave == 0) atomicAdd(&covered[si], (unsigned long long)__popcll(lanes));
#else
        (void)lanes;
#endif
    }
    if (mine) {
        e[v] = (int)sum;
        if (seen) list[i] = v | kDoseSeenBit;
    }
}

// ---- summary over the list.  out[0]: the sum of e; out[1]: voxels with e == 0; out[2]: voxels that saw a source; out[3]: the
// largest (e << 32 | 2^32 - 1 - v), which is the peak and the smallest index that attains it (zero before the launch: below every
// key, whose low word is above 2^31).
__global__ __launch_bounds__(kBlock) void k_dose_summary(const int* __restrict__ e, const unsigned* __restrict__ list, unsigned count,
                                                        unsigned long long* __restrict__ out) {
    struct DoseSums { unsigned long long total, best; unsigned dark, seen; } s = { 0ull, 0ull, 0u, 0u };
    for (unsigned i = blockIdx.x * (unsigned)kBlock + threadIdx.x; i < count; i += gridDim.x * (unsigned)kBlock) {
        const unsigned entry = list[i], v = entry & ~kDoseSeenBit;
        const int q = e[v];
        const unsigned long long key = ((unsigned long long)(unsigned)q << 32) | (unsigned long long)(0xffffffffu - v);
        s.total += (unsigned long long)q;
        s.best = key > s.best ? key : s.best;
        s.dark += q == 0 ? 1u : 0u;
        s.seen += entry >> 31;
    }
    s = block_reduce<kBlock>(s, [](DoseSums a, const DoseSums& b) {
        a.total += b.total; a.dark += b.dark; a.seen += b.seen;
        a.best = b.best > a.best ? b.best : a.best;
        return a;
    });
    if (threadIdx.x == 0) {
        if (s.total) atomicAdd(&out[0], s.total);
        if (s.dark) atomicAdd(&out[1], (unsigned long long)s.dark);
        if (s.seen) atomicAdd(&out[2], (unsigned long long)s.seen);
        if (s.best) atomicMax(&out[3], s.best);
    }
}

}  // namespace rto

namespace {

// The coverage table of a call, the call's own until the field is published.
struct DoseCoverage {
    long long* d = nullptr;
    DoseCoverage() = default;
    DoseCoverage(const DoseCoverage&) = delete;
    DoseCoverage& operator=(const DoseCoverage&) = delete;
    ~DoseCoverage() { (void)hipFree(d); }
};

}  // namespace

extern "C" {

int rto_dose_field(rto_context* c, const int32_t* sources, int n, const uint32_t* transmit, int m, int falloff, int mode, int reach,
                   rto_dose_summary* summary) {
    using namespace rto;
    if (!c) return RTO_E_INVALID;
    const std::string w("rto_dose_field");
    if (!sources) return fail(c, RTO_E_INVALID, w + ": sources is NULL");
    if (n < 1 || n > RTO_DOSE_MAX_SOURCES) return fail(c, RTO_E_INVALID, w + ": n is not in 1 .. RTO_DOSE_MAX_SOURCES");
    int64_t W = 0;
    for (int i = 0; i < n; i++) {
        const int64_t wi = sources[4 * (size_t)i + 3];
        if (wi < 0) return fail(c, RTO_E_INVALID, w + ": a weight is negative");
        W += wi;
    }
    if (W > 0x7fffffffll) return fail(c, RTO_E_INVALID, w + ": the weights sum to more than 2^31 - 1");
    const uint32_t sight[1] = { 65536u };
    if (!transmit) { transmit = sight; m = 1; }
    if (m < 1 || m > RTO_DOSE_MAX_TABLE) return fail(c, RTO_E_INVALID, w + ": m is not in 1 .. RTO_DOSE_MAX_TABLE");
    for (int i = 0; i < m; i++)
        if (transmit[i] > 65536u) return fail(c, RTO_E_INVALID, w + ": a table entry is above 65536");
    if (falloff != RTO_DOSE_FALLOFF_NONE && falloff != RTO_DOSE_FALLOFF_INVERSE_SQUARE) return fail(c, RTO_E_INVALID, w + ": unknown falloff");
    if (mode != RTO_DOSE_ALL && mode != RTO_DOSE_SKIN) return fail(c, RTO_E_INVALID, w + ": unknown mode");
    if (reach < 1) return fail(c, RTO_E_INVALID, w + ": reach is below 1");
    const int rcGrid = resident_grid_check(c, "rto_dose_field", ": the field is 32-bit");
    if (rcGrid != RTO_OK) return rcGrid;
    for (int i = 0; i < n; i++)
        for (int a = 0; a < 3; a++)
            if (sources[4 * (size_t)i + a] < 0 || sources[4 * (size_t)i + a] >= c->voxDim[a])
                return fail(c, RTO_E_INVALID, w + ": source " + std::to_string(i) + " is outside the grid");

    // a pair may leave the march at the first k >= 1 from which every entry of the table is zero: its contribution is then zero
    // whatever follows, and k >= 1 already says that the view is not clear
    int stop = m;
    while (stop > 1 && transmit[stop - 1] == 0u) stop--;
    const DoseArgs A{ n, m, stop, falloff, std::min(reach, RTO_DOSE_MAX_REACH) };

    FieldDraft draft(c, kFieldDose);
    const int rcDraft = draft.begin();
    if (rcDraft != RTO_OK) return rcDraft;
    DoseCoverage cover;
    RTO_HIP(c, fallible_malloc(reinterpret_cast<void**>(&cover.d), (size_t)n * sizeof(long long)));
    hipStream_t s = c->stream;
    const unsigned nvox = (unsigned)grid_voxels(c);
    const int wordsX = (c->voxDim[0] + 31) / 32;
    const ExDims D{ c->voxDim[0], c->voxDim[1], c->voxDim[2], wordsX, (unsigned)((int64_t)wordsX * c->voxDim[1] * c->voxDim[2]) };
    float ms[3] = { -1.f, -1.f, -1.f };
    unsigned count = 0u;
    unsigned long long red[4] = { 0ull, 0ull, 0ull, 0ull };
    {
        StreamEvents<4> events;
        RTO_HIP(c, events.create());
        BuildScratch scratch(s);
        unsigned* d_bits = nullptr; unsigned* d_list = nullptr; unsigned* d_count = nullptr; int4* d_src = nullptr; unsigned* d_table = nullptr;
        unsigned long long* d_red = nullptr;
        RTO_HIP(c, scratch.alloc(&d_bits, (size_t)D.words));
        RTO_HIP(c, scratch.alloc(&d_list, (size_t)nvox));
        RTO_HIP(c, scratch.alloc(&d_count, 1));
        RTO_HIP(c, scratch.alloc(&d_src, (size_t)n));
        RTO_HIP(c, scratch.alloc(&d_table, (size_t)m));
        RTO_HIP(c, scratch.alloc(&d_red, 4));
        RTO_HIP(c, events.record(0, s));
        RTO_HIP(c, hipMemsetAsync(d_count, 0, sizeof(unsigned), s));
        RTO_HIP(c, hipMemsetAsync(d_red, 0, 4 * sizeof(unsigned long long), s));
        RTO_HIP(c, hipMemsetAsync(cover.d, 0, (size_t)n * sizeof(long long), s));
        RTO_HIP(c, hipMemcpyAsync(d_src, sources, (size_t)n * sizeof(int4), hipMemcpyHostToDevice, s));
        RTO_HIP(c, hipMemcpyAsync(d_table, transmit, (size_t)m * sizeof(unsigned), hipMemcpyHostToDevice, s));
        RTO_HIP(c, hipMemsetAsync(draft.d, 0xff, (size_t)nvox * sizeof(int), s));
        const dim3 b(kBlock), perWord((D.words + kBlock - 1) / kBlock);
        if (D.x % 32 == 0) hipLaunchKernelGGL(k_expo_bits<true>, perWord, b, 0, s, c->d_vox, D, d_bits);
        else hipLaunchKernelGGL(k_expo_bits<false>, perWord, b, 0, s, c->d_vox, D, d_bits);
        RTO_HIP(c, hipGetLastError());
        if (mode == RTO_DOSE_SKIN) hipLaunchKernelGGL(k_expo_select<true>, perWord, b, 0, s, d_bits, D, d_list, d_count);
        else hipLaunchKernelGGL(k_expo_select<false>, perWord, b, 0, s, d_bits, D, d_list, d_count);
        RTO_HIP(c, hipGetLastError());
        RTO_HIP(c, hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, s));
        RTO_HIP(c, events.record(1, s));
        RTO_HIP(c, hipStreamSynchronize(s));                               // the uploads from the caller's memory have landed too
        if (count > nvox) return fail(c, RTO_E_INTERNAL, w + ": the list holds more voxels than the grid");
        if (count) {
            hipLaunchKernelGGL(k_dose_march, dim3((count + kBlock - 1) / kBlock), b, 0, s, d_bits, D, d_list, count, d_src, d_table, A,
                               reinterpret_cast<unsigned long long*>(cover.d), draft.d);
            RTO_HIP(c, hipGetLastError());
        }
        RTO_HIP(c, events.record(2, s));
        if (summary && count) {
            const unsigned blocks = std::min<unsigned>((count + kBlock - 1) / kBlock, 4096u);
            hipLaunchKernelGGL(k_dose_summary, dim3(blocks), b, 0, s, draft.d, d_list, count, d_red);
            RTO_HIP(c, hipGetLastError());
        }
        RTO_HIP(c, events.record(3, s));
        RTO_HIP(c, hipMemcpyAsync(red, d_red, sizeof red, hipMemcpyDeviceToHost, s));
        RTO_HIP(c, hipStreamSynchronize(s));
        for (int i = 0; i < (summary ? 3 : 2); i++) RTO_HIP(c, events.elapsed(i, i + 1, &ms[i]));
    }
    if (summary) {
        summary->evaluated = (int64_t)count;
        summary->total = (int64_t)red[0];
        summary->dark = (int64_t)red[1];
        summary->seen = (int64_t)red[2];
        summary->peak = count ? (int64_t)(red[3] >> 32) : -1;
        summary->peak_voxel = count ? (int64_t)(0xffffffffu - (unsigned)(red[3] & 0xffffffffull)) : -1;
    }
    draft.publish();
    (void)hipFree(c->d_doseCov);
    c->d_doseCov = cover.d;
    cover.d = nullptr;
    c->doseN = n; c->doseW = W; c->doseM = m; c->doseFalloff = falloff; c->doseMode = mode; c->doseReach = A.reach;
    for (int i = 0; i < 3; i++) c->doseMs[i] = ms[i];
    return RTO_OK;
}

int rto_download_dose(rto_context* c, int32_t* out, int64_t capacity) { return download_field(c, "rto_download_dose", kFieldDose, out, capacity); }

int rto_dose_device(rto_context* c, int32_t** d_e) { return field_device(c, "rto_dose_device", kFieldDose, d_e); }

int rto_download_dose_coverage(rto_context* c, int64_t* out, int64_t capacity) {
    if (!c) return RTO_E_INVALID;
    const int rc = resident_field_check(c, "rto_download_dose_coverage", kFieldDose);
    if (rc != RTO_OK) return rc;
    return download_resident(c, "rto_download_dose_coverage", out, capacity, c->d_doseCov, (int64_t)c->doseN, sizeof(int64_t));
}

int rto_last_dose_ms(const rto_context* c, float ms[3]) { return copy_last_ms(c, &rto_context::doseMs, ms); }

}  // extern "C"
