// rto_exposure.inc -- exposure fields of the resident grid (include/rto_hip.h, rto_exposure_field): for every evaluated EMPTY voxel
// the sum of the weights of the directions along which the ray from the voxel's centre crosses no SOLID voxel of the grid within
// the reach, kept resident as one int32 per voxel (-1 for a voxel that is not evaluated).  Included at the end of rto_api.hip, after
// rto_skeleton.inc.
//
// Rule (DESIGN.md section 25).  In doubled integer coordinates the centre of p is 2 p + 1 and voxel q the open cube (2 q, 2 q + 2)^3;
// q != p is crossed when the open half line from the centre along d meets that cube.  For primitive d = (a, b, c) the planes of an
// axis are crossed at t = (2 m + 1) / (2 |a|), never at t = 1, where the ray is at the centre of p + d: the offsets q - p crossed in
// (0, 1], with equal t of several axes merged into one step that moves on all of them, are ONE PERIOD, the same for every p; period
// k is that list shifted by k d.  The max-norm of the offsets never decreases, and a ray that has left the grid never returns.
//
// (1) k_expo_bits makes the SOLID bit rows: one 32-bit word per 32 voxels of a grid row (word wx of row (y, z) holds x = 32 wx ..
// 32 wx + 31; bits beyond dimX are 0), section 23's layout.
// (2) e is filled with -1 (a memset: every byte 0xff), and k_expo_select, one thread per word, appends the linear indices of the
// evaluated voxels to a list, one atomic per wave; every entry owns its e[v], so the list's order changes no value.
// (3) The host makes one period per direction (expo_template), three signed 10-bit offsets packed into one int32, padded with zeros
// to four entries a row, and uploads them with a table of {first row, entries, primitive d, weight} per direction.
// (4) k_expo_march: one thread per listed voxel.  The loops over directions, periods and entries are wave-uniform, so the table and
// the template rows are read through wave-uniform addresses; a lane tests one bit per entry and leaves a direction when it is
// blocked, out of the grid or beyond the reach; the wave leaves when all its lanes have.  No atomics, no LDS; e[v] is written once.
// (5) k_expo_summary adds e over the list.

namespace rto {

struct ExDims { int x, y, z, wordsX; unsigned words; };
struct ExDir { int row, len, dx, dy, dz, w; };                         // row: the first int4 of the direction's period

constexpr int kExPad = 4;                                                // template entries per row

__host__ __device__ __forceinline__ int ex_pack(int ox, int oy, int oz) { return (ox & 0x3ff) | ((oy & 0x3ff) << 10) | ((oz & 0x3ff) << 20); }

// ---- bit rows.  One thread per word.  WIDE: dimX % 32 == 0, so a word's 32 bytes are whole and aligned.
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void k_expo_bits(const uint8_t* __restrict__ vox, ExDims D, unsigned* __restrict__ S) {
    const unsigned w = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    if (w >= D.words) return;
    const unsigned wx = w % (unsigned)D.wordsX, row = w / (unsigned)D.wordsX;
    const size_t base = (size_t)row * (size_t)D.x + (size_t)wx * 32u;
    unsigned bits = 0u;
    if (WIDE) {
        const uint4 a = *reinterpret_cast<const uint4*>(vox + base), b = *reinterpret_cast<const uint4*>(vox + base + 16);
        const unsigned q[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
#pragma unroll
        for (int j = 0; j < 32; j++) bits |= (((q[j >> 2] >> (8 * (j & 3))) & 0xffu) == 1u ? 1u : 0u) << j;
    } else {
        const int cnt = min(32, D.x - (int)wx * 32);
        for (int j = 0; j < cnt; j++) bits |= ((unsigned)vox[base + j] == 1u ? 1u : 0u) << j;
    }
    S[w] = bits;
}

// ---- selection.  One thread per word (e is -1 everywhere before the launch): the word's evaluated voxels as a mask -- EMPTY, and
// under SKIN with a SOLID face neighbour: the x neighbours by shifts of the row's own word and the end bits of the words beside it,
// the y and z neighbours the same word of the four rows around -- then the wave's counts are summed by a scan, one atomic a wave
// reserves its stretch of the list, and every lane writes its voxels in ascending order.  Every lane of a wave reaches the shuffles.
template <bool SKIN>
__global__ __launch_bounds__(kBlock) void k_expo_select(const unsigned* __restrict__ S, ExDims D, unsigned* __restrict__ list,
                                                       unsigned* __restrict__ count) {
    const unsigned w = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    unsigned cand = 0u, v0 = 0u;
    if (w < D.words) {
        const unsigned wordsX = (unsigned)D.wordsX, wx = w % wordsX, row = w / wordsX;
        const int left = D.x - (int)wx * 32;                            // voxels of the row from this word on
        const unsigned own = S[w];
        cand = ~own & (left >= 32 ? ~0u : (1u << left) - 1u);
        if (SKIN && cand) {
            const unsigned y = row % (unsigned)D.y, z = row / (unsigned)D.y, plane = wordsX * (unsigned)D.y;
            unsigned near = (own << 1) | (own >> 1);
            if (wx > 0u) near |= S[w - 1u] >> 31;
            if (wx + 1u < wordsX) near |= S[w + 1u] << 31;
            if (y > 0u) near |= S[w - wordsX];
            if (y + 1u < (unsigned)D.y) near |= S[w + wordsX];
            if (z > 0u) near |= S[w - plane];
            if (z + 1u < (unsigned)D.z) near |= S[w + plane];
            cand &= near;
        }
        v0 = row * (unsigned)D.x + wx * 32u;
    }
    unsigned at = wave_append((unsigned)__popc(cand), count);
    while (cand) {
        list[at++] = v0 + (unsigned)(__ffs(cand) - 1);
        cand &= cand - 1u;
    }
}

// ---- march.  One thread per listed voxel.  table[d] and the rows of tmpl are the same for all lanes of a wave.
__global__ __launch_bounds__(kBlock) void k_expo_march(const unsigned* __restrict__ S, ExDims D, const unsigned* __restrict__ list, unsigned count,
                                                      const ExDir* __restrict__ table, const int4* __restrict__ tmpl, int n, int reach,
                                                      int* __restrict__ e) {
    const unsigned i = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    const bool mine = i < count;
    const unsigned v = mine ? list[i] : 0u;
    const unsigned row = v / (unsigned)D.x;
    const int x = (int)(v % (unsigned)D.x), y = (int)(row % (unsigned)D.y), z = (int)(row / (unsigned)D.y);
    int sum = 0;
    for (int d = 0; d < n; d++) {
        const ExDir dir = table[d];
        const int rows = (dir.len + kExPad - 1) / kExPad;
        bool live = mine, blocked = false;
        int kx = 0, ky = 0, kz = 0;                                     // the period's shift, k d
        while (__any(live)) {
            for (int r = 0; r < rows; r++) {
                const int4 q = tmpl[dir.row + r];
                const int four[kExPad] = { q.x, q.y, q.z, q.w };
#pragma unroll
                for (int u = 0; u < kExPad; u++) {
                    if (r * kExPad + u < dir.len && live) {
                        // an offset is at most the grid's size and one period: no sum here leaves 32 bits
                        const int rx = kx + ((int)((unsigned)four[u] << 22) >> 22), ry = ky + ((int)((unsigned)four[u] << 12) >> 22),
                                  rz = kz + ((int)((unsigned)four[u] << 2) >> 22);
                        const int qx = x + rx, qy = y + ry, qz = z + rz;
                        if (max(max(abs(rx), abs(ry)), abs(rz)) > reach || (unsigned)qx >= (unsigned)D.x || (unsigned)qy >= (unsigned)D.y ||
                            (unsigned)qz >= (unsigned)D.z) {
                            live = false;
                        } else if ((S[((unsigned)qz * (unsigned)D.y + (unsigned)qy) * (unsigned)D.wordsX + ((unsigned)qx >> 5)] >> (qx & 31)) & 1u) {
                            blocked = true;
                            live = false;
                        }
                    }
                }
                if (!__any(live)) break;
            }
            kx += dir.dx; ky += dir.dy; kz += dir.dz;
        }
        if (!blocked) sum += dir.w;
    }
    if (mine) e[v] = sum;
}

// ---- summary over the list.  out[0]: the sum of e; out[1]: voxels with e == 0; out[2]: voxels with e == W (zero before the launch).
__global__ __launch_bounds__(kBlock) void k_expo_summary(const int* __restrict__ e, const unsigned* __restrict__ list, unsigned count, int W,
                                                        unsigned long long* __restrict__ out) {
    struct ExSums { unsigned long long total; unsigned dark, open; } s = { 0ull, 0u, 0u };
    for (unsigned i = blockIdx.x * (unsigned)kBlock + threadIdx.x; i < count; i += gridDim.x * (unsigned)kBlock) {
        const int q = e[list[i]];
        s.total += (unsigned long long)q;
        s.dark += q == 0 ? 1u : 0u;
        s.open += q == W ? 1u : 0u;
    }
    s = block_reduce<kBlock>(s, [](ExSums a, const ExSums& b) {
        a.total += b.total; a.dark += b.dark; a.open += b.open;
        return a;
    });
    if (threadIdx.x == 0) {
        if (s.total) atomicAdd(&out[0], s.total);
        if (s.dark) atomicAdd(&out[1], (unsigned long long)s.dark);
        if (s.open) atomicAdd(&out[2], (unsigned long long)s.open);
    }
}

}  // namespace rto

namespace {

// One period of direction d as packed entries appended to `packed` in rows of kExPad (the last row filled with zeros); prim = d
// over the gcd of its components.  The planes of axis a are crossed at t = (2 m + 1) / (2 |a|): the next crossing of every axis is
// kept as the fraction (2 m + 1) / |a|, the smallest found by cross-multiplication (products below 2^18), and every axis that ties
// moves in the same step.  The entries made.
int expo_template(const int32_t d[3], std::vector<int>& packed, int prim[3]) {
    auto gcd = [](int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; };
    const int g = gcd(gcd(std::abs(d[0]), std::abs(d[1])), std::abs(d[2]));
    int len[3], sign[3], m[3] = { 0, 0, 0 }, at[3] = { 0, 0, 0 }, entries = 0;
    for (int a = 0; a < 3; a++) {
        prim[a] = d[a] / g;
        len[a] = std::abs(prim[a]);
        sign[a] = prim[a] < 0 ? -1 : 1;
    }
    while (m[0] < len[0] || m[1] < len[1] || m[2] < len[2]) {
        int first = -1;
        for (int a = 0; a < 3; a++)
            if (m[a] < len[a] && (first < 0 || (2 * m[a] + 1) * len[first] < (2 * m[first] + 1) * len[a])) first = a;
        const int num = 2 * m[first] + 1, den = len[first];
        for (int a = 0; a < 3; a++)
            if (m[a] < len[a] && (2 * m[a] + 1) * den == num * len[a]) { m[a]++; at[a] += sign[a]; }
        packed.push_back(rto::ex_pack(at[0], at[1], at[2]));
        entries++;
    }
    while (packed.size() % rto::kExPad) packed.push_back(0);
    return entries;
}

}  // namespace

extern "C" {

int rto_exposure_field(rto_context* c, const int32_t* dirs, const int32_t* weights, int n, int mode, int reach, rto_expo_summary* summary) {
    using namespace rto;
    if (!c) return RTO_E_INVALID;
    const std::string w("rto_exposure_field");
    if (!dirs) return fail(c, RTO_E_INVALID, w + ": dirs is NULL");
    if (n < 1 || n > RTO_EXPO_MAX_DIRS) return fail(c, RTO_E_INVALID, w + ": n is not in 1 .. RTO_EXPO_MAX_DIRS");
    for (int i = 0; i < n; i++) {
        const int32_t* d = dirs + 3 * (size_t)i;
        if (!d[0] && !d[1] && !d[2]) return fail(c, RTO_E_INVALID, w + ": a direction is zero");
        for (int a = 0; a < 3; a++)
            if (d[a] < -RTO_EXPO_MAX_COMP || d[a] > RTO_EXPO_MAX_COMP) return fail(c, RTO_E_INVALID, w + ": a component is beyond RTO_EXPO_MAX_COMP");
    }
    int64_t W = 0;
    for (int i = 0; i < n; i++) {
        const int64_t wi = weights ? weights[i] : 1;
        if (wi < 0) return fail(c, RTO_E_INVALID, w + ": a weight is negative");
        W += wi;
    }
    if (W > 0x7fffffffll) return fail(c, RTO_E_INVALID, w + ": the weights sum to more than 2^31 - 1");
    if (mode != RTO_EXPO_ALL && mode != RTO_EXPO_SKIN) return fail(c, RTO_E_INVALID, w + ": unknown mode");
    if (reach < 1) return fail(c, RTO_E_INVALID, w + ": reach is below 1");
    const int rcGrid = resident_grid_check(c, "rto_exposure_field", ": the field is 32-bit");
    if (rcGrid != RTO_OK) return rcGrid;

    std::vector<int> packed;
    std::vector<ExDir> table((size_t)n);
    for (int i = 0; i < n; i++) {
        int prim[3];
        const int row = (int)(packed.size() / kExPad);
        const int len = expo_template(dirs + 3 * (size_t)i, packed, prim);
        table[(size_t)i] = ExDir{ row, len, prim[0], prim[1], prim[2], weights ? weights[i] : 1 };
    }

    FieldDraft draft(c, kFieldExposure);
    const int rcDraft = draft.begin();
    if (rcDraft != RTO_OK) return rcDraft;
    hipStream_t s = c->stream;
    const unsigned nvox = (unsigned)grid_voxels(c);
    const int wordsX = (c->voxDim[0] + 31) / 32;
    const ExDims D{ c->voxDim[0], c->voxDim[1], c->voxDim[2], wordsX, (unsigned)((int64_t)wordsX * c->voxDim[1] * c->voxDim[2]) };
    float ms[3] = { -1.f, -1.f, -1.f };
    unsigned count = 0u;
    unsigned long long red[3] = { 0ull, 0ull, 0ull };
    {
        StreamEvents<4> events;
        RTO_HIP(c, events.create());
        BuildScratch scratch(s);
        unsigned* d_bits = nullptr; unsigned* d_list = nullptr; unsigned* d_count = nullptr; ExDir* d_table = nullptr; int4* d_tmpl = nullptr;
        unsigned long long* d_red = nullptr;
        RTO_HIP(c, scratch.alloc(&d_bits, (size_t)D.words));
        RTO_HIP(c, scratch.alloc(&d_list, (size_t)nvox));
        RTO_HIP(c, scratch.alloc(&d_count, 1));
        RTO_HIP(c, scratch.alloc(&d_table, (size_t)n));
        RTO_HIP(c, scratch.alloc(&d_tmpl, packed.size() / kExPad));
        RTO_HIP(c, scratch.alloc(&d_red, 3));
        RTO_HIP(c, events.record(0, s));
        RTO_HIP(c, hipMemsetAsync(d_count, 0, sizeof(unsigned), s));
        RTO_HIP(c, hipMemsetAsync(d_red, 0, 3 * sizeof(unsigned long long), s));
        RTO_HIP(c, hipMemcpyAsync(d_table, table.data(), table.size() * sizeof(ExDir), hipMemcpyHostToDevice, s));
        RTO_HIP(c, hipMemcpyAsync(d_tmpl, packed.data(), packed.size() * sizeof(int), hipMemcpyHostToDevice, s));
        RTO_HIP(c, hipMemsetAsync(draft.d, 0xff, (size_t)nvox * sizeof(int), s));
        const dim3 b(kBlock), perWord((D.words + kBlock - 1) / kBlock);
        if (D.x % 32 == 0) hipLaunchKernelGGL(k_expo_bits<true>, perWord, b, 0, s, c->d_vox, D, d_bits);
        else hipLaunchKernelGGL(k_expo_bits<false>, perWord, b, 0, s, c->d_vox, D, d_bits);
        RTO_HIP(c, hipGetLastError());
        if (mode == RTO_EXPO_SKIN) hipLaunchKernelGGL(k_expo_select<true>, perWord, b, 0, s, d_bits, D, d_list, d_count);
        else hipLaunchKernelGGL(k_expo_select<false>, perWord, b, 0, s, d_bits, D, d_list, d_count);
        RTO_HIP(c, hipGetLastError());
        RTO_HIP(c, hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, s));
        RTO_HIP(c, events.record(1, s));
        RTO_HIP(c, hipStreamSynchronize(s));
        if (count > nvox) return fail(c, RTO_E_INTERNAL, w + ": the list holds more voxels than the grid");
        if (count) {
            hipLaunchKernelGGL(k_expo_march, dim3((count + kBlock - 1) / kBlock), b, 0, s, d_bits, D, d_list, count, d_table, d_tmpl, n, reach, draft.d);
            RTO_HIP(c, hipGetLastError());
        }
        RTO_HIP(c, events.record(2, s));
        if (summary && count) {
            const unsigned blocks = std::min<unsigned>((count + kBlock - 1) / kBlock, 4096u);
            hipLaunchKernelGGL(k_expo_summary, dim3(blocks), b, 0, s, draft.d, d_list, count, (int)W, d_red);
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
        summary->open = (int64_t)red[2];
    }
    draft.publish();
    c->expoN = n; c->expoW = W; c->expoMode = mode; c->expoReach = reach;
    for (int i = 0; i < 3; i++) c->expoMs[i] = ms[i];
    return RTO_OK;
}

int rto_download_exposure(rto_context* c, int32_t* out, int64_t capacity) { return download_field(c, "rto_download_exposure", kFieldExposure, out, capacity); }

int rto_exposure_device(rto_context* c, int32_t** d_e) { return field_device(c, "rto_exposure_device", kFieldExposure, d_e); }

int rto_last_exposure_ms(const rto_context* c, float ms[3]) { return copy_last_ms(c, &rto_context::expoMs, ms); }

}  // extern "C"
