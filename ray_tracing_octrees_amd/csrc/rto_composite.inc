// rto_composite.inc -- field compositing (include/rto_hip.h, rto_composite_field_*): per pixel the valued voxels of an int32 volume
// that the pixel ray crosses, coloured through a LUT and composited front to back in integers, the march stopped by saturation or
// by the grid's solids.  Included at the end of rto_api.hip, after rto_voxel_walk.inc (section 28's walk: WalkBox, VoxelWalk,
// k_project_bricks, walk_box, walk_bricks_launch), rto_field_view.inc (kFieldSlots, and the host pieces of every field frame:
// field_frame_check, work_buffer, stage_events, HostStage, misaligned) and rto_lit.inc (tile_pixel, lit_mix32, frame_bound_check).
//
// Rule (DESIGN.md section 29).  The visited voxels are section 28's; a valued voxel's LUT index is section 27's; the entry's alpha
// byte a gives a' = a + (a >> 7); T starts at 65536 and every contributing voxel takes c = (T a') >> 8 of it into R, G and B.
//
// Kernels (one stream, no host step):
//   k_project_bricks     rto_voxel_walk.inc: the largest and smallest valued value of every brick.
//   k_composite_solid    one byte per brick: does it hold a FILLED voxel?  One wave per (brick row, run along x): lane l reads
//                        BYTES bytes of row y = l >> 3 at chunk l & 7, for the brick row's 8 z at once (eight loads in flight,
//                        the byte grid once).  BYTES is the largest power of two up to 16 that divides dimX, so that every row
//                        starts aligned to it and no load straddles a row or a brick pair.
//   k_composite_march    one lane per pixel, 8x8 tiles per wave.  Per workgroup, once: the 256 LUT entries as (a', rgb), the prefix
//                        count of entries with a' != 0, and under LINEAR and SQRT the 256 thresholds of the index.  Then the
//                        walk's entry by rank and one trip per voxel or per skipped brick.
//   k_composite_fold     one wave: the summary block's records into the caller's rto_composite_summary.

namespace rto {

// One record of the summary block while a frame is in flight (zeroed in front of it): visited | contributing << 32 and saturated |
// occluded << 32, all below 2^32 (frame_bound_check).
struct alignas(128) CompositeSumRaw {
    unsigned long long seen;
    unsigned long long ended;
};

struct OpOr { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a | b; } };

struct CompositeArgs {
    const unsigned char* vox;     // the resident grid's bytes; null: occlude == 0
    int scale;
    int rangeLo, rangeHi;
    unsigned stop;
    const unsigned char* solid;   // 1: the brick holds a FILLED voxel; read only with vox
    // Keep `box` exactly here: where it stands decides which arguments the build parks in VGPR lanes, and no budget test sees that
    // (LAB_NOTES, "One voxel walk and one host path", shape (b)).  First in the struct, tools/composite_bench.py's twelve air/opaque
    // figures ran 3.3 to 4.9 % slower; last, thirteen long-march figures 1.1 to 1.9 %.  Run that tool after any change to this struct.
    WalkBox box;
    const unsigned* lut;
    const float4* under;          // may be null; may be rgba
    float4* rgba;
    unsigned* trans;              // the four below may be null
    int* first;
    int* stops;
    int* counts;
    float bg[4], miss[4];
    CompositeSumRaw* sum;
};

// Does one of the four bytes of x equal 1?  x ^ 0x01010101 has a zero byte exactly there, and (y - 0x01010101) & ~y & 0x80808080 is
// non-zero exactly when y has a zero byte.
__device__ __forceinline__ bool composite_has_filled(unsigned x) {
    const unsigned y = x ^ 0x01010101u;
    return ((y - 0x01010101u) & ~y & 0x80808080u) != 0u;
}

template <int BYTES> struct CompositeLoad;
template <> struct CompositeLoad<16> { static __device__ __forceinline__ uint4 at(const unsigned char* p) { return *reinterpret_cast<const uint4*>(p); } };
template <> struct CompositeLoad<8> { static __device__ __forceinline__ uint4 at(const unsigned char* p) { const uint2 v = *reinterpret_cast<const uint2*>(p); return make_uint4(v.x, v.y, 0u, 0u); } };
template <> struct CompositeLoad<4> { static __device__ __forceinline__ uint4 at(const unsigned char* p) { return make_uint4(*reinterpret_cast<const unsigned*>(p), 0u, 0u, 0u); } };
template <> struct CompositeLoad<2> { static __device__ __forceinline__ uint4 at(const unsigned char* p) { return make_uint4(*reinterpret_cast<const unsigned short*>(p), 0u, 0u, 0u); } };
template <> struct CompositeLoad<1> { static __device__ __forceinline__ uint4 at(const unsigned char* p) { return make_uint4(*p, 0u, 0u, 0u); } };

// A wave's run is 8 chunks of BYTES voxels along x: BYTES bricks.  dimX % BYTES == 0 and the grid's base is aligned to BYTES
// (composite_field picks BYTES so), hence every load is aligned and x + BYTES <= dimX for every x < dimX.
template <int BYTES>
__global__ __launch_bounds__(kBlock) void k_composite_solid(const unsigned char* __restrict__ vox, int dimX, int dimY, int dimZ, int nbx, int nby,
                                                            int runsX, unsigned waves, unsigned char* __restrict__ solid) {
    const unsigned w = blockIdx.x * (unsigned)(kBlock / kWave) + (threadIdx.x >> 6);      // wave-uniform
    if (w >= waves) return;
    const int lane = threadIdx.x & 63;
    const int rx = (int)(w % (unsigned)runsX);
    const unsigned row = w / (unsigned)runsX;
    const int by = (int)(row % (unsigned)nby), bz = (int)(row / (unsigned)nby);
    const int xc = lane & 7;
    const int x = (rx * 8 + xc) * BYTES, y = by * 8 + (lane >> 3);
    const int z1 = min(bz * 8 + 8, dimZ);
    unsigned m = 0u;                                     // bit b: brick b of the run holds a FILLED voxel
    if (x < dimX && y < dimY) {
        const unsigned char* p = vox + ((size_t)(bz * 8) * (size_t)dimY + (size_t)y) * (size_t)dimX + (size_t)x;
        const size_t plane = (size_t)dimY * (size_t)dimX;
        uint4 v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = bz * 8 + k < z1 ? CompositeLoad<BYTES>::at(p + (size_t)k * plane) : make_uint4(0u, 0u, 0u, 0u);   // eight loads in flight
        bool lo = false, hi = false;                     // the chunk's first 8 bytes, and (BYTES == 16) its second
#pragma unroll
        for (int k = 0; k < 8; k++) {
            lo = lo || composite_has_filled(v[k].x) || composite_has_filled(v[k].y);
            hi = hi || composite_has_filled(v[k].z) || composite_has_filled(v[k].w);
        }
        if (BYTES == 16) m = (lo ? 1u : 0u) << (2 * xc) | (hi ? 2u : 0u) << (2 * xc);
        else m = (lo ? 1u : 0u) << ((xc * BYTES) >> 3);
    }
    m = wave_reduce(m, OpOr());
    const int bx = rx * BYTES + lane;
    if (lane < BYTES && bx < nbx) solid[((size_t)bz * (size_t)nby + (size_t)by) * (size_t)nbx + (size_t)bx] = (unsigned char)((m >> lane) & 1u);
}

// The field views' index of value v from the thresholds: the largest k in 0 .. 255 with thr[k] <= w, w = clamp(v) - lo.
__device__ __forceinline__ int composite_index(const unsigned* thr, int scale, int v, int lo, int hi) {
    if (scale == RTO_SCALE_CATEGORY) return (int)(lit_mix32((unsigned)v) & 255u);
    const int cl = v < lo ? lo : (v > hi ? hi : v);
    const unsigned w = (unsigned)cl - (unsigned)lo;      // the true difference, 0 .. 2^32 - 1
    int k = 0;
#pragma unroll
    for (int bit = 128; bit > 0; bit >>= 1) {
        const int t = k | bit;
        if (thr[t] <= w) k = t;
    }
    return k;
}

__global__ __launch_bounds__(kBlock) void k_composite_march(RenderParams P, CompositeArgs A) {
    __shared__ uint2 ent[256];            // (a', r | g << 8 | b << 16)
    __shared__ unsigned thr[256];
    __shared__ int pre[257];              // pre[k]: the entries below k with a' != 0
    static_assert(kBlock == 256, "one thread per LUT entry");
    {
        const unsigned e = A.lut[threadIdx.x];
        const unsigned a = e >> 24, ap = a + (a >> 7);
        ent[threadIdx.x] = make_uint2(ap, e & 0xffffffu);
        int total;
        pre[threadIdx.x] = block_rank<kBlock>(ap != 0u, &total);
        if (threadIdx.x == 255) pre[256] = total;
        // thr[k]: the smallest w whose index is at least k.  Section 27's index is the largest k with k m(k) s <= w D (m(k) = 1, D =
        // 255 under LINEAR; m(k) = k, D = 65025 under SQRT); k m(k) s is monotone in k, so that index is the number of k in 1 .. 255
        // with ceil(k m(k) s / D) <= w, and the thresholds are sorted.  s <= 2^32 - 1 and k m(k) <= D: a threshold fits 32 bits.
        const long long s = (long long)A.rangeHi - (long long)A.rangeLo, k = (long long)threadIdx.x;
        const long long num = (A.scale == RTO_SCALE_SQRT ? k * k : k) * s, den = A.scale == RTO_SCALE_SQRT ? 65025ll : 255ll;
        thr[threadIdx.x] = A.scale == RTO_SCALE_CATEGORY ? 0u : (unsigned)((num + den - 1ll) / den);
    }
    __syncthreads();

    const Geo G = geo_of(P);
    const TilePixel t = tile_pixel(P);
    const bool inFrame = t.in;
    const int lane = threadIdx.x & 63;

    VoxelWalk W;
    const bool visited = W.enter(G, t.r, inFrame, A.box);
    bool alive = visited;

    unsigned T = 65536u, R = 0u, Gc = 0u, B = 0u;
    int count = 0, firstVox = -1, stopVox = -1;
    bool saturated = false, occluded = false;
    int lastBrick = -1;
    bool skip = false;
    while (alive) {
        const int brick = W.brick();
        if (brick != lastBrick) {
            lastBrick = brick;
            skip = false;
            if (A.box.useTable) {
                const uint2 k = A.box.bricks[brick];
                skip = k.x == 0u;                                      // no valued voxel
                if (!skip && A.scale != RTO_SCALE_CATEGORY) {
                    // the index is monotone in the value: every valued voxel of the brick lies between these two entries
                    const int kHi = composite_index(thr, A.scale, (int)(k.x ^ 0x80000000u), A.rangeLo, A.rangeHi);
                    const int kLo = composite_index(thr, A.scale, (int)(~k.y ^ 0x80000000u), A.rangeLo, A.rangeHi);
                    skip = pre[kHi + 1] == pre[kLo];
                }
                if (skip && A.vox) skip = A.solid[brick] == 0;
            }
        }
        if (skip) {
            W.leave_brick(G.vs);
        } else {
            const int idx = W.voxel();
            const int v = A.box.volume[idx];
            if (A.vox && A.vox[idx] == 1) { occluded = true; stopVox = idx; break; }
            if (v >= A.box.validLo && v <= A.box.validHi) {
                const uint2 e = ent[composite_index(thr, A.scale, v, A.rangeLo, A.rangeHi)];
                if (e.x != 0u) {
                    const unsigned c = (T * e.x) >> 8;                  // T a' <= 2^24
                    R += c * (e.y & 255u); Gc += c * ((e.y >> 8) & 255u); B += c * (e.y >> 16);
                    T -= c;
                    if (count == 0) firstVox = idx;
                    count++;
                    if (T <= A.stop) { saturated = true; stopVox = idx; break; }
                }
            }
            W.step(G.vs);
        }
        alive = W.advance();
    }

    if (inFrame) {
        const unsigned pix = (unsigned)t.py * (unsigned)P.W + (unsigned)t.px;   // < 2^32 (frame_bound_check)
        float4 out;
        if (!A.under && !visited) {
            out = make_float4(A.miss[0], A.miss[1], A.miss[2], A.miss[3]);
        } else {
            const float4 bg = A.under ? A.under[pix] : make_float4(A.bg[0], A.bg[1], A.bg[2], A.bg[3]);    // read before the write below
            const float tf = (float)T / 65536.0f;
            out.x = (float)R / 16711680.0f + tf * bg.x;
            out.y = (float)Gc / 16711680.0f + tf * bg.y;
            out.z = (float)B / 16711680.0f + tf * bg.z;
            out.w = (float)(65536u - T) / 65536.0f + tf * bg.w;
        }
        A.rgba[pix] = out;
        if (A.trans) A.trans[pix] = T;
        if (A.first) A.first[pix] = firstVox;
        if (A.stops) A.stops[pix] = stopVox;
        if (A.counts) A.counts[pix] = count;
    }
    // the frame's summary: per wave two adds into the record its workgroup picks
    const unsigned nVis = wave_sum(visited ? 1u : 0u), nCon = wave_sum(count > 0 ? 1u : 0u);
    const unsigned nSat = wave_sum(saturated ? 1u : 0u), nOcc = wave_sum(occluded ? 1u : 0u);
    if (lane == 0 && nVis) {
        CompositeSumRaw* slot = A.sum + blockIdx.x % kFieldSlots;
        atomicAdd(&slot->seen, (unsigned long long)nVis | ((unsigned long long)nCon << 32));
        if (nSat | nOcc) atomicAdd(&slot->ended, (unsigned long long)nSat | ((unsigned long long)nOcc << 32));
    }
}

__global__ __launch_bounds__(kWave) void k_composite_fold(const CompositeSumRaw* __restrict__ sum, rto_composite_summary* __restrict__ out) {
    static_assert(kFieldSlots == kWave, "one lane per record");
    const unsigned long long seen = wave_sum(sum[threadIdx.x].seen), ended = wave_sum(sum[threadIdx.x].ended);
    if (threadIdx.x == 0) {
        rto_composite_summary o;
        o.visited = (int64_t)(seen & 0xffffffffull); o.contributing = (int64_t)(seen >> 32);
        o.saturated = (int64_t)(ended & 0xffffffffull); o.occluded = (int64_t)(ended >> 32);
        *out = o;
    }
}

}  // namespace rto

// ---------------------------------------------------------------- host side
static_assert(sizeof(rto_field_composite) == 112 && sizeof(rto_composite_summary) == 32, "the ABI's sizes");

// Every check of a composite, in the order the ABI promises; *volume: the int32 volume the frame composites.
static int composite_check(rto_context* c, const char* fn, const rto_frame* f, const rto_field_composite* v, const void* lut,
                           const int32_t* d_volume, const void* rgba, const int** volume) {
    const std::string name(fn);
    return field_frame_check(c, name, "composite", f, v, lut, d_volume, rgba, volume,
        [] { return RTO_OK; },
        [&] {
            if (v->scale != RTO_SCALE_CATEGORY && v->range_lo >= v->range_hi)
                return fail(c, RTO_E_INVALID, name + ": a composite has no auto range: LINEAR and SQRT need range_lo < range_hi");
            if (v->stop_q16 < 0 || v->stop_q16 > 65535) return fail(c, RTO_E_INVALID, name + ": stop_q16 must be 0 .. 65535");
            if (v->occlude != 0 && v->occlude != 1) return fail(c, RTO_E_INVALID, name + ": occlude must be 0 or 1");
            return RTO_OK;
        },
        [&] { return check_grid_index(c, name, "d_first"); });
}

// The solid table, the summary block and the timing events, kept on the context under the work buffers' rule (the brick table is
// walk_box's).
static int composite_reserve(rto_context* c, const char* fn, size_t bricks, hipStream_t s) {
    const char* why = ": a larger grid allocates the solid table; composite one frame of it before hipStreamBeginCapture";
    size_t sumCap = c->d_cpSum ? sizeof(CompositeSumRaw[kFieldSlots]) : 0;          // the summary block: of one size, made once
    int rc = work_buffer(c, c->d_cpSum, sumCap, sizeof(CompositeSumRaw[kFieldSlots]), s, fn, why);
    if (rc == RTO_OK) rc = stage_events(c, c->cpEv, s, fn, why);
    if (rc == RTO_OK) rc = work_buffer(c, c->d_cpSolid, c->cpSolidCap, bricks, s, fn, why);
    return rc;
}

template <int BYTES>
static void composite_solid_launch(rto_context* c, int nbx, int nby, int nbz, hipStream_t s) {
    const int runsX = (c->voxDim[0] + 8 * BYTES - 1) / (8 * BYTES);
    const int64_t waves = (int64_t)runsX * nby * nbz;
    const dim3 grid((unsigned)((waves + kBlock / kWave - 1) / (kBlock / kWave)));
    hipLaunchKernelGGL(k_composite_solid<BYTES>, grid, dim3(kBlock), 0, s, c->d_vox, c->voxDim[0], c->voxDim[1], c->voxDim[2], nbx, nby, runsX,
                       (unsigned)waves, c->d_cpSolid);
}

static int composite_field(rto_context* c, const char* fn, const rto_frame* f, const rto_field_composite* v, const unsigned* d_lut, const int* volume,
                           const float4* d_under, float4* d_rgba, uint32_t* d_trans, int32_t* d_first, int32_t* d_stops, int32_t* d_counts,
                           rto_composite_summary* d_summary, hipStream_t s) {
    RenderParams P;
    int rc = fill_params(c, f, nullptr, P, s);
    if (rc != RTO_OK) return rc;
    CompositeArgs A;
    if ((rc = walk_box(c, fn, v, volume, s, A.box)) != RTO_OK) return rc;
    const int nbx = A.box.nbx, nby = A.box.nby, nbz = walk_nbz(A.box);
    if ((rc = composite_reserve(c, fn, (size_t)nbx * (size_t)nby * (size_t)nbz, s)) != RTO_OK) return rc;
    A.vox = v->occlude ? c->d_vox : nullptr;
    A.scale = v->scale;
    A.rangeLo = v->range_lo; A.rangeHi = v->range_hi;
    A.stop = (unsigned)v->stop_q16;
    A.solid = c->d_cpSolid;
    A.lut = d_lut;
    A.under = d_under; A.rgba = d_rgba;
    A.trans = d_trans; A.first = d_first; A.stops = d_stops; A.counts = d_counts;
    std::memcpy(A.bg, v->background_rgba, sizeof A.bg);
    std::memcpy(A.miss, v->miss_rgba, sizeof A.miss);
    A.sum = reinterpret_cast<CompositeSumRaw*>(c->d_cpSum);

    const bool timed = !(stream_is_capturing(s) || c->eventsOff);
    RTO_HIP(c, hipMemsetAsync(c->d_cpSum, 0, kFieldSlots * sizeof(CompositeSumRaw), s));
    RTO_HIP(c, c->cpEv.mark(0, s, timed));
    if (A.box.useTable) {
        RTO_HIP(c, walk_bricks_launch(c, A.box, s));
        if (A.vox) {
            // the widest load that every row of the grid starts aligned to
            const uintptr_t align = (uintptr_t)A.box.dim[0] | reinterpret_cast<uintptr_t>(c->d_vox);
            if (align % 16 == 0) composite_solid_launch<16>(c, nbx, nby, nbz, s);
            else if (align % 8 == 0) composite_solid_launch<8>(c, nbx, nby, nbz, s);
            else if (align % 4 == 0) composite_solid_launch<4>(c, nbx, nby, nbz, s);
            else if (align % 2 == 0) composite_solid_launch<2>(c, nbx, nby, nbz, s);
            else composite_solid_launch<1>(c, nbx, nby, nbz, s);
            RTO_HIP(c, hipGetLastError());
        }
    }
    RTO_HIP(c, c->cpEv.mark(1, s, timed));
    const int64_t tiles = (int64_t)P.tilesX * P.tilesY;
    const dim3 grid((unsigned)((tiles + kBlock / kWave - 1) / (kBlock / kWave)));
    hipLaunchKernelGGL(k_composite_march, grid, dim3(kBlock), 0, s, P, A);
    RTO_HIP(c, hipGetLastError());
    RTO_HIP(c, c->cpEv.mark(2, s, timed));
    if (d_summary) {
        hipLaunchKernelGGL(k_composite_fold, dim3(1), dim3(kWave), 0, s, A.sum, d_summary);
        RTO_HIP(c, hipGetLastError());
    }
    RTO_HIP(c, c->cpEv.mark(3, s, timed));
    return RTO_OK;
}

extern "C" {

int rto_composite_field_device(rto_context* c, const rto_frame* frame, const rto_field_composite* comp, const uint32_t* d_lut,
                               const int32_t* d_volume, const void* d_under, void* d_rgba, uint32_t* d_transmittance, int32_t* d_first,
                               int32_t* d_stops, int32_t* d_counts, rto_composite_summary* d_summary, void* hip_stream) {
    if (!c) return RTO_E_INVALID;
    const char* fn = "rto_composite_field_device";
    if (frame && comp && d_lut && d_rgba &&
        (misaligned(d_rgba, 15) || misaligned(d_under, 15) || misaligned(d_lut, 3) || misaligned(d_volume, 3) || misaligned(d_transmittance, 3) ||
         misaligned(d_first, 3) || misaligned(d_stops, 3) || misaligned(d_counts, 3) || misaligned(d_summary, 7)))
        return fail(c, RTO_E_INVALID, std::string(fn) + ": d_under and d_rgba must be 16-byte, d_summary 8-byte, d_lut, d_volume, d_transmittance, "
                                      "d_first, d_stops and d_counts 4-byte aligned");
    const int* volume = nullptr;
    const int rc = composite_check(c, fn, frame, comp, d_lut, d_volume, d_rgba, &volume);
    if (rc != RTO_OK) return rc;
    RTO_HIP(c, hipSetDevice(c->device));
    return composite_field(c, fn, frame, comp, d_lut, volume, reinterpret_cast<const float4*>(d_under), reinterpret_cast<float4*>(d_rgba),
                           d_transmittance, d_first, d_stops, d_counts, d_summary, (hipStream_t)hip_stream);
}

int rto_composite_field_host(rto_context* c, const rto_frame* frame, const rto_field_composite* comp, const uint32_t* lut,
                             const int32_t* host_volume, const float* host_under, float* host_rgba, uint32_t* host_transmittance,
                             int32_t* host_first, int32_t* host_stops, int32_t* host_counts, rto_composite_summary* host_summary) {
    if (!c) return RTO_E_INVALID;
    const char* fn = "rto_composite_field_host";
    const int* volume = nullptr;
    int rc = composite_check(c, fn, frame, comp, lut, host_volume, host_rgba, &volume);
    if (rc != RTO_OK) return rc;
    RTO_HIP(c, hipSetDevice(c->device));
    HostStage H(c, frame, lut, host_rgba);
    uint32_t* d_trans = H.optional(host_transmittance, H.pixels);
    int32_t* d_first = H.optional(host_first, H.pixels);
    int32_t* d_stops = H.optional(host_stops, H.pixels);
    int32_t* d_counts = H.optional(host_counts, H.pixels);
    rto_composite_summary* d_summary = H.optional(host_summary, 1);
    float4* d_under = nullptr;
    if (host_under) {                                                // under the frame itself: composited in place on the device too
        d_under = host_under == host_rgba ? H.d_rgba : H.device<float4>(H.pixels);
        H.copy_in(d_under, reinterpret_cast<const float4*>(host_under), H.pixels);
    }
    volume = H.volume(host_volume, volume);
    if ((rc = H.status()) != RTO_OK) return rc;
    if ((rc = composite_field(c, fn, frame, comp, H.d_lut, volume, d_under, H.d_rgba, d_trans, d_first, d_stops, d_counts, d_summary, c->stream)) != RTO_OK)
        return rc;
    return H.finish();
}

int rto_last_composite_ms(const rto_context* c, float ms[3]) { return c && ms ? c->cpEv.read(ms) : RTO_E_INVALID; }

}  // extern "C"
