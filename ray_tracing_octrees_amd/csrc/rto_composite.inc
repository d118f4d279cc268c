// rto_composite.inc -- field compositing (include/rto_hip.h, rto_composite_field_*): per pixel the valued voxels of an int32 volume
// that the pixel ray crosses, coloured through a LUT and composited front to back in integers, the march stopped by saturation or
// by the grid's solids.  Included at the end of rto_api.hip, after rto_project.inc (the project_* walk helpers, k_project_bricks,
// project_reserve, kProjectStill), rto_field_view.inc (field_view_volume, kFieldSlots) and rto_lit.inc (tile_pixel, lit_mix32,
// frame_bound_check).
//
// Rule (DESIGN.md section 29).  The visited voxels are section 28's; a valued voxel's LUT index is section 27's; the entry's alpha
// byte a gives a' = a + (a >> 7); T starts at 65536 and every contributing voxel takes c = (T a') >> 8 of it into R, G and B.
//
// Kernels (one stream, no host step):
//   k_project_bricks     unchanged: the largest and smallest valued value of every brick.
//   k_composite_solid    one byte per brick: does it hold a FILLED voxel?  One wave per (brick row, run along x): lane l reads
//                        BYTES bytes of row y = l >> 3 at chunk l & 7, for the brick row's 8 z at once (eight loads in flight,
//                        the byte grid once).  BYTES is the largest power of two up to 16 that divides dimX, so that every row
//                        starts aligned to it and no load straddles a row or a brick pair.
//   k_composite_march    one lane per pixel, 8x8 tiles per wave.  Per workgroup, once: the 256 LUT entries as (a', rgb), the prefix
//                        count of entries with a' != 0, and under LINEAR and SQRT the 256 thresholds of the index.  Then section
//                        28's entry by rank and one trip per voxel or per skipped brick.
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
    const int* volume;            // dimZ x dimY x dimX, x fastest
    const unsigned char* vox;     // the resident grid's bytes; null: occlude == 0
    int dimX, dimY, dimZ;
    int loX, loY, loZ, hiX, hiY, hiZ;     // the box [lo, hi): the clip box or the grid
    int nbx, nby;
    int validLo, validHi;
    int scale;
    int rangeLo, rangeHi;
    int useTable;                 // 0: rto_debug_set_projection_table(ctx, 0), no brick is skipped
    unsigned stop;
    const uint2* bricks;          // (largest key, largest ~key) per brick
    const unsigned char* solid;   // 1: the brick holds a FILLED voxel; read only with vox
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
    const Ray r = t.r;
    const bool inFrame = t.in;
    const int lane = threadIdx.x & 63;

    // section 28's entry, with its helpers
    ProjectAxis X, Y, Z;
    float inX, inY, inZ, outX, outY, outZ;
    bool needX, needY, needZ;
    bool alive = inFrame && __builtin_isfinite(r.ox) && __builtin_isfinite(r.oy) && __builtin_isfinite(r.oz);
    const bool okX = project_axis_init(X, G.vs, r.ox, r.ix, G.gx, A.dimX, A.loX, A.hiX, inX, outX, needX);
    const bool okY = project_axis_init(Y, G.vs, r.oy, r.iy, G.gy, A.dimY, A.loY, A.hiY, inY, outY, needY);
    const bool okZ = project_axis_init(Z, G.vs, r.oz, r.iz, G.gz, A.dimZ, A.loZ, A.hiZ, inZ, outZ, needZ);
    alive = alive && okX && okY && okZ && (X.moving || Y.moving || Z.moving);
    float eT = 0.0f;
    int eAxis = 3;
    if (needX) { eT = inX; eAxis = 0; }
    if (needY && (eAxis == 3 || inY >= eT)) { eT = inY; eAxis = 1; }
    if (needZ && (eAxis == 3 || inZ >= eT)) { eT = inZ; eAxis = 2; }
    if (eAxis != 3) {
        if (X.moving && eAxis != 0) alive = alive && eT < outX;
        if (Y.moving && eAxis != 1) alive = alive && (eT < outY || (eT == outY && eAxis < 1));
        if (Z.moving && eAxis != 2) alive = alive && (eT < outZ || (eT == outZ && eAxis < 2));
    }
    if (alive) {
        if (X.moving) { X.c = eAxis == 0 ? (X.up ? X.lo : X.hi - 1) : (X.up ? project_rank(X, G.vs, eT, 0 < eAxis) - 1 : X.dim - project_rank(X, G.vs, eT, 0 < eAxis)); }
        if (Y.moving) { Y.c = eAxis == 1 ? (Y.up ? Y.lo : Y.hi - 1) : (Y.up ? project_rank(Y, G.vs, eT, 1 < eAxis) - 1 : Y.dim - project_rank(Y, G.vs, eT, 1 < eAxis)); }
        if (Z.moving) { Z.c = eAxis == 2 ? (Z.up ? Z.lo : Z.hi - 1) : (Z.up ? project_rank(Z, G.vs, eT, 2 < eAxis) - 1 : Z.dim - project_rank(Z, G.vs, eT, 2 < eAxis)); }
        project_arm(X, G.vs); project_arm(Y, G.vs); project_arm(Z, G.vs);
        alive = project_inside(X) && project_inside(Y) && project_inside(Z);
    }
    const bool visited = alive;

    unsigned T = 65536u, R = 0u, Gc = 0u, B = 0u;
    int count = 0, firstVox = -1, stopVox = -1;
    bool saturated = false, occluded = false;
    int lastBrick = -1;
    bool skip = false;
    int budget = A.dimX + A.dimY + A.dimZ + 4;        // no walk has more states
    while (alive) {
        const int brick = ((Z.c >> 3) * A.nby + (Y.c >> 3)) * A.nbx + (X.c >> 3);
        if (brick != lastBrick) {
            lastBrick = brick;
            skip = false;
            if (A.useTable) {
                const uint2 k = A.bricks[brick];
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
            // the brick's exit event, as k_project_march takes it
            const int jx = project_brick_exit(X), jy = project_brick_exit(Y), jz = project_brick_exit(Z);
            const unsigned tx = X.moving ? __float_as_uint(project_t(X, G.vs, jx)) : kProjectStill;
            const unsigned ty = Y.moving ? __float_as_uint(project_t(Y, G.vs, jy)) : kProjectStill;
            const unsigned tz = Z.moving ? __float_as_uint(project_t(Z, G.vs, jz)) : kProjectStill;
            if (tx <= ty && tx <= tz) {
                project_catch_up(Y, G.vs, tx, false); project_catch_up(Z, G.vs, tx, false);
                X.c = X.up ? jx : jx - 1; project_arm(X, G.vs);
            } else if (ty <= tz) {
                project_catch_up(X, G.vs, ty, true); project_catch_up(Z, G.vs, ty, false);
                Y.c = Y.up ? jy : jy - 1; project_arm(Y, G.vs);
            } else {
                project_catch_up(X, G.vs, tz, true); project_catch_up(Y, G.vs, tz, true);
                Z.c = Z.up ? jz : jz - 1; project_arm(Z, G.vs);
            }
        } else {
            const int idx = (Z.c * A.dimY + Y.c) * A.dimX + X.c;        // < 2^31 (composite_check)
            const int v = A.volume[idx];
            if (A.vox && A.vox[idx] == 1) { occluded = true; stopVox = idx; break; }
            if (v >= A.validLo && v <= A.validHi) {
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
            if (X.next <= Y.next && X.next <= Z.next) project_step(X, G.vs);
            else if (Y.next <= Z.next) project_step(Y, G.vs);
            else project_step(Z, G.vs);
        }
        alive = project_inside(X) && project_inside(Y) && project_inside(Z) && --budget > 0;
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
    if (!f || !v || !lut || !rgba) return fail(c, RTO_E_INVALID, name + ": NULL frame, composite, LUT or output");
    if (v->source < RTO_FIELD_DISTANCE || v->source > RTO_FIELD_CALLER) return fail(c, RTO_E_INVALID, name + ": unknown source " + std::to_string(v->source));
    if (v->scale < RTO_SCALE_LINEAR || v->scale > RTO_SCALE_CATEGORY) return fail(c, RTO_E_INVALID, name + ": unknown scale " + std::to_string(v->scale));
    for (int r : v->reserved) if (r != 0) return fail(c, RTO_E_INVALID, name + ": composite.reserved must be 0");
    if (v->valid_lo > v->valid_hi || v->valid_lo <= RTO_FIELD_PIXEL_NONE)
        return fail(c, RTO_E_INVALID, name + ": valid_lo must be above INT32_MIN + 1 and at most valid_hi");
    if (v->scale != RTO_SCALE_CATEGORY && v->range_lo >= v->range_hi)
        return fail(c, RTO_E_INVALID, name + ": a composite has no auto range: LINEAR and SQRT need range_lo < range_hi");
    if (v->stop_q16 < 0 || v->stop_q16 > 65535) return fail(c, RTO_E_INVALID, name + ": stop_q16 must be 0 .. 65535");
    if (v->occlude != 0 && v->occlude != 1) return fail(c, RTO_E_INVALID, name + ": occlude must be 0 or 1");
    int rc = frame_bound_check(c, name, f, 1);
    if (rc != RTO_OK) return rc;
    if (v->source == RTO_FIELD_CALLER && !d_volume) return fail(c, RTO_E_INVALID, name + ": RTO_FIELD_CALLER needs a volume");
    if (v->source != RTO_FIELD_CALLER && d_volume) return fail(c, RTO_E_INVALID, name + ": a volume goes with RTO_FIELD_CALLER only");
    if (c->numNodes <= 0) return fail(c, RTO_E_NO_OCTREE, name + ": no octree uploaded");
    if (!c->d_vox) return fail(c, RTO_E_UNSUPPORTED, name + ": the octree came from rto_upload_octree: no voxel grid is resident");
    if (grid_voxels(c) > 0x7fffffffll) return fail(c, RTO_E_UNSUPPORTED, name + ": the grid has 2^31 voxels or more: a voxel's index does not fit d_first");
    if (v->clip)
        for (int a = 0; a < 3; a++)
            if (v->clip_lo[a] < 0 || v->clip_hi[a] > c->voxDim[a] || v->clip_lo[a] >= v->clip_hi[a])
                return fail(c, RTO_E_INVALID, name + ": the clip box needs 0 <= clip_lo < clip_hi <= dim on every axis");
    return field_view_volume(c, fn, v->source, d_volume, volume);
}

// The solid table and the summary block, kept on the context under the field views' rules for work buffers (the brick table is the
// projections': project_reserve).
static int composite_reserve(rto_context* c, const char* fn, size_t bricks, hipStream_t s) {
    int rc = project_reserve(c, fn, bricks, s);
    if (rc != RTO_OK) return rc;
    if (c->cpSolidCap >= bricks && c->d_cpSum) return RTO_OK;
    if (stream_is_capturing(s))
        return fail(c, RTO_E_UNSUPPORTED, std::string(fn) + ": a larger grid allocates the solid table; composite one frame of it "
                                          "before hipStreamBeginCapture");
    if (!c->d_cpSum) {
        RTO_HIP(c, hipMalloc(&c->d_cpSum, rto::kFieldSlots * sizeof(rto::CompositeSumRaw)));
        for (hipEvent_t& e : c->cpEv) RTO_HIP(c, hipEventCreate(&e));
    }
    if (c->cpSolidCap < bricks) {
        (void)hipFree(c->d_cpSolid); c->d_cpSolid = nullptr;       // hipFree waits for the device: no frame still reads it
        c->cpSolidCap = 0;
        RTO_HIP(c, hipMalloc(&c->d_cpSolid, bricks));
        c->cpSolidCap = bricks;
    }
    return RTO_OK;
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
    const int nbx = (c->voxDim[0] + 7) / 8, nby = (c->voxDim[1] + 7) / 8, nbz = (c->voxDim[2] + 7) / 8;
    if ((rc = composite_reserve(c, fn, (size_t)nbx * (size_t)nby * (size_t)nbz, s)) != RTO_OK) return rc;
    CompositeArgs A;
    A.volume = volume;
    A.vox = v->occlude ? c->d_vox : nullptr;
    A.dimX = c->voxDim[0]; A.dimY = c->voxDim[1]; A.dimZ = c->voxDim[2];
    A.loX = v->clip ? v->clip_lo[0] : 0; A.loY = v->clip ? v->clip_lo[1] : 0; A.loZ = v->clip ? v->clip_lo[2] : 0;
    A.hiX = v->clip ? v->clip_hi[0] : A.dimX; A.hiY = v->clip ? v->clip_hi[1] : A.dimY; A.hiZ = v->clip ? v->clip_hi[2] : A.dimZ;
    A.nbx = nbx; A.nby = nby;
    A.validLo = v->valid_lo; A.validHi = v->valid_hi;
    A.scale = v->scale;
    A.rangeLo = v->range_lo; A.rangeHi = v->range_hi;
    A.useTable = c->pjTable ? 1 : 0;
    A.stop = (unsigned)v->stop_q16;
    A.bricks = c->d_pjBricks; A.solid = c->d_cpSolid;
    A.lut = d_lut;
    A.under = d_under; A.rgba = d_rgba;
    A.trans = d_trans; A.first = d_first; A.stops = d_stops; A.counts = d_counts;
    std::memcpy(A.bg, v->background_rgba, sizeof A.bg);
    std::memcpy(A.miss, v->miss_rgba, sizeof A.miss);
    A.sum = reinterpret_cast<CompositeSumRaw*>(c->d_cpSum);

    const bool timed = !(stream_is_capturing(s) || c->eventsOff);
    RTO_HIP(c, hipMemsetAsync(c->d_cpSum, 0, kFieldSlots * sizeof(CompositeSumRaw), s));
    if (timed) RTO_HIP(c, hipEventRecord(c->cpEv[0], s));
    if (A.useTable) {
        const int runsX = (nbx + 7) / 8;
        const int64_t waves = (int64_t)runsX * nby * nbz;             // the grid has fewer than 2^31 voxels
        const dim3 grid((unsigned)((waves + kBlock / kWave - 1) / (kBlock / kWave)));
        hipLaunchKernelGGL(k_project_bricks, grid, dim3(kBlock), 0, s, volume, A.dimX, A.dimY, A.dimZ, nbx, nby, runsX, (unsigned)waves,
                           A.validLo, A.validHi, c->d_pjBricks);
        RTO_HIP(c, hipGetLastError());
        if (A.vox) {
            // the widest load that every row of the grid starts aligned to
            const uintptr_t align = (uintptr_t)A.dimX | reinterpret_cast<uintptr_t>(c->d_vox);
            if (align % 16 == 0) composite_solid_launch<16>(c, nbx, nby, nbz, s);
            else if (align % 8 == 0) composite_solid_launch<8>(c, nbx, nby, nbz, s);
            else if (align % 4 == 0) composite_solid_launch<4>(c, nbx, nby, nbz, s);
            else if (align % 2 == 0) composite_solid_launch<2>(c, nbx, nby, nbz, s);
            else composite_solid_launch<1>(c, nbx, nby, nbz, s);
            RTO_HIP(c, hipGetLastError());
        }
    }
    if (timed) RTO_HIP(c, hipEventRecord(c->cpEv[1], s));
    const int64_t tiles = (int64_t)P.tilesX * P.tilesY;
    const dim3 grid((unsigned)((tiles + kBlock / kWave - 1) / (kBlock / kWave)));
    hipLaunchKernelGGL(k_composite_march, grid, dim3(kBlock), 0, s, P, A);
    RTO_HIP(c, hipGetLastError());
    if (timed) RTO_HIP(c, hipEventRecord(c->cpEv[2], s));
    if (d_summary) {
        hipLaunchKernelGGL(k_composite_fold, dim3(1), dim3(kWave), 0, s, A.sum, d_summary);
        RTO_HIP(c, hipGetLastError());
    }
    if (timed) RTO_HIP(c, hipEventRecord(c->cpEv[3], s));
    c->cpTimed = timed;
    return RTO_OK;
}

extern "C" {

int rto_composite_field_device(rto_context* c, const rto_frame* frame, const rto_field_composite* comp, const uint32_t* d_lut,
                               const int32_t* d_volume, const void* d_under, void* d_rgba, uint32_t* d_transmittance, int32_t* d_first,
                               int32_t* d_stops, int32_t* d_counts, rto_composite_summary* d_summary, void* hip_stream) {
    if (!c) return RTO_E_INVALID;
    const char* fn = "rto_composite_field_device";
    auto off = [](const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
    if (frame && comp && d_lut && d_rgba &&
        (off(d_rgba, 15) || off(d_under, 15) || off(d_lut, 3) || off(d_volume, 3) || off(d_transmittance, 3) || off(d_first, 3) || off(d_stops, 3) ||
         off(d_counts, 3) || off(d_summary, 7)))
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
    const size_t pixels = (size_t)frame->width * (size_t)frame->height;
    BuildScratch scratch(c->stream);
    float4 *d_rgba = nullptr, *d_under = nullptr;
    uint32_t* d_trans = nullptr;
    int32_t *d_first = nullptr, *d_stops = nullptr, *d_counts = nullptr;
    unsigned* d_lut = nullptr;
    rto_composite_summary* d_summary = nullptr;
    RTO_HIP(c, scratch.alloc(&d_rgba, pixels));
    RTO_HIP(c, scratch.alloc(&d_lut, 256));
    if (host_transmittance) RTO_HIP(c, scratch.alloc(&d_trans, pixels));
    if (host_first) RTO_HIP(c, scratch.alloc(&d_first, pixels));
    if (host_stops) RTO_HIP(c, scratch.alloc(&d_stops, pixels));
    if (host_counts) RTO_HIP(c, scratch.alloc(&d_counts, pixels));
    if (host_summary) RTO_HIP(c, scratch.alloc(&d_summary, 1));
    if (host_under) {                                                // under the frame itself: composited in place on the device too
        if (host_under == host_rgba) d_under = d_rgba;
        else RTO_HIP(c, scratch.alloc(&d_under, pixels));
        RTO_HIP(c, hipMemcpyAsync(d_under, host_under, pixels * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    }
    RTO_HIP(c, hipMemcpyAsync(d_lut, lut, 256 * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    if (host_volume) {                                               // RTO_FIELD_CALLER (composite_check)
        int32_t* d_volume = nullptr;
        RTO_HIP(c, scratch.alloc(&d_volume, (size_t)grid_voxels(c)));
        RTO_HIP(c, hipMemcpyAsync(d_volume, host_volume, (size_t)grid_voxels(c) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        volume = d_volume;
    }
    if ((rc = composite_field(c, fn, frame, comp, d_lut, volume, d_under, d_rgba, d_trans, d_first, d_stops, d_counts, d_summary, c->stream)) != RTO_OK)
        return rc;
    RTO_HIP(c, hipMemcpyAsync(host_rgba, d_rgba, pixels * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    if (host_transmittance) RTO_HIP(c, hipMemcpyAsync(host_transmittance, d_trans, pixels * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (host_first) RTO_HIP(c, hipMemcpyAsync(host_first, d_first, pixels * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (host_stops) RTO_HIP(c, hipMemcpyAsync(host_stops, d_stops, pixels * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (host_counts) RTO_HIP(c, hipMemcpyAsync(host_counts, d_counts, pixels * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (host_summary) RTO_HIP(c, hipMemcpyAsync(host_summary, d_summary, sizeof *host_summary, hipMemcpyDeviceToHost, c->stream));
    RTO_HIP(c, hipStreamSynchronize(c->stream));
    return RTO_OK;
}

int rto_last_composite_ms(const rto_context* c, float ms[3]) {
    if (!c || !ms) return RTO_E_INVALID;
    ms[0] = ms[1] = ms[2] = -1.0f;
    if (!c->cpTimed) return RTO_OK;
    if (hipEventSynchronize(c->cpEv[3]) != hipSuccess) return RTO_E_HIP;
    for (int k = 0; k < 3; k++)
        if (hipEventElapsedTime(&ms[k], c->cpEv[k], c->cpEv[k + 1]) != hipSuccess) {
            ms[0] = ms[1] = ms[2] = -1.0f;
            return RTO_E_HIP;
        }
    return RTO_OK;
}

}  // extern "C"
