// rto_field_view.inc -- field views (include/rto_hip.h, rto_render_field_*): a frame of the octree coloured by an int32 volume of the
// resident grid (a resident field, the component labels or a caller's volume).  Included at the end of rto_api.hip, after
// rto_lit.inc (lit_mix32, and of its frame pass tile_pixel, rooted_box_walk, kLargestBelow1e30, frame_bound_check and
// frame_tree_check) and rto_query.inc (query_face).  Its host side also holds what the field projections and composites share
// with it (field_frame_check and its pieces, work_buffer, stage_events, HostStage, misaligned); their voxel walk is
// rto_voxel_walk.inc, the stage timer (StageEvents) rto_api.hip.
//
// Rule (DESIGN.md section 27).  The hit is the box query of view.mode on the frame's pixel ray in the window the clip box leaves;
// the voxel of the hit is floor((p - gridMin) / voxelSize) of p = o + d tHit, clamped into the leaf (and the clip box), with the
// entry face's axis taken from the leaf's own boundary; HIT samples it, FRONT its neighbour across the entry face.  The value goes
// through [valid_lo, valid_hi], the range (the caller's, or the frame's own minimum and maximum) and the scale to one of 256 LUT
// entries.  Integers end to end; the floats are the ray, the window, p and the Lambert term.
//
// Kernels (one stream, no host step):
//   k_field_sample  one lane per pixel, 8x8 tiles per wave, k_lit_primary's stacks: the walk, the voxel rule, one 4-byte gather and
//                   one int32 store per pixel (with view.shade one float more: the Lambert term, parked in the pixel's red channel
//                   for the second pass).  hits, valued, minimum and maximum are reduced per wave and reach the context's summary
//                   block with one 64-bit add (both counts) and, only while they still move an extreme, an atomic max each.  The
//                   block is kFieldSlots records on cache lines of their own, a wave's picked by its workgroup: every wave of a
//                   frame adding to one word ran at the rate of that word (config 2 at 1080p: 0.27 ms against 0.09 for the walk).
//   k_field_shade   persistent workgroups over the pixels: the 256 LUT entries are converted to float4 once per workgroup (one per
//                   thread), wave 0 folds the summary block's records, values go to indices, colours and -- if asked for -- to 256
//                   LDS bins that reach d_bins with one atomic per non-zero bin.  Thread 0 of workgroup 0 writes the caller's summary.

namespace rto {

constexpr int kFieldMiss = RTO_FIELD_PIXEL_MISS, kFieldNone = RTO_FIELD_PIXEL_NONE;

// One record of the summary block while a frame is in flight; the block is zeroed in front of the frame.  counts = hits | valued
// << 32 (both below 2^32: field_check).  The extremes are kept as unsigned keys that only grow, so that zero is their start
// value: key(v) = v ^ 0x80000000 orders int32 as unsigned; maxKey holds the largest key and minInv the largest ~key.  No valued
// pixel has key 0 (valid_lo > INT32_MIN + 1), and ~key = 0 is INT32_MAX, which is what "nothing below it" decodes to anyway.
struct alignas(128) FieldSumRaw {
    unsigned long long counts;
    unsigned maxKey, minInv;
};
constexpr int kFieldSlots = kWave;       // one wave folds them

struct FieldArgs {
    const int* volume;       // dimZ x dimY x dimX, x fastest
    int dimX, dimY, dimZ;
    int sample, shade, clip;
    int validLo, validHi;
    int clipLo[3], clipHi[3];
    float planeLo[3], planeHi[3];   // the clip box's planes, gridMin[a] + (float)i * voxelSize
    int rootLeaf;            // 1: the tree is one leaf, nodes[0]
    const rto_node* nodes;
    int* values;             // the caller's d_values or the context's buffer
    float* ndotl;            // the frame's rgba buffer (4 floats per pixel): [4 pix] takes the Lambert term when shade
    FieldSumRaw* sum;
};

// One axis of the voxel of the hit: floor((p - g) / vs) clamped in float into [lo, hi] (a NaN goes to lo), then into the clip box.
__device__ __forceinline__ int field_axis(float p, float g, float vs, int lo, int hi, bool clip, int clo, int chi) {
    float q = __builtin_floorf((p - g) / vs);
    const float flo = (float)lo, fhi = (float)hi;
    q = q >= flo ? q : flo;
    q = q > fhi ? fhi : q;
    int v = (int)q;
    if (clip) { v = v < clo ? clo : v; v = v > chi - 1 ? chi - 1 : v; }
    return v;
}

template <int QMODE>
__global__ __launch_bounds__(kBlock) void k_field_sample(RenderParams P, FieldArgs A, const uint2* __restrict__ desc) {
    extern __shared__ uint2 lds_stack[];
    uint2* stk;
    unsigned* stkNode;
    desc_stacks(lds_stack, P.depth, stk, stkNode);
    const Geo G = geo_of(P);
    const int lane = threadIdx.x & 63;
    const TilePixel t = tile_pixel(P);
    const Ray r = t.r;
    const bool inFrame = t.in;
    // the window: (0, below 1e30), or what the clip box leaves of it
    float tlo = 0.0f, thi = kLargestBelow1e30;
    bool valid = inFrame;
    if (A.clip && inFrame) {
        const float t1x = (A.planeLo[0] - r.ox) * r.ix, t2x = (A.planeHi[0] - r.ox) * r.ix;
        const float t1y = (A.planeLo[1] - r.oy) * r.iy, t2y = (A.planeHi[1] - r.oy) * r.iy;
        const float t1z = (A.planeLo[2] - r.oz) * r.iz, t2z = (A.planeHi[2] - r.oz) * r.iz;
        const float tNear = gmax(gmax(gmin(t1x, t2x), gmin(t1y, t2y)), gmin(t1z, t2z));
        const float tFar = gmin(gmin(gmax(t1x, t2x), gmax(t1y, t2y)), gmax(t1z, t2z));
        valid = tNear <= tFar && tFar > 0.0f;
        tlo = gmax(0.0f, tNear);
        thi = gmin(thi, tFar);
    }
    const DescHit w = rooted_box_walk<QMODE>(P, G, r, tlo, thi, valid, A.rootLeaf, A.nodes, desc, stk, stkNode);

    int value = kFieldMiss;
    float ndotl = 0.0f;
    if (w.hit) {
        const int face = query_face(G, r, w.x, w.y, w.z, w.size, w.t);
        if (A.shade) ndotl = shade_term(P, G, r, w.x, w.y, w.z, w.size);
        const float hx = r.ox + r.dx * w.t, hy = r.oy + r.dy * w.t, hz = r.oz + r.dz * w.t;
        const int top = w.size - 1;
        int vx = field_axis(hx, G.gx, G.vs, w.x, w.x + top, A.clip != 0, A.clipLo[0], A.clipHi[0]);
        int vy = field_axis(hy, G.gy, G.vs, w.y, w.y + top, A.clip != 0, A.clipLo[1], A.clipHi[1]);
        int vz = field_axis(hz, G.gz, G.vs, w.z, w.z + top, A.clip != 0, A.clipLo[2], A.clipHi[2]);
        bool have = true;
        if (face >= 0) {
            const int a = face >> 1;
            const bool up = (face & 1) != 0;
            const int step = A.sample == RTO_SAMPLE_FRONT ? (up ? 1 : -1) : 0;
            if (a == 0) vx = (up ? w.x + top : w.x) + step;
            else if (a == 1) vy = (up ? w.y + top : w.y) + step;
            else vz = (up ? w.z + top : w.z) + step;
        } else if (A.sample == RTO_SAMPLE_FRONT) {
            have = false;
        }
        // no voxel outside the grid: FRONT's neighbour across a grid face, and nothing else a canonical tree of the grid can give
        have = have && vx >= 0 && vx < A.dimX && vy >= 0 && vy < A.dimY && vz >= 0 && vz < A.dimZ;
        value = kFieldNone;
        if (have) {
            const int v = A.volume[((size_t)vz * (size_t)A.dimY + (size_t)vy) * (size_t)A.dimX + (size_t)vx];
            if (v >= A.validLo && v <= A.validHi) value = v;
        }
    }
    if (inFrame) {
        const unsigned pix = (unsigned)t.py * (unsigned)P.W + (unsigned)t.px;   // < 2^32 (field_check)
        A.values[pix] = value;
        if (A.shade) A.ndotl[4 * (size_t)pix] = ndotl;
    }
    // the frame's summary: per wave one add for both counts, and an atomic max only for an extreme the record does not hold yet
    // (the keys only grow, so a stale read can cost a needless atomic, never lose one)
    const bool isHit = inFrame && value != kFieldMiss, isVal = isHit && value != kFieldNone;
    const unsigned key = (unsigned)value ^ 0x80000000u;
    const unsigned nHit = wave_sum(isHit ? 1u : 0u), nVal = wave_sum(isVal ? 1u : 0u);
    const unsigned kMax = wave_max(isVal ? key : 0u), kInv = wave_max(isVal ? ~key : 0u);
    if (lane == 0 && nHit) {
        FieldSumRaw* slot = A.sum + blockIdx.x % kFieldSlots;
        atomicAdd(&slot->counts, (unsigned long long)nHit | ((unsigned long long)nVal << 32));
        if (nVal) {
            if (kMax > *reinterpret_cast<volatile unsigned*>(&slot->maxKey)) atomicMax(&slot->maxKey, kMax);
            if (kInv > *reinterpret_cast<volatile unsigned*>(&slot->minInv)) atomicMax(&slot->minInv, kInv);
        }
    }
}

struct ShadeArgs {
    const int* values;
    const unsigned* lut;     // 256 entries, bytes r, g, b, a in memory order
    float4* rgba;
    const FieldSumRaw* sum;
    rto_field_view_summary* outSum;     // may be null
    unsigned long long* bins;           // 256, may be null
    unsigned pixels;
    int scale, shade;
    int rangeLo, rangeHi;    // equal: the frame's own minimum and maximum
    float miss[4], none[4];
};

// The largest k in 0..255 with k * m(k) * s <= rhs, m(k) = k under SQRT and 1 under LINEAR; all in int64 (s <= 2^32 - 1,
// k * k * s < 2^48, rhs <= 65025 (2^32 - 1)).  LINEAR's answer is floor(w * 255 / s) because w <= s.
template <bool SQRT>
__device__ __forceinline__ int field_search(long long s, long long rhs) {
    int k = 0;
#pragma unroll
    for (int bit = 128; bit > 0; bit >>= 1) {
        const int t = k | bit;
        const long long lhs = (long long)(SQRT ? t * t : t) * s;
        if (lhs <= rhs) k = t;
    }
    return k;
}

__global__ __launch_bounds__(kBlock) void k_field_shade(ShadeArgs S) {
    __shared__ float4 lutF[256];
    __shared__ unsigned bins[256];
    __shared__ unsigned long long sumCounts;
    __shared__ unsigned sumMax, sumInv;
    static_assert(kBlock == 256, "one thread per LUT entry and bin");
    {
        const unsigned e = S.lut[threadIdx.x];
        lutF[threadIdx.x] = make_float4((float)(e & 255u) / 255.0f, (float)((e >> 8) & 255u) / 255.0f,
                                        (float)((e >> 16) & 255u) / 255.0f, (float)(e >> 24) / 255.0f);
        bins[threadIdx.x] = 0u;
    }
    if (threadIdx.x < kFieldSlots) {                             // wave 0, whole: the block's records folded
        const FieldSumRaw* slot = S.sum + threadIdx.x;
        const unsigned long long n = wave_sum(slot->counts);
        const unsigned kMax = wave_max(slot->maxKey), kInv = wave_max(slot->minInv);
        if (threadIdx.x == 0) { sumCounts = n; sumMax = kMax; sumInv = kInv; }
    }
    __syncthreads();
    // the summary, decoded; every thread needs the range
    const unsigned long long hits = sumCounts & 0xffffffffull, valued = sumCounts >> 32;
    const int vmin = valued ? (int)(~sumInv ^ 0x80000000u) : 0, vmax = valued ? (int)(sumMax ^ 0x80000000u) : 0;
    const bool autoRange = S.rangeLo == S.rangeHi;
    const int lo = autoRange ? vmin : S.rangeLo, hi = autoRange ? vmax : S.rangeHi;
    if (S.outSum && blockIdx.x == 0 && threadIdx.x == 0) {
        rto_field_view_summary o;
        o.hits = (int64_t)hits; o.valued = (int64_t)valued;
        o.vmin = vmin; o.vmax = vmax; o.lo = lo; o.hi = hi;
        *S.outSum = o;
    }
    const long long s = (long long)hi - (long long)lo;
    const unsigned stride = gridDim.x * blockDim.x;
    // the step never wraps: pixels + 128 < 2^32 (field_check) and the grid holds at most `pixels` threads rounded up to a workgroup
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < S.pixels; i = S.pixels - i > stride ? i + stride : S.pixels) {
        const int v = S.values[i];
        float4 c;
        if (v == kFieldMiss) {
            c = make_float4(S.miss[0], S.miss[1], S.miss[2], S.miss[3]);
        } else if (v == kFieldNone) {
            c = make_float4(S.none[0], S.none[1], S.none[2], S.none[3]);
        } else {
            int k;
            if (S.scale == RTO_SCALE_CATEGORY) {
                k = (int)(lit_mix32((unsigned)v) & 255u);
            } else if (s == 0) {
                k = 0;
            } else {
                const long long cl = v < lo ? lo : (v > hi ? hi : v);
                const long long wv = cl - (long long)lo;
                k = S.scale == RTO_SCALE_SQRT ? field_search<true>(s, wv * 65025ll) : field_search<false>(s, wv * 255ll);
            }
            c = lutF[k];
            if (S.shade) {
                const float m = 0.25f + 0.75f * reinterpret_cast<const float*>(S.rgba)[4 * (size_t)i];
                c.x = c.x * m; c.y = c.y * m; c.z = c.z * m;
            }
            if (S.bins) atomicAdd(&bins[k], 1u);
        }
        S.rgba[i] = c;
    }
    if (S.bins) {
        __syncthreads();
        const unsigned n = bins[threadIdx.x];
        if (n) atomicAdd(S.bins + threadIdx.x, (unsigned long long)n);
    }
}

}  // namespace rto

// ---------------------------------------------------------------- host side
static_assert(sizeof(rto_field_view) == 112 && sizeof(rto_field_view_summary) == 32, "the ABI's sizes");

// The view's volume, or the reader's own refusal.
static int field_view_volume(rto_context* c, const char* fn, int source, const int32_t* d_volume, const int** out) {
    if (source == RTO_FIELD_CALLER) { *out = d_volume; return RTO_OK; }
    if (source == RTO_FIELD_LABELS) {
        if (!c->d_ccLabels)
            return fail(c, RTO_E_INVALID, std::string(fn) + ": no labels are resident (not labelled yet, or the grid has changed since)");
        *out = c->d_ccLabels;
        return RTO_OK;
    }
    const int rc = resident_field_check(c, fn, (FieldSlot)source);
    if (rc == RTO_OK) *out = c->d_field[source];
    return rc;
}

// ---- the refusals the volume entry points share (the field frames below; iso_check where its own promised order allows)
static int check_valid_window(rto_context* c, const std::string& name, int lo, int hi) {
    if (lo > hi || lo <= RTO_FIELD_PIXEL_NONE) return fail(c, RTO_E_INVALID, name + ": valid_lo must be above INT32_MIN + 1 and at most valid_hi");
    return RTO_OK;
}

static int check_caller_volume(rto_context* c, const std::string& name, int source, const void* given) {
    if (source == RTO_FIELD_CALLER && !given) return fail(c, RTO_E_INVALID, name + ": RTO_FIELD_CALLER needs a volume");
    if (source != RTO_FIELD_CALLER && given) return fail(c, RTO_E_INVALID, name + ": a volume goes with RTO_FIELD_CALLER only");
    return RTO_OK;
}

static int check_clip_box(rto_context* c, const std::string& name, int clip, const int* lo, const int* hi) {
    if (clip)
        for (int a = 0; a < 3; a++)
            if (lo[a] < 0 || hi[a] > c->voxDim[a] || lo[a] >= hi[a])
                return fail(c, RTO_E_INVALID, name + ": the clip box needs 0 <= clip_lo < clip_hi <= dim on every axis");
    return RTO_OK;
}

// The range rule of views and projections.
static int check_range_order(rto_context* c, const std::string& name, int lo, int hi) {
    return lo > hi ? fail(c, RTO_E_INVALID, name + ": range_lo > range_hi") : RTO_OK;
}

// The preconditions of projections and composites: a resident grid whose voxel indices fit the int32 output `word` names.
static int check_grid_index(rto_context* c, const std::string& name, const char* word) {
    if (c->numNodes <= 0) return fail(c, RTO_E_NO_OCTREE, name + ": no octree uploaded");
    if (!c->d_vox) return fail(c, RTO_E_UNSUPPORTED, name + ": the octree came from rto_upload_octree: no voxel grid is resident");
    if (grid_voxels(c) > 0x7fffffffll)
        return fail(c, RTO_E_UNSUPPORTED, name + ": the grid has 2^31 voxels or more: a voxel's index does not fit " + word);
    return RTO_OK;
}

// Every check of a field frame, in the order the ABI promises to views, projections and composites alike; V is the family's struct
// and `what` its name in the messages.  A family's own lines go into three slots: enums (after the source), range (after the valid
// window) and pre (the tree and grid preconditions, after the caller's volume).  *volume: the int32 volume the frame reads.
template <class V, class Enums, class Range, class Pre>
static int field_frame_check(rto_context* c, const std::string& name, const char* what, const rto_frame* f, const V* v, const void* lut,
                             const int32_t* d_volume, const void* rgba, const int** volume, Enums enums, Range range, Pre pre) {
    if (!f || !v || !lut || !rgba) return fail(c, RTO_E_INVALID, name + ": NULL frame, " + what + ", LUT or output");
    if (v->source < RTO_FIELD_DISTANCE || v->source > RTO_FIELD_CALLER) return fail(c, RTO_E_INVALID, name + ": unknown source " + std::to_string(v->source));
    int rc = enums();
    if (rc != RTO_OK) return rc;
    if (v->scale < RTO_SCALE_LINEAR || v->scale > RTO_SCALE_CATEGORY) return fail(c, RTO_E_INVALID, name + ": unknown scale " + std::to_string(v->scale));
    for (int r : v->reserved) if (r != 0) return fail(c, RTO_E_INVALID, name + ": " + what + ".reserved must be 0");
    if ((rc = check_valid_window(c, name, v->valid_lo, v->valid_hi)) != RTO_OK || (rc = range()) != RTO_OK ||
        (rc = frame_bound_check(c, name, f, 1)) != RTO_OK || (rc = check_caller_volume(c, name, v->source, d_volume)) != RTO_OK ||
        (rc = pre()) != RTO_OK || (rc = check_clip_box(c, name, v->clip, v->clip_lo, v->clip_hi)) != RTO_OK)
        return rc;
    return field_view_volume(c, name.c_str(), v->source, d_volume, volume);
}

static int field_check(rto_context* c, const char* fn, const rto_frame* f, const rto_field_view* v, const void* lut, const int32_t* d_volume,
                       const void* rgba, const int** volume) {
    const std::string name(fn);
    return field_frame_check(c, name, "view", f, v, lut, d_volume, rgba, volume,
        [&] {
            if (v->sample != RTO_SAMPLE_HIT && v->sample != RTO_SAMPLE_FRONT) return fail(c, RTO_E_INVALID, name + ": unknown sample " + std::to_string(v->sample));
            if (v->mode != RTO_QUERY_FIRST && v->mode != RTO_QUERY_CLOSEST) return fail(c, RTO_E_INVALID, name + ": mode must be RTO_QUERY_FIRST or RTO_QUERY_CLOSEST");
            return RTO_OK;
        },
        [&] { return check_range_order(c, name, v->range_lo, v->range_hi); },
        [&] { return frame_tree_check(c, name, true, ": a field view needs a canonical octree (descriptor tree)"); });
}

// ---- the work buffers a frame keeps on the context.  d must hold n elements: if it must grow and the stream is capturing, the call
// is refused with fn + why; otherwise it is freed, allocated anew and its capacity recorded.
template <class T>
static int work_buffer(rto_context* c, T*& d, size_t& cap, size_t n, hipStream_t s, const char* fn, const char* why) {
    if (cap >= n) return RTO_OK;
    if (stream_is_capturing(s)) return fail(c, RTO_E_UNSUPPORTED, std::string(fn) + why);
    (void)hipFree(d); d = nullptr;                       // hipFree waits for the device: no frame still reads it
    cap = 0;
    RTO_HIP(c, hipMalloc(&d, n * sizeof(T)));
    cap = n;
    return RTO_OK;
}

// A family's stage timer, made on first use: creating events is refused under capture with the buffers.
template <int N>
static int stage_events(rto_context* c, StageEvents<N>& ev, hipStream_t s, const char* fn, const char* why) {
    if (ev.ready()) return RTO_OK;
    if (stream_is_capturing(s)) return fail(c, RTO_E_UNSUPPORTED, std::string(fn) + why);
    RTO_HIP(c, ev.ensure());
    return RTO_OK;
}

// The work buffers of a field view: the summary block, the timing events and, for a caller without d_values, a value buffer that
// grows with the frame.
static int field_reserve(rto_context* c, const char* fn, size_t pixels, bool needValues, hipStream_t s) {
    const char* why = ": a larger frame allocates its work buffers; render one such frame before hipStreamBeginCapture";
    size_t sumCap = c->d_fvSum ? sizeof(FieldSumRaw[kFieldSlots]) : 0;              // the summary block: of one size, made once
    int rc = work_buffer(c, c->d_fvSum, sumCap, sizeof(FieldSumRaw[kFieldSlots]), s, fn, why);
    if (rc == RTO_OK) rc = stage_events(c, c->fvEv, s, fn, why);
    if (rc == RTO_OK && needValues) rc = work_buffer(c, c->d_fvValues, c->fvCap, pixels, s, fn, why);
    return rc;
}

// ---- the _host forms' staging: the frame and the LUT on the device, the outputs the caller asked for, the caller's volume; what
// was registered comes back in finish().  Device memory is the call's scratch.  The first HIP error sticks, with the call that
// failed, and makes everything after it a no-op: status(), asked once before the frame runs, reports it.
struct HostStage {
    rto_context* c;
    BuildScratch scratch;
    size_t pixels;
    hipError_t err = hipSuccess;
    const char* failed = nullptr;                        // the call that gave err
    struct Out { void* host; const void* dev; size_t bytes; };
    std::vector<Out> outs;
    float4* d_rgba;
    unsigned* d_lut;

    HostStage(rto_context* ctx, const rto_frame* f, const uint32_t* lut, float* host_rgba)
        : c(ctx), scratch(ctx->stream), pixels((size_t)f->width * (size_t)f->height) {
        d_rgba = optional(reinterpret_cast<float4*>(host_rgba), pixels);
        d_lut = upload(reinterpret_cast<const unsigned*>(lut), 256);
    }
    template <class T> T* device(size_t count) {
        T* d = nullptr;
        if (err == hipSuccess && (err = scratch.alloc(&d, count)) != hipSuccess) failed = "hipMallocAsync of a staging buffer";
        return d;
    }
    template <class T> void copy_in(T* d, const T* host, size_t count) {
        if (err == hipSuccess && (err = hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, c->stream)) != hipSuccess)
            failed = "hipMemcpyAsync of an input to its staging buffer";
    }
    template <class T> T* upload(const T* host, size_t count) {
        T* d = device<T>(count);
        copy_in(d, host, count);
        return d;
    }
    // an output the caller may leave out: its device buffer, downloaded by finish(), or null
    template <class T> T* optional(T* host, size_t count) {
        if (!host) return nullptr;
        T* d = device<T>(count);
        outs.push_back({ host, d, count * sizeof(T) });
        return d;
    }
    // the frame's volume: the caller's (RTO_FIELD_CALLER, the family's check), uploaded, or the resident one
    const int* volume(const int32_t* host_volume, const int* resident) {
        return host_volume ? upload(host_volume, (size_t)grid_voxels(c)) : resident;
    }
    int status() const { return err == hipSuccess ? RTO_OK : fail(c, RTO_E_HIP, std::string(failed) + ": " + hipGetErrorString(err)); }
    int finish() {
        for (const Out& o : outs) RTO_HIP(c, hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, c->stream));
        RTO_HIP(c, hipStreamSynchronize(c->stream));
        return RTO_OK;
    }
};

// Is a pointer off the alignment its mask asks for?  (A null one is not.)
static bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

static int render_field(rto_context* c, const char* fn, const rto_frame* f, const rto_field_view* v, const unsigned* d_lut, const int* volume,
                        float4* d_rgba, int32_t* d_values, rto_field_view_summary* d_summary, int64_t* d_bins, hipStream_t s) {
    RenderParams P;
    int rc = fill_params(c, f, nullptr, P, s);
    if (rc != RTO_OK) return rc;
    const size_t pixels = (size_t)P.W * (size_t)P.H;
    if ((rc = field_reserve(c, fn, pixels, d_values == nullptr, s)) != RTO_OK) return rc;
    FieldArgs A;
    A.volume = volume;
    A.dimX = c->voxDim[0]; A.dimY = c->voxDim[1]; A.dimZ = c->voxDim[2];
    A.sample = v->sample; A.shade = v->shade != 0 ? 1 : 0; A.clip = v->clip != 0 ? 1 : 0;
    A.validLo = v->valid_lo; A.validHi = v->valid_hi;
    for (int a = 0; a < 3; a++) {
        A.clipLo[a] = A.clip ? v->clip_lo[a] : 0;
        A.clipHi[a] = A.clip ? v->clip_hi[a] : c->voxDim[a];
        const volatile float lo = (float)A.clipLo[a] * c->voxelSize, hi = (float)A.clipHi[a] * c->voxelSize;   // one rounding each
        A.planeLo[a] = c->gridMin[a] + lo;
        A.planeHi[a] = c->gridMin[a] + hi;
    }
    A.rootLeaf = c->numNodes == 1 ? 1 : 0;
    A.nodes = c->d_nodes;
    A.values = d_values ? d_values : c->d_fvValues;
    A.ndotl = reinterpret_cast<float*>(d_rgba);
    A.sum = reinterpret_cast<FieldSumRaw*>(c->d_fvSum);
    ShadeArgs S;
    S.values = A.values; S.lut = d_lut; S.rgba = d_rgba; S.sum = A.sum; S.outSum = d_summary;
    S.bins = reinterpret_cast<unsigned long long*>(d_bins);
    S.pixels = (unsigned)pixels;
    S.scale = v->scale; S.shade = A.shade;
    S.rangeLo = v->range_lo; S.rangeHi = v->range_hi;
    std::memcpy(S.miss, v->miss_rgba, sizeof S.miss);
    std::memcpy(S.none, v->none_rgba, sizeof S.none);

    const bool timed = !(stream_is_capturing(s) || c->eventsOff);
    RTO_HIP(c, hipMemsetAsync(c->d_fvSum, 0, kFieldSlots * sizeof(FieldSumRaw), s));
    if (d_bins) RTO_HIP(c, hipMemsetAsync(d_bins, 0, 256 * sizeof(int64_t), s));
    RTO_HIP(c, c->fvEv.mark(0, s, timed));
    const size_t lds = desc_stack_bytes(P.depth);
    const int64_t tiles = (int64_t)P.tilesX * P.tilesY;
    const dim3 grid((unsigned)((tiles + kBlock / kWave - 1) / (kBlock / kWave)));
    if (v->mode == RTO_QUERY_FIRST) hipLaunchKernelGGL(k_field_sample<kQueryFirst>, grid, dim3(kBlock), lds, s, P, A, c->d_desc);
    else hipLaunchKernelGGL(k_field_sample<kQueryClosest>, grid, dim3(kBlock), lds, s, P, A, c->d_desc);
    RTO_HIP(c, hipGetLastError());
    RTO_HIP(c, c->fvEv.mark(1, s, timed));
    const int64_t blocks = std::min<int64_t>((int64_t)c->numCUs * 8, ((int64_t)pixels + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_field_shade, dim3((unsigned)blocks), dim3(kBlock), 0, s, S);
    RTO_HIP(c, hipGetLastError());
    RTO_HIP(c, c->fvEv.mark(2, s, timed));
    return RTO_OK;
}

extern "C" {

int rto_render_field_device(rto_context* c, const rto_frame* frame, const rto_field_view* view, const uint32_t* d_lut, const int32_t* d_volume,
                            void* d_rgba, int32_t* d_values, rto_field_view_summary* d_summary, int64_t* d_bins, void* hip_stream) {
    if (!c) return RTO_E_INVALID;
    const char* fn = "rto_render_field_device";
    if (frame && view && d_lut && d_rgba &&
        (misaligned(d_rgba, 15) || misaligned(d_lut, 3) || misaligned(d_volume, 3) || misaligned(d_values, 3) || misaligned(d_summary, 7) ||
         misaligned(d_bins, 7)))
        return fail(c, RTO_E_INVALID, std::string(fn) + ": d_rgba must be 16-byte, d_summary and d_bins 8-byte, d_lut, d_volume and d_values 4-byte aligned");
    const int* volume = nullptr;
    const int rc = field_check(c, fn, frame, view, d_lut, d_volume, d_rgba, &volume);
    if (rc != RTO_OK) return rc;
    RTO_HIP(c, hipSetDevice(c->device));
    return render_field(c, fn, frame, view, d_lut, volume, reinterpret_cast<float4*>(d_rgba), d_values, d_summary, d_bins, (hipStream_t)hip_stream);
}

int rto_render_field_host(rto_context* c, const rto_frame* frame, const rto_field_view* view, const uint32_t* lut, const int32_t* host_volume,
                          float* host_rgba, int32_t* host_values, rto_field_view_summary* host_summary, int64_t* host_bins) {
    if (!c) return RTO_E_INVALID;
    const char* fn = "rto_render_field_host";
    const int* volume = nullptr;
    int rc = field_check(c, fn, frame, view, lut, host_volume, host_rgba, &volume);
    if (rc != RTO_OK) return rc;
    RTO_HIP(c, hipSetDevice(c->device));
    HostStage H(c, frame, lut, host_rgba);
    int32_t* d_values = H.optional(host_values, H.pixels);
    rto_field_view_summary* d_summary = H.optional(host_summary, 1);
    int64_t* d_bins = H.optional(host_bins, 256);
    volume = H.volume(host_volume, volume);
    if ((rc = H.status()) != RTO_OK) return rc;
    if ((rc = render_field(c, fn, frame, view, H.d_lut, volume, H.d_rgba, d_values, d_summary, d_bins, c->stream)) != RTO_OK) return rc;
    return H.finish();
}

int rto_last_field_view_ms(const rto_context* c, float ms[2]) { return c && ms ? c->fvEv.read(ms) : RTO_E_INVALID; }

}  // extern "C"
