// rto_project.inc -- field projections (include/rto_hip.h, rto_project_field_*): per pixel a reduction (maximum, minimum, mean,
// count, first) of an int32 volume of the resident grid over the voxels the pixel ray crosses, coloured as a field view is.
// Included at the end of rto_api.hip, after rto_field_view.inc (FieldSumRaw and its summary block, ShadeArgs, k_field_shade,
// field_view_volume, field_reserve) and rto_lit.inc (tile_pixel, frame_bound_check).
//
// Rule (DESIGN.md section 28).  The planes of a moving axis a are P(j) = gridMin[a] + (float)j * voxelSize, j = 0 .. dim[a], met at
// T(j) = (P(j) - o[a]) * inv[a]; the events are the planes with T > 0 in (T, axis) order, one axis' equal T in its direction of
// travel; the walk is the start state and the state after every event; the visited voxels are the states inside the box.  Floats
// decide that set and nothing else.  The kernel never sorts: T is monotone along an axis, so the walk is a merge of three sorted
// sequences, a state is found by rank (how many planes of an axis are ordered before a key) and a brick is left by its smallest
// leaving plane.
//
// Kernels (one stream, no host step):
//   k_project_bricks  one wave per run of 8 bricks along x: lane l reads column x = 64 run + l of the run's 8 x 8 (y, z) rows (256
//                     bytes a load, the volume once), keeps the largest key and the largest ~key of its valued voxels, and groups
//                     of 8 lanes fold them (lane_xor) into one 8-byte record per brick; 0 = no valued voxel.
//   k_project_march   one lane per pixel, 8x8 tiles per wave, no LDS: entry by rank, then one trip per voxel (a 4-byte gather) or
//                     per skipped brick; the summary as k_field_sample leaves it.
//   k_field_shade     unchanged.

namespace rto {

constexpr unsigned kProjectStill = 0x7fffffffu;      // the "next event" of an axis that has none: above the bits of every T > 0

struct ProjectArgs {
    const int* volume;       // dimZ x dimY x dimX, x fastest
    int dimX, dimY, dimZ;
    int loX, loY, loZ, hiX, hiY, hiZ;     // the box [lo, hi): the clip box or the grid
    int nbx, nby;            // bricks along x and y
    int validLo, validHi;
    int useTable;            // 0: rto_debug_set_projection_table(ctx, 0), no brick is skipped
    int totals;              // sums or counts were asked for: only bricks without a valued voxel are skipped, FIRST walks on
    const uint2* bricks;     // (largest key, largest ~key) per brick
    int* values;             // the caller's d_values or the context's buffer
    int* voxels;             // may be null
    long long* sums;         // may be null
    int* counts;             // may be null
    FieldSumRaw* sum;
};

__global__ __launch_bounds__(kBlock) void k_project_bricks(const int* __restrict__ volume, int dimX, int dimY, int dimZ, int nbx, int nby,
                                                           int runsX, unsigned waves, int validLo, int validHi, uint2* __restrict__ bricks) {
    const unsigned w = blockIdx.x * (unsigned)(kBlock / kWave) + (threadIdx.x >> 6);      // wave-uniform
    if (w >= waves) return;
    const int lane = threadIdx.x & 63;
    const int rx = (int)(w % (unsigned)runsX);
    const unsigned row = w / (unsigned)runsX;
    const int by = (int)(row % (unsigned)nby), bz = (int)(row / (unsigned)nby);
    const int x = rx * 64 + lane;
    const int y1 = min(by * 8 + 8, dimY), z1 = min(bz * 8 + 8, dimZ);
    unsigned kMax = 0u, kInv = 0u;
    if (x < dimX) {
        const int outside = validLo - 1;                 // representable (valid_lo > INT32_MIN + 1) and not valued
        for (int z = bz * 8; z < z1; z++) {
            const int* row = volume + ((size_t)z * (size_t)dimY + (size_t)(by * 8)) * (size_t)dimX + (size_t)x;
            int v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = by * 8 + k < y1 ? row[(size_t)k * (size_t)dimX] : outside;   // eight loads in flight
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const bool valued = v[k] >= validLo && v[k] <= validHi;
                const unsigned key = (unsigned)v[k] ^ 0x80000000u;
                kMax = valued && key > kMax ? key : kMax;
                kInv = valued && ~key > kInv ? ~key : kInv;
            }
        }
    }
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) {              // the 8 lanes of a brick
        const unsigned a = lane_xor(kMax, off), b = lane_xor(kInv, off);
        kMax = a > kMax ? a : kMax;
        kInv = b > kInv ? b : kInv;
    }
    const int bx = rx * 8 + (lane >> 3);
    if ((lane & 7) == 0 && bx < nbx) bricks[((size_t)bz * (size_t)nby + (size_t)by) * (size_t)nbx + (size_t)bx] = make_uint2(kMax, kInv);
}

// One axis of a pixel's walk.  A moving axis at coordinate c meets plane c + up next, at `next` (the bits of its T, which is
// positive: unsigned order is float order); a still axis never moves and holds kProjectStill.
struct ProjectAxis {
    float o, inv, g;
    int dim, lo, hi;
    int c, up, step;
    unsigned next;
    bool moving;
};

// T of plane j: one convert, multiply, add, subtract, multiply
__device__ __forceinline__ float project_t(const ProjectAxis& A, float vs, int j) { return ((A.g + (float)j * vs) - A.o) * A.inv; }

__device__ __forceinline__ void project_arm(ProjectAxis& A, float vs) {
    A.next = A.moving ? __float_as_uint(project_t(A, vs, A.c + A.up)) : kProjectStill;
}

__device__ __forceinline__ void project_step(ProjectAxis& A, float vs) {
    A.c += A.step;
    project_arm(A, vs);
}

// How many planes of a moving axis, in its direction of travel, come before the key: T <= t when incl, else T < t.  T is
// monotone in that direction, so the count is a binary search.
__device__ __forceinline__ int project_rank(const ProjectAxis& A, float vs, float t, bool incl) {
    int a = 0, b = A.dim + 1;
    while (a < b) {
        const int mid = (a + b) >> 1;
        const float tm = project_t(A, vs, A.up ? mid : A.dim - mid);
        if (incl ? tm <= t : tm < t) a = mid + 1; else b = mid;
    }
    return a;
}

// The axis before the walk: what it is, the T of the planes that bring it into the box and out of it, and whether it can be
// inside at all (a still axis: its one coordinate; a moving one: the leaving plane still ahead).
__device__ __forceinline__ bool project_axis_init(ProjectAxis& A, float vs, float o, float inv, float g, int dim, int lo, int hi,
                                                  float& tIn, float& tOut, bool& needIn) {
    A.o = o; A.inv = inv; A.g = g; A.dim = dim; A.lo = lo; A.hi = hi;
    A.moving = __builtin_isfinite(inv);
    A.up = inv > 0.0f ? 1 : 0;
    A.step = A.moving ? (A.up ? 1 : -1) : 0;
    A.c = 0; A.next = kProjectStill;
    tIn = tOut = 0.0f; needIn = false;
    if (!A.moving) {
        const float q = __builtin_floorf((o - g) / vs);
        const bool in = q >= (float)lo && q < (float)hi;
        if (in) A.c = (int)q;
        return in;
    }
    tIn = project_t(A, vs, A.up ? lo : hi);
    tOut = project_t(A, vs, A.up ? hi : lo);
    needIn = tIn > 0.0f;
    return tOut > 0.0f;
}

__device__ __forceinline__ bool project_inside(const ProjectAxis& A) { return A.c >= A.lo && A.c < A.hi; }

// The plane through which a moving axis leaves its brick, and the coordinate behind it.
__device__ __forceinline__ int project_brick_exit(const ProjectAxis& A) {
    const int b = A.c >> 3;
    return A.up ? min(b * 8 + 8, A.dim) : b * 8;
}

// Axis B, which is not the axis of the key (t, B before the key's axis when `first`), crosses every plane ordered before the key.
// Inside a brick that is at most 7 planes.
__device__ __forceinline__ void project_catch_up(ProjectAxis& B, float vs, unsigned t, bool first) {
    for (int i = 0; i < 8 && (B.next < t || (first && B.next == t)); i++) project_step(B, vs);
}

template <int OP>
__global__ __launch_bounds__(kBlock) void k_project_march(RenderParams P, ProjectArgs A) {
    const Geo G = geo_of(P);
    const int lane = threadIdx.x & 63;
    const TilePixel t = tile_pixel(P);
    const Ray r = t.r;
    const bool inFrame = t.in;

    ProjectAxis X, Y, Z;
    float inX, inY, inZ, outX, outY, outZ;
    bool needX, needY, needZ;
    bool alive = inFrame && __builtin_isfinite(r.ox) && __builtin_isfinite(r.oy) && __builtin_isfinite(r.oz);
    const bool okX = project_axis_init(X, G.vs, r.ox, r.ix, G.gx, A.dimX, A.loX, A.hiX, inX, outX, needX);
    const bool okY = project_axis_init(Y, G.vs, r.oy, r.iy, G.gy, A.dimY, A.loY, A.hiY, inY, outY, needY);
    const bool okZ = project_axis_init(Z, G.vs, r.oz, r.iz, G.gz, A.dimZ, A.loZ, A.hiZ, inZ, outZ, needZ);
    alive = alive && okX && okY && okZ && (X.moving || Y.moving || Z.moving);
    // the entry: the largest entering event in (T, axis) order (axis 3, T 0: none, the walk starts inside); it must come before
    // every other axis' leaving event
    float eT = 0.0f;
    int eAxis = 3;
    if (needX) { eT = inX; eAxis = 0; }
    if (needY && (eAxis == 3 || inY >= eT)) { eT = inY; eAxis = 1; }
    if (needZ && (eAxis == 3 || inZ >= eT)) { eT = inZ; eAxis = 2; }
    if (eAxis != 3) {
        if (X.moving && eAxis != 0) alive = alive && eT < outX;                       // x comes before the entry's axis on a tie
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
    const bool visited = alive;                       // the pixel is no miss

    unsigned runMax = 0u, runInv = 0u;                // keys of the running extremes (count == 0: none yet)
    long long sum = 0;
    int count = 0, firstVox = -1, maxVox = -1, minVox = -1, firstVal = 0;
    int lastBrick = -1;
    bool skip = false;
    int budget = A.dimX + A.dimY + A.dimZ + 4;        // no walk has more states: a loop that cannot hang whatever the floats do
    while (alive) {
        const int brick = ((Z.c >> 3) * A.nby + (Y.c >> 3)) * A.nbx + (X.c >> 3);
        if (brick != lastBrick) {
            lastBrick = brick;
            skip = false;
            if (A.useTable) {
                const uint2 k = A.bricks[brick];
                if (A.totals || OP == RTO_PROJECT_MEAN || OP == RTO_PROJECT_COUNT || OP == RTO_PROJECT_FIRST) skip = k.x == 0u;
                else if (OP == RTO_PROJECT_MAX) skip = k.x <= runMax;      // <=: the deciding voxel is the first to hold the value
                else skip = k.x == 0u || (count > 0 && k.y <= runInv);        // ~key 0 is a value (INT32_MAX): k.x says "none"
            }
        }
        if (skip) {
            // the brick's exit event: the smallest (T, axis) among its leaving planes; the other axes cross what comes before it
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
            const int idx = (Z.c * A.dimY + Y.c) * A.dimX + X.c;        // < 2^31 (project_check)
            const int v = A.volume[idx];
            bool done = false;
            if (v >= A.validLo && v <= A.validHi) {
                const unsigned key = (unsigned)v ^ 0x80000000u;
                if (count == 0) { firstVox = maxVox = minVox = idx; firstVal = v; runMax = key; runInv = ~key; }   // ~key may be 0: INT32_MAX
                count++;
                sum += (long long)v;
                if (key > runMax) { runMax = key; maxVox = idx; }
                if (~key > runInv) { runInv = ~key; minVox = idx; }
                done = OP == RTO_PROJECT_FIRST && !A.totals;
            }
            if (done) break;
            if (X.next <= Y.next && X.next <= Z.next) project_step(X, G.vs);
            else if (Y.next <= Z.next) project_step(Y, G.vs);
            else project_step(Z, G.vs);
        }
        alive = project_inside(X) && project_inside(Y) && project_inside(Z) && --budget > 0;
    }

    int value = kFieldMiss, voxel = -1;
    if (visited) {
        value = kFieldNone;
        if (count > 0) {
            voxel = firstVox;
            if (OP == RTO_PROJECT_MAX) { value = (int)(runMax ^ 0x80000000u); voxel = maxVox; }
            else if (OP == RTO_PROJECT_MIN) { value = (int)(~runInv ^ 0x80000000u); voxel = minVox; }
            else if (OP == RTO_PROJECT_MEAN) {
                long long q = sum / (long long)count;
                if (sum % (long long)count != 0 && sum < 0) q--;        // floor towards minus infinity
                value = (int)q;
            }
            else if (OP == RTO_PROJECT_COUNT) value = count;
            else value = firstVal;
        }
    }
    if (inFrame) {
        const unsigned pix = (unsigned)t.py * (unsigned)P.W + (unsigned)t.px;   // < 2^32 (frame_bound_check)
        A.values[pix] = value;
        if (A.voxels) A.voxels[pix] = voxel;
        if (A.sums) A.sums[pix] = sum;
        if (A.counts) A.counts[pix] = count;
    }
    // the frame's summary, as k_field_sample leaves it
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

}  // namespace rto

// ---------------------------------------------------------------- host side
static_assert(sizeof(rto_field_projection) == 112, "the ABI's size");

// Every check of a projection, in the order the ABI promises; *volume: the int32 volume the frame reduces.
static int project_check(rto_context* c, const char* fn, const rto_frame* f, const rto_field_projection* v, const void* lut,
                         const int32_t* d_volume, const void* rgba, const int** volume) {
    const std::string name(fn);
    if (!f || !v || !lut || !rgba) return fail(c, RTO_E_INVALID, name + ": NULL frame, projection, LUT or output");
    if (v->source < RTO_FIELD_DISTANCE || v->source > RTO_FIELD_CALLER) return fail(c, RTO_E_INVALID, name + ": unknown source " + std::to_string(v->source));
    if (v->op < RTO_PROJECT_MAX || v->op > RTO_PROJECT_FIRST) return fail(c, RTO_E_INVALID, name + ": unknown op " + std::to_string(v->op));
    if (v->scale < RTO_SCALE_LINEAR || v->scale > RTO_SCALE_CATEGORY) return fail(c, RTO_E_INVALID, name + ": unknown scale " + std::to_string(v->scale));
    for (int r : v->reserved) if (r != 0) return fail(c, RTO_E_INVALID, name + ": projection.reserved must be 0");
    if (v->valid_lo > v->valid_hi || v->valid_lo <= RTO_FIELD_PIXEL_NONE)
        return fail(c, RTO_E_INVALID, name + ": valid_lo must be above INT32_MIN + 1 and at most valid_hi");
    if (v->range_lo > v->range_hi) return fail(c, RTO_E_INVALID, name + ": range_lo > range_hi");
    int rc = frame_bound_check(c, name, f, 1);
    if (rc != RTO_OK) return rc;
    if (v->source == RTO_FIELD_CALLER && !d_volume) return fail(c, RTO_E_INVALID, name + ": RTO_FIELD_CALLER needs a volume");
    if (v->source != RTO_FIELD_CALLER && d_volume) return fail(c, RTO_E_INVALID, name + ": a volume goes with RTO_FIELD_CALLER only");
    if (c->numNodes <= 0) return fail(c, RTO_E_NO_OCTREE, name + ": no octree uploaded");
    if (!c->d_vox) return fail(c, RTO_E_UNSUPPORTED, name + ": the octree came from rto_upload_octree: no voxel grid is resident");
    if (grid_voxels(c) > 0x7fffffffll) return fail(c, RTO_E_UNSUPPORTED, name + ": the grid has 2^31 voxels or more: a voxel's index does not fit d_voxels");
    if (v->clip)
        for (int a = 0; a < 3; a++)
            if (v->clip_lo[a] < 0 || v->clip_hi[a] > c->voxDim[a] || v->clip_lo[a] >= v->clip_hi[a])
                return fail(c, RTO_E_INVALID, name + ": the clip box needs 0 <= clip_lo < clip_hi <= dim on every axis");
    return field_view_volume(c, fn, v->source, d_volume, volume);
}

// The brick table, kept on the context under the field views' rules for work buffers: it grows with the grid, and a call that
// grows it must not be stream-captured.
static int project_reserve(rto_context* c, const char* fn, size_t bricks, hipStream_t s) {
    if (c->pjBrickCap >= bricks && c->pjEv[0]) return RTO_OK;
    if (stream_is_capturing(s))
        return fail(c, RTO_E_UNSUPPORTED, std::string(fn) + ": a larger grid allocates the brick table; project one frame of it "
                                          "before hipStreamBeginCapture");
    if (!c->pjEv[0]) for (hipEvent_t& e : c->pjEv) RTO_HIP(c, hipEventCreate(&e));
    if (c->pjBrickCap < bricks) {
        (void)hipFree(c->d_pjBricks); c->d_pjBricks = nullptr;       // hipFree waits for the device: no frame still reads it
        c->pjBrickCap = 0;
        RTO_HIP(c, hipMalloc(&c->d_pjBricks, bricks * sizeof(uint2)));
        c->pjBrickCap = bricks;
    }
    return RTO_OK;
}

template <int OP>
static void project_launch(dim3 grid, hipStream_t s, const RenderParams& P, const ProjectArgs& A) {
    hipLaunchKernelGGL(k_project_march<OP>, grid, dim3(kBlock), 0, s, P, A);
}

static int project_field(rto_context* c, const char* fn, const rto_frame* f, const rto_field_projection* v, const unsigned* d_lut, const int* volume,
                         float4* d_rgba, int32_t* d_values, int32_t* d_voxels, int64_t* d_sums, int32_t* d_counts,
                         rto_field_view_summary* d_summary, int64_t* d_bins, hipStream_t s) {
    RenderParams P;
    int rc = fill_params(c, f, nullptr, P, s);
    if (rc != RTO_OK) return rc;
    const size_t pixels = (size_t)P.W * (size_t)P.H;
    if ((rc = field_reserve(c, fn, pixels, d_values == nullptr, s)) != RTO_OK) return rc;
    const int nbx = (c->voxDim[0] + 7) / 8, nby = (c->voxDim[1] + 7) / 8, nbz = (c->voxDim[2] + 7) / 8;
    if ((rc = project_reserve(c, fn, (size_t)nbx * (size_t)nby * (size_t)nbz, s)) != RTO_OK) return rc;
    ProjectArgs A;
    A.volume = volume;
    A.dimX = c->voxDim[0]; A.dimY = c->voxDim[1]; A.dimZ = c->voxDim[2];
    A.loX = v->clip ? v->clip_lo[0] : 0; A.loY = v->clip ? v->clip_lo[1] : 0; A.loZ = v->clip ? v->clip_lo[2] : 0;
    A.hiX = v->clip ? v->clip_hi[0] : A.dimX; A.hiY = v->clip ? v->clip_hi[1] : A.dimY; A.hiZ = v->clip ? v->clip_hi[2] : A.dimZ;
    A.nbx = nbx; A.nby = nby;
    A.validLo = v->valid_lo; A.validHi = v->valid_hi;
    A.useTable = c->pjTable ? 1 : 0;
    A.totals = (d_sums || d_counts) ? 1 : 0;
    A.bricks = c->d_pjBricks;
    A.values = d_values ? d_values : c->d_fvValues;
    A.voxels = d_voxels; A.sums = reinterpret_cast<long long*>(d_sums); A.counts = d_counts;
    A.sum = reinterpret_cast<FieldSumRaw*>(c->d_fvSum);
    ShadeArgs S;
    S.values = A.values; S.lut = d_lut; S.rgba = d_rgba; S.sum = A.sum; S.outSum = d_summary;
    S.bins = reinterpret_cast<unsigned long long*>(d_bins);
    S.pixels = (unsigned)pixels;
    S.scale = v->scale; S.shade = 0;
    S.rangeLo = v->range_lo; S.rangeHi = v->range_hi;
    std::memcpy(S.miss, v->miss_rgba, sizeof S.miss);
    std::memcpy(S.none, v->none_rgba, sizeof S.none);

    const bool timed = !(stream_is_capturing(s) || c->eventsOff);
    RTO_HIP(c, hipMemsetAsync(c->d_fvSum, 0, kFieldSlots * sizeof(FieldSumRaw), s));
    if (d_bins) RTO_HIP(c, hipMemsetAsync(d_bins, 0, 256 * sizeof(int64_t), s));
    if (timed) RTO_HIP(c, hipEventRecord(c->pjEv[0], s));
    if (A.useTable) {
        const int runsX = (nbx + 7) / 8;
        const int64_t waves = (int64_t)runsX * nby * nbz;             // < 2^31 / 512 + ...: the grid has fewer than 2^31 voxels
        const dim3 grid((unsigned)((waves + kBlock / kWave - 1) / (kBlock / kWave)));
        hipLaunchKernelGGL(k_project_bricks, grid, dim3(kBlock), 0, s, volume, A.dimX, A.dimY, A.dimZ, nbx, nby, runsX, (unsigned)waves,
                           A.validLo, A.validHi, c->d_pjBricks);
        RTO_HIP(c, hipGetLastError());
    }
    if (timed) RTO_HIP(c, hipEventRecord(c->pjEv[1], s));
    const int64_t tiles = (int64_t)P.tilesX * P.tilesY;
    const dim3 grid((unsigned)((tiles + kBlock / kWave - 1) / (kBlock / kWave)));
    switch (v->op) {
        case RTO_PROJECT_MAX: project_launch<RTO_PROJECT_MAX>(grid, s, P, A); break;
        case RTO_PROJECT_MIN: project_launch<RTO_PROJECT_MIN>(grid, s, P, A); break;
        case RTO_PROJECT_MEAN: project_launch<RTO_PROJECT_MEAN>(grid, s, P, A); break;
        case RTO_PROJECT_COUNT: project_launch<RTO_PROJECT_COUNT>(grid, s, P, A); break;
        default: project_launch<RTO_PROJECT_FIRST>(grid, s, P, A); break;
    }
    RTO_HIP(c, hipGetLastError());
    if (timed) RTO_HIP(c, hipEventRecord(c->pjEv[2], s));
    const int64_t blocks = std::min<int64_t>((int64_t)c->numCUs * 8, ((int64_t)pixels + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_field_shade, dim3((unsigned)blocks), dim3(kBlock), 0, s, S);
    RTO_HIP(c, hipGetLastError());
    if (timed) RTO_HIP(c, hipEventRecord(c->pjEv[3], s));
    c->pjTimed = timed;
    return RTO_OK;
}

extern "C" {

int rto_project_field_device(rto_context* c, const rto_frame* frame, const rto_field_projection* proj, const uint32_t* d_lut,
                             const int32_t* d_volume, void* d_rgba, int32_t* d_values, int32_t* d_voxels, int64_t* d_sums, int32_t* d_counts,
                             rto_field_view_summary* d_summary, int64_t* d_bins, void* hip_stream) {
    if (!c) return RTO_E_INVALID;
    const char* fn = "rto_project_field_device";
    auto off = [](const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
    if (frame && proj && d_lut && d_rgba &&
        (off(d_rgba, 15) || off(d_lut, 3) || off(d_volume, 3) || off(d_values, 3) || off(d_voxels, 3) || off(d_counts, 3) || off(d_sums, 7) ||
         off(d_summary, 7) || off(d_bins, 7)))
        return fail(c, RTO_E_INVALID, std::string(fn) + ": d_rgba must be 16-byte, d_sums, d_summary and d_bins 8-byte, d_lut, d_volume, d_values, "
                                      "d_voxels and d_counts 4-byte aligned");
    const int* volume = nullptr;
    const int rc = project_check(c, fn, frame, proj, d_lut, d_volume, d_rgba, &volume);
    if (rc != RTO_OK) return rc;
    RTO_HIP(c, hipSetDevice(c->device));
    return project_field(c, fn, frame, proj, d_lut, volume, reinterpret_cast<float4*>(d_rgba), d_values, d_voxels, d_sums, d_counts, d_summary,
                         d_bins, (hipStream_t)hip_stream);
}

int rto_project_field_host(rto_context* c, const rto_frame* frame, const rto_field_projection* proj, const uint32_t* lut,
                           const int32_t* host_volume, float* host_rgba, int32_t* host_values, int32_t* host_voxels, int64_t* host_sums,
                           int32_t* host_counts, rto_field_view_summary* host_summary, int64_t* host_bins) {
    if (!c) return RTO_E_INVALID;
    const char* fn = "rto_project_field_host";
    const int* volume = nullptr;
    int rc = project_check(c, fn, frame, proj, lut, host_volume, host_rgba, &volume);
    if (rc != RTO_OK) return rc;
    RTO_HIP(c, hipSetDevice(c->device));
    const size_t pixels = (size_t)frame->width * (size_t)frame->height;
    BuildScratch scratch(c->stream);
    float4* d_rgba = nullptr;
    int32_t *d_values = nullptr, *d_voxels = nullptr, *d_counts = nullptr;
    int64_t *d_sums = nullptr, *d_bins = nullptr;
    unsigned* d_lut = nullptr;
    rto_field_view_summary* d_summary = nullptr;
    RTO_HIP(c, scratch.alloc(&d_rgba, pixels));
    RTO_HIP(c, scratch.alloc(&d_lut, 256));
    if (host_values) RTO_HIP(c, scratch.alloc(&d_values, pixels));
    if (host_voxels) RTO_HIP(c, scratch.alloc(&d_voxels, pixels));
    if (host_sums) RTO_HIP(c, scratch.alloc(&d_sums, pixels));
    if (host_counts) RTO_HIP(c, scratch.alloc(&d_counts, pixels));
    if (host_summary) RTO_HIP(c, scratch.alloc(&d_summary, 1));
    if (host_bins) RTO_HIP(c, scratch.alloc(&d_bins, 256));
    RTO_HIP(c, hipMemcpyAsync(d_lut, lut, 256 * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    if (host_volume) {                                               // RTO_FIELD_CALLER (project_check)
        int32_t* d_volume = nullptr;
        RTO_HIP(c, scratch.alloc(&d_volume, (size_t)grid_voxels(c)));
        RTO_HIP(c, hipMemcpyAsync(d_volume, host_volume, (size_t)grid_voxels(c) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        volume = d_volume;
    }
    if ((rc = project_field(c, fn, frame, proj, d_lut, volume, d_rgba, d_values, d_voxels, d_sums, d_counts, d_summary, d_bins, c->stream)) != RTO_OK)
        return rc;
    RTO_HIP(c, hipMemcpyAsync(host_rgba, d_rgba, pixels * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    if (host_values) RTO_HIP(c, hipMemcpyAsync(host_values, d_values, pixels * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (host_voxels) RTO_HIP(c, hipMemcpyAsync(host_voxels, d_voxels, pixels * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (host_sums) RTO_HIP(c, hipMemcpyAsync(host_sums, d_sums, pixels * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    if (host_counts) RTO_HIP(c, hipMemcpyAsync(host_counts, d_counts, pixels * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (host_summary) RTO_HIP(c, hipMemcpyAsync(host_summary, d_summary, sizeof *host_summary, hipMemcpyDeviceToHost, c->stream));
    if (host_bins) RTO_HIP(c, hipMemcpyAsync(host_bins, d_bins, 256 * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    RTO_HIP(c, hipStreamSynchronize(c->stream));
    return RTO_OK;
}

int rto_last_projection_ms(const rto_context* c, float ms[3]) {
    if (!c || !ms) return RTO_E_INVALID;
    ms[0] = ms[1] = ms[2] = -1.0f;
    if (!c->pjTimed) return RTO_OK;
    if (hipEventSynchronize(c->pjEv[3]) != hipSuccess) return RTO_E_HIP;
    for (int k = 0; k < 3; k++)
        if (hipEventElapsedTime(&ms[k], c->pjEv[k], c->pjEv[k + 1]) != hipSuccess) {
            ms[0] = ms[1] = ms[2] = -1.0f;
            return RTO_E_HIP;
        }
    return RTO_OK;
}

int rto_debug_set_projection_table(rto_context* c, int enabled) {
    if (!c) return RTO_E_INVALID;
    c->pjTable = enabled != 0;
    return RTO_OK;
}

}  // extern "C"
