// rto_project.inc -- field projections (include/rto_hip.h, rto_project_field_*): per pixel a reduction (maximum, minimum, mean,
// count, first) of an int32 volume of the resident grid over the voxels the pixel ray crosses, coloured as a field view is.
// Included at the end of rto_api.hip, after rto_voxel_walk.inc (the rule of DESIGN.md section 28: WalkBox, VoxelWalk, k_project_bricks,
// walk_box, walk_bricks_launch), rto_field_view.inc (FieldSumRaw and its summary block, ShadeArgs, k_field_shade, field_reserve, and
// the host pieces of every field frame: field_frame_check, HostStage, misaligned) and rto_lit.inc (tile_pixel, frame_bound_check).
//
// Kernels (one stream, no host step):
//   k_project_bricks  rto_voxel_walk.inc: the largest and smallest valued value of every brick.
//   k_project_march   one lane per pixel, 8x8 tiles per wave, no LDS: the walk's entry by rank, then one trip per voxel (a 4-byte
//                     gather) or per skipped brick; the summary as k_field_sample leaves it.
//   k_field_shade     unchanged.

namespace rto {

struct ProjectArgs {
    WalkBox box;
    int totals;              // sums or counts were asked for: only bricks without a valued voxel are skipped, FIRST walks on
    int* values;             // the caller's d_values or the context's buffer
    int* voxels;             // may be null
    long long* sums;         // may be null
    int* counts;             // may be null
    FieldSumRaw* sum;
};

template <int OP>
__global__ __launch_bounds__(kBlock) void k_project_march(RenderParams P, ProjectArgs A) {
    const Geo G = geo_of(P);
    const int lane = threadIdx.x & 63;
    const TilePixel t = tile_pixel(P);
    const bool inFrame = t.in;

    VoxelWalk W;
    const bool visited = W.enter(G, t.r, inFrame, A.box);       // the pixel is no miss
    bool alive = visited;

    unsigned runMax = 0u, runInv = 0u;                // keys of the running extremes (count == 0: none yet)
    long long sum = 0;
    int count = 0, firstVox = -1, maxVox = -1, minVox = -1, firstVal = 0;
    int lastBrick = -1;
    bool skip = false;
    while (alive) {
        const int brick = W.brick();
        if (brick != lastBrick) {
            lastBrick = brick;
            skip = false;
            if (A.box.useTable) {
                const uint2 k = A.box.bricks[brick];
                if (A.totals || OP == RTO_PROJECT_MEAN || OP == RTO_PROJECT_COUNT || OP == RTO_PROJECT_FIRST) skip = k.x == 0u;
                else if (OP == RTO_PROJECT_MAX) skip = k.x <= runMax;      // <=: the deciding voxel is the first to hold the value
                else skip = k.x == 0u || (count > 0 && k.y <= runInv);        // ~key 0 is a value (INT32_MAX): k.x says "none"
            }
        }
        if (skip) {
            W.leave_brick(G.vs);
        } else {
            const int idx = W.voxel();
            const int v = A.box.volume[idx];
            bool done = false;
            if (v >= A.box.validLo && v <= A.box.validHi) {
                const unsigned key = (unsigned)v ^ 0x80000000u;
                if (count == 0) { firstVox = maxVox = minVox = idx; firstVal = v; runMax = key; runInv = ~key; }   // ~key may be 0: INT32_MAX
                count++;
                sum += (long long)v;
                if (key > runMax) { runMax = key; maxVox = idx; }
                if (~key > runInv) { runInv = ~key; minVox = idx; }
                done = OP == RTO_PROJECT_FIRST && !A.totals;
            }
            if (done) break;
            W.step(G.vs);
        }
        alive = W.advance();
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
    return field_frame_check(c, name, "projection", f, v, lut, d_volume, rgba, volume,
        [&] { return v->op < RTO_PROJECT_MAX || v->op > RTO_PROJECT_FIRST ? fail(c, RTO_E_INVALID, name + ": unknown op " + std::to_string(v->op)) : RTO_OK; },
        [&] { return check_range_order(c, name, v->range_lo, v->range_hi); },
        [&] { return check_grid_index(c, name, "d_voxels"); });
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
    ProjectArgs A;
    if ((rc = walk_box(c, fn, v, volume, s, A.box)) != RTO_OK) return rc;
    A.totals = (d_sums || d_counts) ? 1 : 0;
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
    RTO_HIP(c, c->pjEv.mark(0, s, timed));
    if (A.box.useTable) RTO_HIP(c, walk_bricks_launch(c, A.box, s));
    RTO_HIP(c, c->pjEv.mark(1, s, timed));
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
    RTO_HIP(c, c->pjEv.mark(2, s, timed));
    const int64_t blocks = std::min<int64_t>((int64_t)c->numCUs * 8, ((int64_t)pixels + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_field_shade, dim3((unsigned)blocks), dim3(kBlock), 0, s, S);
    RTO_HIP(c, hipGetLastError());
    RTO_HIP(c, c->pjEv.mark(3, s, timed));
    return RTO_OK;
}

extern "C" {

int rto_project_field_device(rto_context* c, const rto_frame* frame, const rto_field_projection* proj, const uint32_t* d_lut,
                             const int32_t* d_volume, void* d_rgba, int32_t* d_values, int32_t* d_voxels, int64_t* d_sums, int32_t* d_counts,
                             rto_field_view_summary* d_summary, int64_t* d_bins, void* hip_stream) {
    if (!c) return RTO_E_INVALID;
    const char* fn = "rto_project_field_device";
    if (frame && proj && d_lut && d_rgba &&
        (misaligned(d_rgba, 15) || misaligned(d_lut, 3) || misaligned(d_volume, 3) || misaligned(d_values, 3) || misaligned(d_voxels, 3) ||
         misaligned(d_counts, 3) || misaligned(d_sums, 7) || misaligned(d_summary, 7) || misaligned(d_bins, 7)))
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
    HostStage H(c, frame, lut, host_rgba);
    int32_t* d_values = H.optional(host_values, H.pixels);
    int32_t* d_voxels = H.optional(host_voxels, H.pixels);
    int64_t* d_sums = H.optional(host_sums, H.pixels);
    int32_t* d_counts = H.optional(host_counts, H.pixels);
    rto_field_view_summary* d_summary = H.optional(host_summary, 1);
    int64_t* d_bins = H.optional(host_bins, 256);
    volume = H.volume(host_volume, volume);
    if ((rc = H.status()) != RTO_OK) return rc;
    if ((rc = project_field(c, fn, frame, proj, H.d_lut, volume, H.d_rgba, d_values, d_voxels, d_sums, d_counts, d_summary, d_bins, c->stream)) != RTO_OK)
        return rc;
    return H.finish();
}

int rto_last_projection_ms(const rto_context* c, float ms[3]) { return c && ms ? c->pjEv.read(ms) : RTO_E_INVALID; }

int rto_debug_set_projection_table(rto_context* c, int enabled) {
    if (!c) return RTO_E_INVALID;
    c->pjTable = enabled != 0;
    return RTO_OK;
}

}  // extern "C"
