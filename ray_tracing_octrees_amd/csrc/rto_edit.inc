// rto_edit.inc -- voxel edits (include/rto_hip.h, rto_edit_voxels): sphere and box brushes carve (-> EMPTY) or fill (-> FILLED)
// the grid rto_build_octree keeps in HBM, then the octree (and the leaf triangles, when they were resident) is rebuilt from that
// grid with no host copy.  Included at the end of rto_api.hip.
//
// Coverage rule (DESIGN.md section 11), exact in integers at 1/64 voxel.  On the host, in double: cq = floor((centre - gridMin) /
// voxelSize * 64 + 0.5), eq = floor(extent / voxelSize * 64 + 0.5), |cq|, eq <= 2^27.  Voxel i (cell [i, i+1), centre i + 1/2) has
// D[a] = 64 (2 i[a] + 1) - 2 cq[a]; a sphere covers it when D0^2 + D1^2 + D2^2 <= (2 eq0)^2, a box when |D[a]| <= 2 eq[a] on every
// axis.  Brushes apply in array order (the later one wins); changed = voxels whose final value differs from the value before.

namespace rto {

// One quantised brush.  lo / hi: the voxels its clipped bounding box holds, inclusive (lo > hi on some axis: it touches nothing).
// For a box that bounding box IS the covered set; a sphere tests each voxel inside it.
struct EditBrush {
    long long cq[3];
    long long r2;            // sphere: (2 eq0)^2
    int lo[3], hi[3];
    int shape, op;
};
constexpr int kEditRun = 16;                         // voxels per thread: one 16-byte row chunk, x-aligned
constexpr int kEditRunsX = 16, kEditRowsY = 16;      // a 256-thread block: 16 runs along x by 16 rows along y, one z slice

// The union of the brushes' boxes, half-open: [xlo, x1) x [y0, y1) x [z0, z1); the runs start at x0 = xlo rounded down to 16.
struct EditBox { int x0, xlo, y0, z0, x1, y1, z1; int runsX, blocksX, blocksY; };

// One launch over the union box.  Each thread owns one x-aligned run of 16 voxels of one row and scans the brushes from the last
// back: the first brush that covers a voxel decides it, voxels no brush covers keep their value.  Rows of a grid with dimX % 16 ==
// 0 are read and written 16 bytes at a time (WIDE: the box rounded out to 16-byte chunks, bytes outside it written back as
// they were, and only runs with a change are written); other grids read and write only bytes inside the box.  The changed count:
// block_add_count.
template <bool WIDE>
__global__ __launch_bounds__(kBlock) void k_edit_brushes(uint8_t* __restrict__ vox, int dimX, int dimY, const EditBrush* __restrict__ brushes,
                                                        int n, EditBox box, unsigned long long* __restrict__ changed) {
    const int t = (int)threadIdx.x;
    const int bid = (int)blockIdx.x;
    const int bx = bid % box.blocksX, by = (bid / box.blocksX) % box.blocksY, bz = bid / (box.blocksX * box.blocksY);
    const int run = bx * kEditRunsX + (t % kEditRunsX);
    const int y = box.y0 + by * kEditRowsY + t / kEditRunsX;
    const int z = box.z0 + bz;
    const int x0 = box.x0 + run * kEditRun;
    int count = 0;
    if (run < box.runsX && y < box.y1) {
        // voxels of this run inside the box (the box lies inside the grid)
        const int first = max(x0, box.xlo), last = min(x0 + kEditRun, box.x1) - 1;
        const unsigned need = last >= first ? ((1u << (last - first + 1)) - 1u) << (first - x0) : 0u;
        unsigned decided = 0u, fill = 0u;                          // bit j: voxel x0 + j is decided / its final value is FILLED
        for (int b = n - 1; b >= 0 && (decided & need) != need; b--) {
            const EditBrush& B = brushes[b];
            if (y < B.lo[1] || y > B.hi[1] || z < B.lo[2] || z > B.hi[2] || B.hi[0] < first || B.lo[0] > last) continue;
            unsigned cover = 0u;
            if (B.shape == RTO_BRUSH_BOX) {
                const int a = max(B.lo[0], first) - x0, e = min(B.hi[0], last) - x0;
                cover = ((1u << (e - a + 1)) - 1u) << a;
            } else {
                const long long dy = 64ll * (2 * y + 1) - 2 * B.cq[1], dz = 64ll * (2 * z + 1) - 2 * B.cq[2];
                const long long rem = B.r2 - (dy * dy + dz * dz);
#pragma unroll
                for (int j = 0; j < kEditRun; j++) {
                    const long long dx = 64ll * (2 * (x0 + j) + 1) - 2 * B.cq[0];
                    const bool in = x0 + j >= B.lo[0] && x0 + j <= B.hi[0] && dx * dx <= rem;
                    cover |= (in ? 1u : 0u) << j;
                }
            }
            cover &= need & ~decided;
            decided |= cover;
            if (B.op == RTO_EDIT_FILL) fill |= cover;
        }
        if (decided) {
            uint8_t* row = vox + ((size_t)z * dimY + y) * (size_t)dimX + x0;
            if (WIDE) {
                uint4 w = *reinterpret_cast<const uint4*>(row);
                unsigned words[4] = { w.x, w.y, w.z, w.w };
                unsigned diff = 0u;
#pragma unroll
                for (int j = 0; j < kEditRun; j++) {
                    const unsigned sh = 8u * (unsigned)(j & 3);
                    const unsigned old = (words[j >> 2] >> sh) & 0xffu;
                    const unsigned nv = (fill >> j) & 1u;
                    const bool d = ((decided >> j) & 1u) && old != nv;
                    diff |= (d ? 1u : 0u) << j;
                    words[j >> 2] = d ? ((words[j >> 2] & ~(0xffu << sh)) | (nv << sh)) : words[j >> 2];
                }
                if (diff) *reinterpret_cast<uint4*>(row) = make_uint4(words[0], words[1], words[2], words[3]);
                count = __popc(diff);
            } else {
#pragma unroll
                for (int j = 0; j < kEditRun; j++) {
                    if ((decided >> j) & 1u) {
                        const uint8_t nv = (uint8_t)((fill >> j) & 1u);
                        if (row[j] != nv) { row[j] = nv; count++; }
                    }
                }
            }
        }
    }
    block_add_count(count, changed);
}

}  // namespace rto

namespace {
inline long long floor_div64(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }   // b > 0

// The quantised form of one brush (rto_brush_quantize) and its clipped voxel box.
int quantize_brush(const rto_brush* b, const float grid_min[3], float voxel_size, long long cq[3], long long eq[3]) {
    if (!b || !grid_min) return RTO_E_INVALID;
    if (b->shape != RTO_BRUSH_SPHERE && b->shape != RTO_BRUSH_BOX) return RTO_E_INVALID;
    if (b->op != RTO_EDIT_CARVE && b->op != RTO_EDIT_FILL) return RTO_E_INVALID;
    const double vs = (double)voxel_size;
    if (!std::isfinite(vs) || !(vs > 0.0)) return RTO_E_INVALID;
    const double kLimit = 134217728.0;                                                   // 2^27 sixty-fourths = 2^21 voxels
    for (int a = 0; a < 3; a++) {
        const double c = (double)b->centre[a], g = (double)grid_min[a], e = (double)b->extent[a];
        if (!std::isfinite(c) || !std::isfinite(g) || !std::isfinite(e) || e < 0.0) return RTO_E_INVALID;
        const double rel = c - g;                  // one IEEE operation per statement: what tests/edit_ref.py computes
        const double vc = rel / vs;
        const double sc = vc * 64.0;
        const double fc = std::floor(sc + 0.5);
        const double ve = e / vs;
        const double se = ve * 64.0;
        const double fe = std::floor(se + 0.5);
        if (!(std::fabs(fc) <= kLimit) || !(fe <= kLimit)) return RTO_E_INVALID;
        cq[a] = (long long)fc; eq[a] = (long long)fe;
    }
    return RTO_OK;
}

// Voxels i with |64 (2 i + 1) - 2 cq| <= 2 eq, i.e. cq - eq - 32 <= 64 i <= cq + eq - 32, clipped to [0, dim - 1].
rto::EditBrush clip_brush(const rto_brush& b, const long long cq[3], const long long eq[3], const int dims[3]) {
    rto::EditBrush B;
    for (int a = 0; a < 3; a++) {
        B.cq[a] = cq[a];
        const long long e = b.shape == RTO_BRUSH_SPHERE ? eq[0] : eq[a];           // a sphere's radius bounds every axis
        const long long lo = -floor_div64(-(cq[a] - e - 32), 64), hi = floor_div64(cq[a] + e - 32, 64);
        B.lo[a] = (int)std::max<long long>(lo, 0);
        B.hi[a] = (int)std::min<long long>(hi, (long long)dims[a] - 1);
    }
    if (B.lo[0] > B.hi[0] || B.lo[1] > B.hi[1] || B.lo[2] > B.hi[2])      // outside the grid on some axis: empty on every axis, so
        for (int a = 0; a < 3; a++) { B.lo[a] = 1; B.hi[a] = 0; }          // that the kernel's row test (y, z) rejects it before x is looked at
    B.r2 = (2 * eq[0]) * (2 * eq[0]);
    B.shape = b.shape; B.op = b.op;
    return B;
}
}  // namespace

extern "C" {

int rto_brush_quantize(const rto_brush* b, const float grid_min[3], float voxel_size, int64_t cq[3], int64_t eq[3]) {
    long long q[3], e[3];
    const int rc = quantize_brush(b, grid_min, voxel_size, q, e);
    if (rc != RTO_OK) return rc;
    for (int a = 0; a < 3; a++) {
        if (cq) cq[a] = q[a];
        if (eq) eq[a] = e[a];
    }
    return RTO_OK;
}

int rto_edit_voxels(rto_context* c, const rto_brush* brushes, int n, int64_t* changed) {
    if (!c) return RTO_E_INVALID;
    if (changed) *changed = 0;
    if (n < 0 || n > RTO_EDIT_MAX_BRUSHES) return fail(c, RTO_E_INVALID, "rto_edit_voxels: n must lie in [0, 65536]");
    if (n > 0 && !brushes) return fail(c, RTO_E_INVALID, "rto_edit_voxels: brushes is NULL");
    const int rcGrid = resident_grid_check(c, "rto_edit_voxels");
    if (rcGrid != RTO_OK) return rcGrid;
    const int dims[3] = { c->voxDim[0], c->voxDim[1], c->voxDim[2] };
    std::vector<rto::EditBrush> host((size_t)n);
    int box[6] = { dims[0], dims[1], dims[2], -1, -1, -1 };        // union, inclusive
    for (int i = 0; i < n; i++) {
        long long cq[3], eq[3];
        if (quantize_brush(&brushes[i], c->gridMin, c->voxelSize, cq, eq) != RTO_OK)
            return fail(c, RTO_E_INVALID, "rto_edit_voxels: brush " + std::to_string(i) + " is invalid (shape, op, NaN / infinite / negative "
                                          "input, or beyond 2^21 voxels)");
        host[(size_t)i] = clip_brush(brushes[i], cq, eq, dims);
        const rto::EditBrush& B = host[(size_t)i];
        if (B.lo[0] > B.hi[0] || B.lo[1] > B.hi[1] || B.lo[2] > B.hi[2]) continue;
        for (int a = 0; a < 3; a++) { box[a] = std::min(box[a], B.lo[a]); box[3 + a] = std::max(box[3 + a], B.hi[a]); }
    }
    c->editMs[0] = c->editMs[1] = c->editMs[2] = -1.f;
    if (n == 0 || box[0] > box[3]) return RTO_OK;                  // nothing inside the grid: nothing to do
    RTO_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    RTO_HIP(c, hipStreamSynchronize(s));
    StreamEvents<2> events;
    RTO_HIP(c, events.create());
    unsigned long long count = 0;
    {
        BuildScratch scratch(s);
        rto::EditBrush* d_brushes = nullptr;
        ChangedCount d_count;
        RTO_HIP(c, scratch.alloc(&d_brushes, (size_t)n));
        RTO_HIP(c, d_count.alloc(scratch));
        RTO_HIP(c, hipMemcpyAsync(d_brushes, host.data(), (size_t)n * sizeof(rto::EditBrush), hipMemcpyHostToDevice, s));
        RTO_HIP(c, d_count.clear(s));
        rto::EditBox eb;
        eb.xlo = box[0]; eb.x0 = box[0] & ~(rto::kEditRun - 1); eb.y0 = box[1]; eb.z0 = box[2];
        eb.x1 = box[3] + 1; eb.y1 = box[4] + 1; eb.z1 = box[5] + 1;
        eb.runsX = (eb.x1 - eb.x0 + rto::kEditRun - 1) / rto::kEditRun;
        eb.blocksX = (eb.runsX + rto::kEditRunsX - 1) / rto::kEditRunsX;
        eb.blocksY = (eb.y1 - eb.y0 + rto::kEditRowsY - 1) / rto::kEditRowsY;
        const long long blocks = (long long)eb.blocksX * eb.blocksY * (eb.z1 - eb.z0);
        if (blocks > 0x7fffffffll) return fail(c, RTO_E_UNSUPPORTED, "rto_edit_voxels: the brushes' box is too large for one launch");
        RTO_HIP(c, events.record(0, s));
        if (dims[0] % rto::kEditRun == 0)
            hipLaunchKernelGGL(rto::k_edit_brushes<true>, dim3((unsigned)blocks), dim3(kBlock), 0, s, c->d_vox, dims[0], dims[1], d_brushes, n, eb, d_count.d);
        else
            hipLaunchKernelGGL(rto::k_edit_brushes<false>, dim3((unsigned)blocks), dim3(kBlock), 0, s, c->d_vox, dims[0], dims[1], d_brushes, n, eb, d_count.d);
        RTO_HIP(c, hipGetLastError());
        RTO_HIP(c, events.record(1, s));
        RTO_HIP(c, d_count.read(s, &count));
    }
    RTO_HIP(c, events.elapsed(0, 1, &c->editMs[0]));
    if (changed) *changed = (int64_t)count;
    if (count == 0) return RTO_OK;           // nothing is dropped: rebuild_from_resident_grid's comment

    return rebuild_from_resident_grid(c, c->d_triOffset != nullptr, &c->editMs[1], &c->editMs[2]);
}

int rto_download_voxels(rto_context* c, uint8_t* out, int64_t capacity, int dims[3]) {
    if (!c) return RTO_E_INVALID;
    const int rcGrid = resident_grid_check(c, "rto_download_voxels");
    if (rcGrid != RTO_OK) return rcGrid;
    if (dims) { dims[0] = c->voxDim[0]; dims[1] = c->voxDim[1]; dims[2] = c->voxDim[2]; }
    if (!out) return RTO_OK;
    return download_resident(c, "rto_download_voxels", out, capacity, c->d_vox, grid_voxels(c), 1);
}

int rto_last_edit_ms(const rto_context* c, float ms[3]) { return copy_last_ms(c, &rto_context::editMs, ms); }

}  // extern "C"
