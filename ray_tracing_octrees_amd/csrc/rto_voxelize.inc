// rto_voxelize.inc -- mesh voxelization (include/rto_hip.h, rto_voxelize_mesh): the reference's loadCSVDataIntoVoxelGrid rule
// (S/BuildingLoader.cpp:131-290) on the GPU, into the grid rto_build_octree keeps in HBM, then the octree from that grid with no
// host copy.  Included at the end of rto_api.hip.
//
// The work per face is uneven (a facade face covers 8-27 voxels of its box, one ground triangle 10^5 or more), so it is spread over
// the flat (face, voxel) pair space (DESIGN.md section 13):
//   k_vox_setup        one thread per face: float vertices, voxel box, the per-face terms of the test in the reference's order
//                      (v0, v1, d00, d01, d11, 1 / denom) and the number of voxels in the box (0: skipped or degenerate face);
//   k_vox_scan_faces   exclusive scan of those counts (block sums, k_scan_counts over them, block-local scans);
//   k_vox_fill         each block finds its first and last face once by binary search in the offsets; each thread then walks
//                      its run of kVoxRun consecutive pairs forward, with the per-voxel part of the test only;
//   k_vox_bbox         the FILLED voxels' integer box and count (recentring and the result's filled count).
// Voxels are written with byte stores of 1 into a buffer cleared by one hipMemsetAsync: two faces may write one byte, with the
// same value.

namespace rto {

constexpr int kVoxRun = 16;                 // pairs per thread of k_vox_fill
constexpr int kVoxBlockPairs = kBlock * kVoxRun;

// One face after k_vox_setup (48 bytes).  lo: the box's first voxel; n: its extent per axis (count = n0 n1 n2).
struct VoxFace {
    float a[3];                             // vertex a (the test's origin)
    float e0[3], e1[3];                     // v0 = c - a, v1 = b - a
    float d00, d01, d11, inv;
    int lo[3], n[3];
};

struct VoxGrid {
    float gmin[3];
    float vs;
    int dims[3];
};

// Float value t truncated to int without overflow?  (int)t is defined for -2^31 <= t < 2^31.
__device__ __forceinline__ bool vox_int_ok(float t) { return t >= -2147483648.0f && t < 2147483648.0f; }

__device__ __forceinline__ float vox_dot(float ax, float ay, float az, float bx, float by, float bz) {
    const float x = ax * bx, y = ay * by, z = az * bz;          // glm 0.9.9.7 compute_dot: tmp = a * b; tmp.x + tmp.y + tmp.z
    return (x + y) + z;
}

__global__ __launch_bounds__(kBlock) void k_vox_setup(const double* __restrict__ xyz, const int* __restrict__ tris, int nf, VoxGrid g,
                                                      VoxFace* __restrict__ faces, long long* __restrict__ counts,
                                                      long long* __restrict__ blockSums, int* __restrict__ invalid) {
    const int f = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    long long cnt = 0;
    if (f < nf) {
        float v[3][3];
        bool finite = true;
        for (int k = 0; k < 3; k++) {
            const long long r = tris[3ll * f + k];
            for (int a = 0; a < 3; a++) {
                v[k][a] = (float)xyz[3 * r + a];              // glm::vec3(double, double, double): round to nearest
                finite = finite && isfinite(v[k][a]);
            }
        }
        VoxFace F;
        bool empty = !finite;
        if (finite) {
            for (int a = 0; a < 3; a++) {
                const float mn = fminf(fminf(v[0][a], v[1][a]), v[2][a]), mx = fmaxf(fmaxf(v[0][a], v[1][a]), v[2][a]);
                const float ts = (mn - g.gmin[a]) / g.vs, te = (mx - g.gmin[a]) / g.vs;
                if (!vox_int_ok(ts) || !vox_int_ok(te)) { atomicOr(invalid, 1); empty = true; continue; }
                const int s = max(0, (int)ts), e = min(g.dims[a] - 1, (int)te + 1);
                F.lo[a] = s; F.n[a] = e - s + 1;
                if (e < s) empty = true;
                F.a[a] = v[0][a];
                F.e0[a] = v[2][a] - v[0][a];
                F.e1[a] = v[1][a] - v[0][a];
            }
        }
        if (!empty) {
            F.d00 = vox_dot(F.e0[0], F.e0[1], F.e0[2], F.e0[0], F.e0[1], F.e0[2]);
            F.d01 = vox_dot(F.e0[0], F.e0[1], F.e0[2], F.e1[0], F.e1[1], F.e1[2]);
            F.d11 = vox_dot(F.e1[0], F.e1[1], F.e1[2], F.e1[0], F.e1[1], F.e1[2]);
            const float dd = F.d00 * F.d11, oo = F.d01 * F.d01;
            const float denom = dd - oo;
            if (fabsf(denom) < 1e-7f) empty = true;            // rejected for every voxel of the face
            F.inv = 1.0f / denom;
        }
        if (!empty) {
            cnt = (long long)F.n[0] * F.n[1] * F.n[2];
            faces[f] = F;
        }
        counts[f] = cnt;
    }
    cnt = block_sum<kBlock>(cnt);                              // for the scan
    if (threadIdx.x == 0) blockSums[blockIdx.x] = cnt;
}

// offsets[f] = exclusive prefix of counts (block-local scan + the block's base); offsets[nf] = total.
__global__ __launch_bounds__(kBlock) void k_vox_scan_faces(const long long* __restrict__ counts, int nf, const long long* __restrict__ blockBase,
                                                           const long long* __restrict__ total, long long* __restrict__ offsets) {
    const int f = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    const long long before = block_exclusive_scan<kBlock>(f < nf ? counts[f] : 0ll);
    if (f < nf) offsets[f] = blockBase[blockIdx.x] + before;
    if (f == 0) offsets[nf] = *total;
}

// Largest f in [lo, hi] with off[f] <= p (off[lo] <= p holds).
__device__ __forceinline__ int vox_face_of(const long long* __restrict__ off, int lo, int hi, long long p) {
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kBlock) void k_vox_fill(const VoxFace* __restrict__ faces, const long long* __restrict__ off, int nf,
                                                     long long total, VoxGrid g, uint8_t* __restrict__ vox) {
    __shared__ int span[2];
    const long long P0 = (long long)blockIdx.x * kVoxBlockPairs;
    const long long P1 = min(P0 + kVoxBlockPairs, total);            // P0 < total
    if (threadIdx.x < 2) span[threadIdx.x] = vox_face_of(off, 0, nf - 1, threadIdx.x == 0 ? P0 : P1 - 1);
    __syncthreads();
    long long p = P0 + (long long)threadIdx.x * kVoxRun;
    if (p >= P1) return;
    const long long pEnd = min(p + kVoxRun, P1);
    int f = vox_face_of(off, span[0], span[1], p);
    long long next = off[f + 1];
    VoxFace F = faces[f];
    long long q = p - off[f];
    const long long nxy = (long long)F.n[0] * F.n[1];
    int z = (int)(q / nxy);
    q -= (long long)z * nxy;
    int y = (int)(q / F.n[0]), x = (int)(q - (long long)y * F.n[0]);
    const size_t sy = (size_t)g.dims[0], sz = (size_t)g.dims[0] * (size_t)g.dims[1];
    for (;;) {
        const int ix = F.lo[0] + x, iy = F.lo[1] + y, iz = F.lo[2] + z;
        const float px = g.gmin[0] + ((float)ix + 0.5f) * g.vs;
        const float py = g.gmin[1] + ((float)iy + 0.5f) * g.vs;
        const float pz = g.gmin[2] + ((float)iz + 0.5f) * g.vs;
        const float wx = px - F.a[0], wy = py - F.a[1], wz = pz - F.a[2];
        const float d02 = vox_dot(F.e0[0], F.e0[1], F.e0[2], wx, wy, wz);
        const float d12 = vox_dot(F.e1[0], F.e1[1], F.e1[2], wx, wy, wz);
        const float un = F.d11 * d02, um = F.d01 * d12;
        const float vn = F.d00 * d12, vm = F.d01 * d02;
        const float u = (un - um) * F.inv;
        const float v = (vn - vm) * F.inv;
        if (u >= 0.0f && v >= 0.0f && u + v <= 1.0f) vox[(size_t)ix + (size_t)iy * sy + (size_t)iz * sz] = 1;
        if (++p >= pEnd) break;
        if (p >= next) {                                              // next face with voxels
            do { f++; next = off[f + 1]; } while (next <= p);
            F = faces[f];
            x = y = z = 0;
        } else if (++x == F.n[0]) {
            x = 0;
            if (++y == F.n[1]) { y = 0; z++; }
        }
    }
}

// The FILLED voxels' box and count: 16 voxels of the flat grid per thread and trip (one 16-byte load when the run is whole),
// a wave and block reduction, then one set of atomics per block.  box: min x, y, z, max x, y, z (initialised by the host).
__global__ __launch_bounds__(kBlock) void k_vox_bbox(const uint8_t* __restrict__ vox, int dimX, int dimY, long long nvox,
                                                     int* __restrict__ box, unsigned long long* __restrict__ filled) {
    int lo[3] = { 0x7fffffff, 0x7fffffff, 0x7fffffff }, hi[3] = { -1, -1, -1 };
    unsigned long long cnt = 0;
    const long long nRuns = (nvox + 15) / 16;
    for (long long r = (long long)blockIdx.x * kBlock + threadIdx.x; r < nRuns; r += (long long)gridDim.x * kBlock) {
        const long long i0 = r * 16;
        unsigned bits = 0u;
        if (i0 + 16 <= nvox) {
            const uint4 w = *reinterpret_cast<const uint4*>(vox + i0);
            const unsigned words[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
            for (int j = 0; j < 16; j++) bits |= (((words[j >> 2] >> (8 * (j & 3))) & 0xffu) != 0u ? 1u : 0u) << j;
        } else {
            for (int j = 0; i0 + j < nvox; j++) bits |= (vox[i0 + j] != 0 ? 1u : 0u) << j;
        }
        if (!bits) continue;
        cnt += (unsigned)__popc(bits);
        const long long row = i0 / dimX;
        int x = (int)(i0 - row * dimX), y = (int)(row % dimY), z = (int)(row / dimY);
        for (int j = 0; j < 16; j++) {
            if ((bits >> j) & 1u) {
                lo[0] = min(lo[0], x); lo[1] = min(lo[1], y); lo[2] = min(lo[2], z);
                hi[0] = max(hi[0], x); hi[1] = max(hi[1], y); hi[2] = max(hi[2], z);
            }
            if (++x == dimX) { x = 0; if (++y == dimY) { y = 0; z++; } }
        }
    }
    struct VoxFilled { unsigned long long cnt; IntBox box; };
    const VoxFilled all = block_reduce<kBlock>(VoxFilled{ cnt, { { lo[0], lo[1], lo[2] }, { hi[0], hi[1], hi[2] } } }, [](VoxFilled a, const VoxFilled& b) {
        a.cnt += b.cnt; a.box = OpBoxUnion()(a.box, b.box);
        return a;
    });
    if (threadIdx.x == 0 && all.cnt) {
        atomicAdd(filled, all.cnt);
#pragma unroll
        for (int a = 0; a < 3; a++) { atomicMin(&box[a], all.box.lo[a]); atomicMax(&box[3 + a], all.box.hi[a]); }
    }
}

}  // namespace rto

namespace {

// The AUTO grid of the rule (include/rto_hip.h), in double as the reference computes it.  false: empty (no finite row or no
// face) or beyond the build's limit (*tooBig).
bool voxelize_auto_grid(const double* xyz, int64_t nv, int64_t nf, float voxelSize, int dims[3], float gmin[3], float* vsOut, bool* tooBig) {
    *tooBig = false;
    if (nv <= 0 || nf <= 0) return false;
    double mn[3] = { std::numeric_limits<double>::max(), std::numeric_limits<double>::max(), std::numeric_limits<double>::max() };
    double mx[3] = { -std::numeric_limits<double>::max(), -std::numeric_limits<double>::max(), -std::numeric_limits<double>::max() };
    bool any = false;
    for (int64_t i = 0; i < nv; i++) {
        const double* r = xyz + 3 * i;
        if (!(std::isfinite(r[0]) && std::isfinite(r[1]) && std::isfinite(r[2]))) continue;
        any = true;
        for (int a = 0; a < 3; a++) { mn[a] = std::min(mn[a], r[a]); mx[a] = std::max(mx[a], r[a]); }
    }
    if (!any) return false;
    const double pad = voxelSize;
    for (int a = 0; a < 3; a++) { mn[a] -= pad; mx[a] += pad; }
    const double kLimit = 9.0e18;                     // (size_t) of the ceil below stays defined
    size_t d[3];
    for (int a = 0; a < 3; a++) {
        const double t = std::ceil((mx[a] - mn[a]) / voxelSize);
        if (!(t < kLimit)) { *tooBig = true; return false; }
        d[a] = (size_t)t;
    }
    const size_t kMaxDim = 1000;
    if (d[0] > kMaxDim || d[1] > kMaxDim || d[2] > kMaxDim) {
        const float scale = (float)std::max({ d[0] / kMaxDim, d[1] / kMaxDim, d[2] / kMaxDim });    // integer division (the quirk)
        voxelSize *= scale;
        for (int a = 0; a < 3; a++) {
            const double t = std::ceil((mx[a] - mn[a]) / voxelSize);
            if (!(t < kLimit)) { *tooBig = true; return false; }
            d[a] = (size_t)t;
        }
    }
    for (int a = 0; a < 3; a++) {
        if (d[a] > ((size_t)1 << kMaxDepth)) { *tooBig = true; return false; }
        dims[a] = (int)d[a];
        gmin[a] = (float)mn[a];
    }
    *vsOut = voxelSize;
    return true;
}

// Owns device buffers until the voxelization commits them to the context.
struct VoxOwned {
    uint8_t* p = nullptr;
    ~VoxOwned() { (void)hipFree(p); }
};

}  // namespace

extern "C" {

int rto_voxelize_mesh(rto_context* c, const double* xyz, int64_t nv, const int32_t* tris, int64_t nf, const rto_voxelize_params* params,
                      rto_voxelize_result* result) {
    if (!c) return RTO_E_INVALID;
    if (!params) return fail(c, RTO_E_INVALID, "rto_voxelize_mesh: params is NULL");
    if (nv < 0 || nf < 0) return fail(c, RTO_E_INVALID, "rto_voxelize_mesh: n_verts and n_tris must be >= 0");
    if ((nv > 0 && !xyz) || (nf > 0 && !tris)) return fail(c, RTO_E_INVALID, "rto_voxelize_mesh: NULL xyz or tris with n > 0");
    if (nf > 0x7fffffffll / kBlock * kBlock - kBlock) return fail(c, RTO_E_INVALID, "rto_voxelize_mesh: too many faces");
    const rto_voxelize_params P = *params;
    if (P.mode != RTO_VOXELIZE_AUTO && P.mode != RTO_VOXELIZE_FIXED) return fail(c, RTO_E_INVALID, "rto_voxelize_mesh: unknown mode");
    if (P.recenter_passes < 0 || P.recenter_passes > 2) return fail(c, RTO_E_INVALID, "rto_voxelize_mesh: recenter_passes must be 0, 1 or 2");
    if (!std::isfinite(P.voxel_size) || !(P.voxel_size > 0.f)) return fail(c, RTO_E_INVALID, "rto_voxelize_mesh: voxel_size must be finite and positive");
    for (int64_t i = 0; i < 3 * nf; i++)
        if (tris[i] < 0 || (int64_t)tris[i] >= nv)
            return fail(c, RTO_E_INVALID, "rto_voxelize_mesh: face " + std::to_string(i / 3) + " names a row outside [0, n_verts)");
    rto::VoxGrid g;
    if (P.mode == RTO_VOXELIZE_FIXED) {
        for (int a = 0; a < 3; a++) {
            if (P.dims[a] < 1) return fail(c, RTO_E_INVALID, "rto_voxelize_mesh: FIXED dims must be >= 1");
            if (P.dims[a] > (1 << kMaxDepth)) return fail(c, RTO_E_INVALID, "rto_voxelize_mesh: grid above the build's size limit");
            if (!std::isfinite(P.grid_min[a])) return fail(c, RTO_E_INVALID, "rto_voxelize_mesh: FIXED grid_min must be finite");
            g.dims[a] = P.dims[a]; g.gmin[a] = P.grid_min[a];
        }
        g.vs = P.voxel_size;
    } else {
        bool tooBig = false;
        if (!voxelize_auto_grid(xyz, nv, nf, P.voxel_size, g.dims, g.gmin, &g.vs, &tooBig))
            return fail(c, RTO_E_INVALID, tooBig ? "rto_voxelize_mesh: grid above the build's size limit"
                                                 : "rto_voxelize_mesh: empty grid (no face, or no row with finite coordinates)");
    }
    const size_t nvox = (size_t)g.dims[0] * g.dims[1] * g.dims[2];

    RTO_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    RTO_HIP(c, hipStreamSynchronize(s));
    StreamEvents<4> events;
    RTO_HIP(c, events.create());
    float ms[4] = { -1.f, -1.f, -1.f, -1.f };
    VoxOwned vox;
    RTO_HIP(c, hipMalloc(&vox.p, nvox));
    RTO_HIP(c, hipMemsetAsync(vox.p, 0, nvox, s));
    long long pairs = 0;
    unsigned long long filled = 0;
    int box[6] = { 0x7fffffff, 0x7fffffff, 0x7fffffff, -1, -1, -1 };
    {
        BuildScratch scratch(s);
        if (nf > 0) {
            const int nfi = (int)nf;
            const int nb = (nfi + kBlock - 1) / kBlock;
            double* d_xyz = nullptr;
            int* d_tris = nullptr;
            rto::VoxFace* d_faces = nullptr;
            long long *d_counts = nullptr, *d_sums = nullptr, *d_off = nullptr, *d_total = nullptr;
            int* d_invalid = nullptr;
            RTO_HIP(c, scratch.alloc(&d_xyz, (size_t)nv * 3));
            RTO_HIP(c, scratch.alloc(&d_tris, (size_t)nf * 3));
            RTO_HIP(c, scratch.alloc(&d_faces, (size_t)nf));
            RTO_HIP(c, scratch.alloc(&d_counts, (size_t)nf));
            RTO_HIP(c, scratch.alloc(&d_sums, (size_t)nb));
            RTO_HIP(c, scratch.alloc(&d_off, (size_t)nf + 1));
            RTO_HIP(c, scratch.alloc(&d_total, 2));
            RTO_HIP(c, scratch.alloc(&d_invalid, 1));
            RTO_HIP(c, hipMemcpyAsync(d_xyz, xyz, (size_t)nv * 3 * sizeof(double), hipMemcpyHostToDevice, s));
            RTO_HIP(c, hipMemcpyAsync(d_tris, tris, (size_t)nf * 3 * sizeof(int), hipMemcpyHostToDevice, s));
            RTO_HIP(c, hipMemsetAsync(d_invalid, 0, sizeof(int), s));
            RTO_HIP(c, events.record(0, s));
            hipLaunchKernelGGL(rto::k_vox_setup, dim3((unsigned)nb), dim3(kBlock), 0, s, d_xyz, d_tris, nfi, g, d_faces, d_counts, d_sums, d_invalid);
            hipLaunchKernelGGL((rto::k_scan_counts<1024, long long, long long>), dim3(1), dim3(1024), 0, s, d_sums, nb, d_sums, d_total);
            hipLaunchKernelGGL(rto::k_vox_scan_faces, dim3((unsigned)nb), dim3(kBlock), 0, s, d_counts, nfi, d_sums, d_total, d_off);
            RTO_HIP(c, hipGetLastError());
            RTO_HIP(c, events.record(1, s));
            long long total = 0;
            int invalid = 0;
            RTO_HIP(c, hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, s));
            RTO_HIP(c, hipMemcpyAsync(&invalid, d_invalid, sizeof invalid, hipMemcpyDeviceToHost, s));
            RTO_HIP(c, hipStreamSynchronize(s));
            if (invalid)
                return fail(c, RTO_E_INVALID, "rto_voxelize_mesh: a face's voxel box overflows int (the reference's cast is undefined there)");
            const long long blocks = (total + rto::kVoxBlockPairs - 1) / rto::kVoxBlockPairs;
            if (blocks > 0x7fffffffll) return fail(c, RTO_E_UNSUPPORTED, "rto_voxelize_mesh: too many (face, voxel) pairs for one launch");
            pairs = total;
            if (blocks > 0)
                hipLaunchKernelGGL(rto::k_vox_fill, dim3((unsigned)blocks), dim3(kBlock), 0, s, d_faces, d_off, nfi, total, g, vox.p);
            RTO_HIP(c, hipGetLastError());
        } else {
            RTO_HIP(c, events.record(0, s));
            RTO_HIP(c, events.record(1, s));
        }
        RTO_HIP(c, events.record(2, s));
        int* d_box = nullptr;
        unsigned long long* d_filled = nullptr;
        RTO_HIP(c, scratch.alloc(&d_box, 6));
        RTO_HIP(c, scratch.alloc(&d_filled, 1));
        RTO_HIP(c, hipMemcpyAsync(d_box, box, sizeof box, hipMemcpyHostToDevice, s));
        RTO_HIP(c, hipMemsetAsync(d_filled, 0, sizeof(unsigned long long), s));
        const long long runs = ((long long)nvox + 15) / 16;
        const unsigned bb = (unsigned)std::max<long long>(1, std::min<long long>((runs + kBlock - 1) / kBlock, (long long)c->numCUs * 8));
        hipLaunchKernelGGL(rto::k_vox_bbox, dim3(bb), dim3(kBlock), 0, s, vox.p, g.dims[0], g.dims[1], (long long)nvox, d_box, d_filled);
        RTO_HIP(c, hipGetLastError());
        RTO_HIP(c, events.record(3, s));
        RTO_HIP(c, hipMemcpyAsync(box, d_box, sizeof box, hipMemcpyDeviceToHost, s));
        RTO_HIP(c, hipMemcpyAsync(&filled, d_filled, sizeof filled, hipMemcpyDeviceToHost, s));
        RTO_HIP(c, hipStreamSynchronize(s));
    }
    if (nf > 0) {
        RTO_HIP(c, events.elapsed(0, 1, &ms[0]));
        RTO_HIP(c, events.elapsed(1, 2, &ms[1]));
    }
    RTO_HIP(c, events.elapsed(2, 3, &ms[2]));

    // recentring (S/main.cpp:376-422): the centres are non-decreasing in the index, so the min / max centre is the centre of the
    // min / max FILLED index, in the reference's float arithmetic
    float gmin[3] = { g.gmin[0], g.gmin[1], g.gmin[2] };
    for (int pass = 0; pass < P.recenter_passes && filled > 0; pass++) {
        for (int a = 0; a < 3; a++) {
            const float lo = gmin[a] + ((float)box[a] + 0.5f) * g.vs;
            const float hi = gmin[a] + ((float)box[3 + a] + 0.5f) * g.vs;
            const float centre = 0.5f * (lo + hi);
            gmin[a] -= centre;
        }
    }

    // ---- commit: adopt the new grid, then rebuild_from_resident_grid -- what rto_build_octree(grid, gmin, vs) leaves
    free_octree(c);
    std::memcpy(c->gridMin, gmin, sizeof c->gridMin);
    c->voxelSize = g.vs;
    c->d_vox = vox.p; vox.p = nullptr;
    c->voxDim[0] = g.dims[0]; c->voxDim[1] = g.dims[1]; c->voxDim[2] = g.dims[2];
    for (int i = 0; i < 4; i++) c->voxelizeMs[i] = ms[i];
    const int rcBuild = rebuild_from_resident_grid(c, P.triangles != 0, &c->voxelizeMs[3], nullptr);
    if (rcBuild != RTO_OK) return rcBuild;
    if (result) {
        std::memset(result, 0, sizeof *result);
        for (int a = 0; a < 3; a++) { result->dims[a] = g.dims[a]; result->grid_min[a] = gmin[a]; }
        result->voxel_size = g.vs;
        result->filled = (int64_t)filled;
        result->pairs = (int64_t)pairs;
    }
    return RTO_OK;
}

int rto_last_voxelize_ms(const rto_context* c, float ms[4]) { return copy_last_ms(c, &rto_context::voxelizeMs, ms); }

}  // extern "C"
