// rto_dc.inc -- dual contouring (include/rto_hip.h, rto_extract_dual_contour, rto_query_dual_vertices_*): the reference's per-voxel
// vertex rule (gatherHermiteData with size 1, calculateIntersection, generateDualVertex, QEFSolver) and its triangulation
// buildTrianglesCPU (453-skeleton/AdaptiveDualContouringRenderer.cpp:49-161, 377-486, 1090-1357) over the resident grid.  Included
// at the end of rto_api.hip, after rto_iso.inc, whose ranking kernels (k_iso_sums, k_iso_scan_sums, k_iso_offsets) it launches
// unchanged.  The rule is DESIGN.md section 32's; its arithmetic is host/DualVertex.h, shared word for word with the CPU form.
//
// Shape, as section 30's.  A run is 32 cells along x at an aligned x; runs are numbered in raster order over the cell box, so an
// exclusive scan of the runs' triangle counts is the reference's order and nothing is sorted.  The rows of y and z (and the tiles
// along x) reach one past the last cell: every voxel a face can read then belongs to exactly one tile, which counts it.
//   k_dc_count   a workgroup per tile of 32 x 8 x 8 cells: it stages the solid bits of the tile and its halo (-1 .. +3 voxels:
//                a quad reads the vertex of voxel c + 1, that vertex gathers voxels up to c + 2 and their neighbours up to c + 3,
//                the central differences read +-1) in LDS, 36 x 12 x 12 bytes.  A tile whose staged bits are all equal writes
//                zeros and leaves.  Each thread walks a column of 8 cells: per cell the faces and, per face, which of its two
//                triangles the area rule keeps -- under RTO_DC_AREA_REFERENCE from the four vertices, computed from the staged
//                bits; under RTO_DC_AREA_NONE without any vertex.  One byte per cell (a base-5 digit per face: none, or 1 + the
//                kept mask) and one count per run (a half-wave sum).  No atomics for the counts; the summary's faces and
//                voxels go through the tally slots, one add per workgroup.
//   rank         k_iso_sums / k_iso_scan_sums / k_iso_offsets.
//   k_dc_place   a half-wave per active run, a lane per cell: tri_cell and (axis, triangle) of each kept triangle.
//   k_dc_emit    one thread per triangle: it computes its three vertices from the grid in HBM (the voxels of neighbouring
//                triangles sit in the same wave: the loads hit the same lines) and writes three float4.
//   k_dc_query   one thread per queried voxel.
// No kernel here indexes an array by a variable: none uses scratch (tests/test_dual_contour.py reads the code object's metadata).

#include "../host/DualVertex.h"

namespace rto {

constexpr int kDcHaloX = kIsoTileX + 4, kDcHaloY = kIsoTileY + 4, kDcHaloZ = kIsoTileZ + 4;      // voxels -1 .. tile + 2
constexpr int kDcHalo = kDcHaloX * kDcHaloY * kDcHaloZ;

struct DcArgs {
    const uint8_t* vox;              // dimZ x dimY x dimX, x fastest; FILLED is 1
    rto_dc::Grid g;
    int lo[3], hi[3];                // the cells: lo <= c < hi (hi <= dim - 1)
    int t0[3];                       // the first tile on each axis
    int runsX, ny, nz;               // runs along x; rows along y and z: the cells' and one more
    int areaRule;
};

struct DcSolidGlobal {
    const uint8_t* v;
    int dx, dy, dz;
    __device__ __forceinline__ bool operator()(int x, int y, int z) const {
        if (x < 0 || y < 0 || z < 0 || x >= dx || y >= dy || z >= dz) return false;
        return v[((size_t)z * (size_t)dy + (size_t)y) * (size_t)dx + (size_t)x] == 1;
    }
};
// The staged bits of one tile; (x0, y0, z0): the voxel of entry 0.  The caller stays inside the halo.
struct DcSolidTile {
    const uint8_t* s;
    int x0, y0, z0;
    __device__ __forceinline__ bool operator()(int x, int y, int z) const {
        return s[((z - z0) * kDcHaloY + (y - y0)) * kDcHaloX + (x - x0)] != 0;
    }
};

__device__ __forceinline__ size_t dc_run(const DcArgs& A, int bx, int y, int z) {
    return ((size_t)(z - A.lo[2]) * (size_t)A.ny + (size_t)(y - A.lo[1])) * (size_t)A.runsX + (size_t)bx;
}
__device__ __forceinline__ bool dc_cell_in_box(const DcArgs& A, int x, int y, int z) {
    return x >= A.lo[0] && x < A.hi[0] && y >= A.lo[1] && y < A.hi[1] && z >= A.lo[2] && z < A.hi[2];
}

// Which of the two triangles of the face of cell (x, y, z) towards +axis does the area rule keep: bit 0, bit 1.
template <class Solid> __device__ __forceinline__ unsigned dc_face_kept(const Solid& S, const rto_dc::Grid& g, int x, int y, int z, int axis) {
    rto_dc::V3 q0{ 0.f, 0.f, 0.f }, q1 = q0, q2 = q0, q3 = q0;
    for (int k = 0; k < 4; k++) {                        // one body, four trips: the vertex function is inlined once
        const int o = rto_dc::face_corner(axis, k);
        rto_dc::V3 v;
        rto_dc::vertex(S, g, x + (o & 1), y + ((o >> 1) & 1), z + ((o >> 2) & 1), &v);
        if (k == 0) q0 = v; else if (k == 1) q1 = v; else if (k == 2) q2 = v; else q3 = v;
    }
    rto_dc::V3 n;
    float l2a, l2b;
    (void)rto_dc::triangle_normal(q0, q1, q2, false, &n, &l2a);
    (void)rto_dc::triangle_normal(q0, q2, q3, false, &n, &l2b);
    return (rto_dc::area_kept(l2a) ? 1u : 0u) | (rto_dc::area_kept(l2b) ? 2u : 0u);
}

__global__ __launch_bounds__(kBlock) void k_dc_count(DcArgs A, int tilesX, int tilesY, unsigned* __restrict__ runCount, uint8_t* __restrict__ cases,
                                                    unsigned long long* __restrict__ tally) {
    __shared__ uint8_t bits[kDcHalo];
    const int t = (int)threadIdx.x;
    const int bx = (int)(blockIdx.x % (unsigned)tilesX);
    const unsigned rest = blockIdx.x / (unsigned)tilesX;
    const int by = (int)(rest % (unsigned)tilesY), bz = (int)(rest / (unsigned)tilesY);
    const int c0x = (A.t0[0] + bx) * kIsoTileX, c0y = (A.t0[1] + by) * kIsoTileY, c0z = (A.t0[2] + bz) * kIsoTileZ;
    const DcSolidGlobal G{ A.vox, A.g.dimX, A.g.dimY, A.g.dimZ };

    int anySolid = 0, anyEmpty = 0;
    for (int i = t; i < kDcHalo; i += kBlock) {
        const int sx = i % kDcHaloX, r = i / kDcHaloX;
        const int sy = r % kDcHaloY, sz = r / kDcHaloY;
        const bool s = G(c0x - 1 + sx, c0y - 1 + sy, c0z - 1 + sz);
        bits[i] = s ? 1 : 0;
        anySolid |= s ? 1 : 0; anyEmpty |= s ? 0 : 1;
    }
    anySolid = __syncthreads_or(anySolid);               // also the barrier behind the staging
    anyEmpty = __syncthreads_or(anyEmpty);
    if (!anySolid || !anyEmpty) {                        // block-uniform: no face, and no voxel a face reads
        if (t < kIsoTileY * kIsoTileZ) {
            const int y = c0y + (t & 7), z = c0z + (t >> 3);
            if (y >= A.lo[1] && y <= A.hi[1] && z >= A.lo[2] && z <= A.hi[2]) runCount[dc_run(A, bx, y, z)] = 0u;
        }
        return;
    }

    const DcSolidTile S{ bits, c0x - 1, c0y - 1, c0z - 1 };
    const int lx = t & 31, ly = t >> 5;
    const int x = c0x + lx, y = c0y + ly;
    const bool rowY = y >= A.lo[1] && y <= A.hi[1];      // uniform over the half-wave
    unsigned faces = 0u, voxels = 0u;
    for (int lz = 0; lz < kIsoTileZ; lz++) {
        const int z = c0z + lz;
        const bool rowZ = z >= A.lo[2] && z <= A.hi[2];
        unsigned code = 0u, n = 0u;
        if (dc_cell_in_box(A, x, y, z)) {
            const bool c = S(x, y, z);
            unsigned mul = 1u;
            for (int axis = 0; axis < 3; axis++, mul *= 5u) {
                if (S(x + (axis == 0 ? 1 : 0), y + (axis == 1 ? 1 : 0), z + (axis == 2 ? 1 : 0)) == c) continue;
                faces++;
                const unsigned kept = A.areaRule == RTO_DC_AREA_NONE ? 3u : dc_face_kept(S, A.g, x, y, z, axis);
                code += (1u + kept) * mul;
                n += (kept & 1u) + (kept >> 1);
            }
        }
        // this tile's voxel (x, y, z): is it one of the four of a face found, and has it a Hermite point
        if (x < A.g.dimX && y < A.g.dimY && z < A.g.dimZ) {
            bool read = false;
            for (int j = 0; j < 12; j++) {
                const int axis = j >> 2, q = j & 3;
                const int o = rto_dc::face_corner(axis, q);
                const int cx = x - (o & 1), cy = y - ((o >> 1) & 1), cz = z - ((o >> 2) & 1);
                if (dc_cell_in_box(A, cx, cy, cz) && S(cx, cy, cz) != S(cx + (axis == 0 ? 1 : 0), cy + (axis == 1 ? 1 : 0), cz + (axis == 2 ? 1 : 0))) read = true;
            }
            if (read && rto_dc::has_point(S, A.g, x, y, z)) voxels++;
        }
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) n += lane_xor(n, off);          // the half-wave's 32 cells
        if (rowY && rowZ) {
            const size_t run = dc_run(A, bx, y, z);
            cases[run * 32 + (size_t)lx] = (uint8_t)code;
            if (lx == 0) runCount[run] = n;
        }
    }
    // one reduction, one barrier, for both: a thread has at most 24 faces and 8 voxels, a workgroup fewer than 2^32 of either
    const unsigned long long both = block_sum<kBlock>((unsigned long long)faces | (unsigned long long)voxels << 32);      // every thread is here
    faces = (unsigned)(both & 0xffffffffull);
    voxels = (unsigned)(both >> 32);
    if (t == 0) {
        if (faces) atomicAdd(tally + 4 * (blockIdx.x % kIsoTallySlots), (unsigned long long)faces);
        if (voxels) atomicAdd(tally + 4 * (blockIdx.x % kIsoTallySlots) + 1, (unsigned long long)voxels);
    }
}

// The kept triangles of a cell's code, in order: bit 2 axis + t.
__device__ __forceinline__ unsigned dc_kept_bits(unsigned code) {
    unsigned bits = 0u;
#pragma unroll
    for (int axis = 0; axis < 3; axis++) {
        const unsigned digit = code % 5u;
        code /= 5u;
        if (digit) bits |= (digit - 1u) << (2 * axis);
    }
    return bits;
}

__global__ __launch_bounds__(kBlock) void k_dc_place(DcArgs A, const uint8_t* __restrict__ cases, const unsigned* __restrict__ activeRun,
                                                    const unsigned* __restrict__ activeOff, unsigned active, int* __restrict__ triCell,
                                                    uint8_t* __restrict__ triWhich) {
    const int t = (int)threadIdx.x;
    const unsigned hw = blockIdx.x * (unsigned)(kBlock / 32) + ((unsigned)t >> 5);
    const int lane = t & 31;
    unsigned bits = 0u, base = 0u;
    int cell = 0;
    if (hw < active) {                                   // uniform over the half-wave, not over the wave
        const unsigned run = activeRun[hw];
        base = activeOff[hw];
        const unsigned rx = run % (unsigned)A.runsX, q = run / (unsigned)A.runsX;
        const int x = (A.t0[0] + (int)rx) * kIsoTileX + lane;
        const int y = A.lo[1] + (int)(q % (unsigned)A.ny), z = A.lo[2] + (int)(q / (unsigned)A.ny);
        bits = dc_kept_bits(cases[(size_t)run * 32 + (size_t)lane]);
        if (bits) cell = (z * A.g.dimY + y) * A.g.dimX + x;      // < 2^31 (dc_check); a lane past the box has no bit and forms no index
    }
    const unsigned n = (unsigned)__builtin_popcount(bits);
    unsigned incl = n;                                   // the prefix inside the run
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {
        const unsigned up = __shfl_up(incl, off, 32);
        if (lane >= off) incl += up;
    }
    size_t d = (size_t)base + (size_t)(incl - n);
    for (unsigned k = 0; k < 6u; k++)
        if (bits >> k & 1u) {
            triCell[d] = cell;
            triWhich[d] = (uint8_t)k;
            d++;
        }
}

__global__ __launch_bounds__(kBlock) void k_dc_emit(DcArgs A, const uint8_t* __restrict__ triWhich, const int* __restrict__ triCell, unsigned total,
                                                   float4* __restrict__ dst, unsigned long long* __restrict__ tally) {
    const unsigned d = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    unsigned degenerate = 0u;
    if (d < total) {
        const DcSolidGlobal G{ A.vox, A.g.dimX, A.g.dimY, A.g.dimZ };
        const int which = triWhich[d], axis = which >> 1, tri = which & 1;
        const int cell = triCell[d];
        const int x = cell % A.g.dimX, r = cell / A.g.dimX;
        const int y = r % A.g.dimY, z = r / A.g.dimY;
        rto_dc::V3 a{ 0.f, 0.f, 0.f }, b = a, c = a;
        for (int k = 0; k < 3; k++) {                    // corners 0, 1 + tri, 2 + tri of the face
            const int o = rto_dc::face_corner(axis, k == 0 ? 0 : k + tri);
            rto_dc::V3 v;
            rto_dc::vertex(G, A.g, x + (o & 1), y + ((o >> 1) & 1), z + ((o >> 2) & 1), &v);
            if (k == 0) a = v; else if (k == 1) b = v; else c = v;
        }
        rto_dc::V3 n;
        float l2;
        if (!rto_dc::triangle_normal(a, b, c, G(x, y, z), &n, &l2)) degenerate = 1u;
        float4* o = dst + 3 * (size_t)d;
        o[0] = make_float4(a.x, a.y, a.z, b.x);
        o[1] = make_float4(b.y, b.z, c.x, c.y);
        o[2] = make_float4(c.z, n.x, n.y, n.z);
    }
    const unsigned nDeg = wave_sum(degenerate);          // every lane of the wave is here
    if ((threadIdx.x & 63) == 0 && nDeg) atomicAdd(tally + 4 * (blockIdx.x % kIsoTallySlots) + 2, (unsigned long long)nDeg);
}

__global__ __launch_bounds__(kBlock) void k_dc_query(const uint8_t* __restrict__ vox, rto_dc::Grid g, const long long* __restrict__ voxels, long long n,
                                                    rto_dual_vertex* __restrict__ out) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const long long v = voxels[i];
    const long long nvox = (long long)g.dimX * g.dimY * g.dimZ;
    rto_dual_vertex res;
    res.p[0] = res.p[1] = res.p[2] = 0.0f;
    res.points = -1;
    if (v >= 0 && v < nvox) {
        const DcSolidGlobal G{ vox, g.dimX, g.dimY, g.dimZ };
        const int x = (int)(v % g.dimX), y = (int)(v / g.dimX % g.dimY), z = (int)(v / ((long long)g.dimX * g.dimY));
        rto_dc::V3 p;
        res.points = rto_dc::vertex(G, g, x, y, z, &p);
        res.p[0] = p.x; res.p[1] = p.y; res.p[2] = p.z;
    }
    out[i] = res;
}

}  // namespace rto

// ---------------------------------------------------------------- host side
static_assert(sizeof(rto_dc_params) == 48 && sizeof(rto_dc_summary) == 48 && sizeof(rto_dual_vertex) == 16, "the ABI's sizes");

static rto_dc::Grid dc_grid(const rto_context* c) {
    return rto_dc::Grid{ c->voxDim[0], c->voxDim[1], c->voxDim[2], c->gridMin[0], c->gridMin[1], c->gridMin[2], c->voxelSize };
}

// Every check of an extraction but the triangle count, in the order the ABI promises.
static int dc_check(rto_context* c, const char* fn, const rto_dc_params* p) {
    const std::string name(fn);
    if (!p) return fail(c, RTO_E_INVALID, name + ": params is NULL");
    if (p->area_rule != RTO_DC_AREA_REFERENCE && p->area_rule != RTO_DC_AREA_NONE)
        return fail(c, RTO_E_INVALID, name + ": unknown area_rule " + std::to_string(p->area_rule));
    for (int r : p->reserved) if (r != 0) return fail(c, RTO_E_INVALID, name + ": params.reserved must be 0");
    if (c->numNodes <= 0) return fail(c, RTO_E_NO_OCTREE, name + ": no octree uploaded");
    if (!c->d_vox) return fail(c, RTO_E_UNSUPPORTED, name + ": the octree came from rto_upload_octree: no voxel grid is resident");
    if (grid_voxels(c) > 0x7fffffffll) return fail(c, RTO_E_UNSUPPORTED, name + ": the grid has more than 2^31 - 1 voxels: a cell's index does not fit tri_cell");
    return check_clip_box(c, name, p->clip, p->clip_lo, p->clip_hi);
}

static int dc_extract(rto_context* c, const char* fn, const rto_dc_params* p, rto_dc_summary* summary) {
    using namespace rto;
    hipStream_t s = c->stream;
    DcArgs A;
    std::memset(&A, 0, sizeof A);
    A.vox = c->d_vox;
    A.g = dc_grid(c);
    A.areaRule = p->area_rule;
    bool empty = false;
    const int tile[3] = { kIsoTileX, kIsoTileY, kIsoTileZ };
    int tiles[3] = { 0, 0, 0 };
    for (int a = 0; a < 3; a++) {
        A.lo[a] = p->clip ? p->clip_lo[a] : 0;
        A.hi[a] = std::min(p->clip ? p->clip_hi[a] : c->voxDim[a], c->voxDim[a] - 1);
        if (A.hi[a] <= A.lo[a]) { empty = true; continue; }
        A.t0[a] = A.lo[a] / tile[a];
        tiles[a] = A.hi[a] / tile[a] + 1 - A.t0[a];          // the tiles that hold lo .. hi, hi included
    }
    A.runsX = tiles[0]; A.ny = A.hi[1] - A.lo[1] + 1; A.nz = A.hi[2] - A.lo[2] + 1;

    long long total = 0, activeRuns = 0;
    std::vector<unsigned long long> slots(4 * kIsoTallySlots, 0ull);
    unsigned long long tally[3] = { 0ull, 0ull, 0ull };
    float ms[3] = { -1.f, -1.f, -1.f };                       // an empty cell box runs no kernel
    if (!empty) {
        // count: events 0 .. 1; rank: 1 .. 2; emit: 3 .. 4, begun after the count's read-back and the output buffer's growth
        StreamEvents<5> events;
        RTO_HIP(c, events.create());
        BuildScratch scratch(s);
        const long long runs = (long long)A.runsX * A.ny * A.nz;
        const long long nb = (runs + kIsoRunsPerBlock - 1) / kIsoRunsPerBlock;
        unsigned *d_runCount = nullptr, *d_activeRun = nullptr, *d_activeOff = nullptr;
        uint8_t* d_cases = nullptr;
        long long *d_blockTris = nullptr, *d_total = nullptr;
        unsigned *d_blockActive = nullptr, *d_totalActive = nullptr;
        unsigned long long* d_tally = nullptr;
        RTO_HIP(c, scratch.alloc(&d_runCount, (size_t)runs));
        RTO_HIP(c, scratch.alloc(&d_activeRun, (size_t)runs));
        RTO_HIP(c, scratch.alloc(&d_activeOff, (size_t)runs));
        RTO_HIP(c, scratch.alloc(&d_cases, (size_t)runs * 32));
        RTO_HIP(c, scratch.alloc(&d_blockTris, (size_t)nb));
        RTO_HIP(c, scratch.alloc(&d_blockActive, (size_t)nb));
        RTO_HIP(c, scratch.alloc(&d_total, 1));
        RTO_HIP(c, scratch.alloc(&d_totalActive, 1));
        RTO_HIP(c, scratch.alloc(&d_tally, slots.size()));
        RTO_HIP(c, hipMemsetAsync(d_tally, 0, slots.size() * sizeof(unsigned long long), s));

        RTO_HIP(c, events.record(0, s));
        hipLaunchKernelGGL(k_dc_count, dim3((unsigned)((int64_t)tiles[0] * tiles[1] * tiles[2])), dim3(kBlock), 0, s, A, tiles[0], tiles[1], d_runCount,
                           d_cases, d_tally);
        RTO_HIP(c, hipGetLastError());
        RTO_HIP(c, events.record(1, s));
        hipLaunchKernelGGL(k_iso_sums, dim3((unsigned)nb), dim3(kBlock), 0, s, d_runCount, runs, d_blockTris, d_blockActive);
        hipLaunchKernelGGL(k_iso_scan_sums, dim3(1), dim3(1024), 0, s, d_blockTris, d_blockActive, (int)nb, d_total, d_totalActive);
        hipLaunchKernelGGL(k_iso_offsets, dim3((unsigned)nb), dim3(kBlock), 0, s, d_runCount, runs, d_blockTris, d_blockActive, d_activeRun, d_activeOff);
        RTO_HIP(c, hipGetLastError());
        RTO_HIP(c, events.record(2, s));
        unsigned active = 0u;
        RTO_HIP(c, hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, s));     // the read-back that sizes the output
        RTO_HIP(c, hipMemcpyAsync(&active, d_totalActive, sizeof active, hipMemcpyDeviceToHost, s));
        RTO_HIP(c, hipStreamSynchronize(s));
        activeRuns = (long long)active;
        if (total >= kIsoTooMany) return fail(c, RTO_E_UNSUPPORTED, std::string(fn) + ": more than 2^31 - 1 triangles");

        // ---- emit into a buffer of the context's own (the previous list lives until here)
        if (total > c->dcCap || !c->d_dc) {
            float4* d_new = nullptr;
            int* d_newCell = nullptr;
            const size_t cap = total ? (size_t)total : 1;
            RTO_HIP(c, hipMalloc(&d_new, cap * 3 * sizeof(float4)));
            if (hipMalloc(&d_newCell, cap * sizeof(int)) != hipSuccess) { (void)hipFree(d_new); return fail(c, RTO_E_HIP, std::string(fn) + ": out of device memory"); }
            (void)hipFree(c->d_dc); (void)hipFree(c->d_dcCell);
            c->d_dc = d_new; c->d_dcCell = d_newCell; c->dcCap = (int64_t)cap;
            c->dcTris = -1;                                  // the old list is gone: nothing is served until this one is complete
        }
        uint8_t* d_which = nullptr;
        RTO_HIP(c, scratch.alloc(&d_which, (size_t)total));
        RTO_HIP(c, events.record(3, s));
        if (total > 0) {
            hipLaunchKernelGGL(k_dc_place, dim3((unsigned)((activeRuns + kBlock / 32 - 1) / (kBlock / 32))), dim3(kBlock), 0, s, A, d_cases, d_activeRun,
                               d_activeOff, (unsigned)activeRuns, c->d_dcCell, d_which);
            hipLaunchKernelGGL(k_dc_emit, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, A, d_which, c->d_dcCell, (unsigned)total,
                               c->d_dc, d_tally);
            RTO_HIP(c, hipGetLastError());
        }
        RTO_HIP(c, events.record(4, s));
        RTO_HIP(c, hipMemcpyAsync(slots.data(), d_tally, slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        RTO_HIP(c, hipStreamSynchronize(s));
        for (int k = 0; k < kIsoTallySlots; k++)
            for (int j = 0; j < 3; j++) tally[j] += slots[4 * k + j];
        RTO_HIP(c, events.elapsed(0, 1, &ms[0]));
        RTO_HIP(c, events.elapsed(1, 2, &ms[1]));
        RTO_HIP(c, events.elapsed(3, 4, &ms[2]));
    }
    c->dcTris = (int64_t)total;
    std::memcpy(c->dcMs, ms, sizeof ms);
    if (summary) {
        summary->faces = (int64_t)tally[0]; summary->triangles = (int64_t)total; summary->dropped = 2 * (int64_t)tally[0] - (int64_t)total;
        summary->degenerate = (int64_t)tally[2]; summary->vertex_voxels = (int64_t)tally[1]; summary->reserved = 0;
    }
    return RTO_OK;
}

// The checks of a vertex query, then its launch; d_voxels and d_out are on the device.
static int dc_query_check(rto_context* c, const char* fn, const void* voxels, int64_t n, const void* out) {
    const std::string name(fn);
    if (n < 0) return fail(c, RTO_E_INVALID, name + ": n is negative");
    if (n > 0 && (!voxels || !out)) return fail(c, RTO_E_INVALID, name + ": voxels or out is NULL");
    if ((reinterpret_cast<uintptr_t>(voxels) & 7) != 0 || (reinterpret_cast<uintptr_t>(out) & 3) != 0)
        return fail(c, RTO_E_INVALID, name + ": voxels must be 8-byte aligned, out 4-byte aligned");
    if (c->numNodes <= 0) return fail(c, RTO_E_NO_OCTREE, name + ": no octree uploaded");
    if (!c->d_vox) return fail(c, RTO_E_UNSUPPORTED, name + ": the octree came from rto_upload_octree: no voxel grid is resident");
    return RTO_OK;
}
static int dc_query_launch(rto_context* c, const int64_t* d_voxels, int64_t n, rto_dual_vertex* d_out) {
    using namespace rto;
    const int64_t chunk = (int64_t)kBlock << 20;             // a grid of at most 2^20 workgroups
    for (int64_t i = 0; i < n; i += chunk) {
        const int64_t m = std::min(chunk, n - i);
        hipLaunchKernelGGL(k_dc_query, dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, c->d_vox, dc_grid(c),
                           reinterpret_cast<const long long*>(d_voxels + i), (long long)m, d_out + i);
    }
    RTO_HIP(c, hipGetLastError());
    return RTO_OK;
}

extern "C" {

int rto_extract_dual_contour(rto_context* c, const rto_dc_params* params, rto_dc_summary* summary) {
    if (!c) return RTO_E_INVALID;
    const char* fn = "rto_extract_dual_contour";
    const int rc = dc_check(c, fn, params);
    if (rc != RTO_OK) return rc;
    RTO_HIP(c, hipSetDevice(c->device));
    return dc_extract(c, fn, params, summary);
}

int rto_dual_contour_device(rto_context* c, void** d_tris, int32_t** d_tri_cell, int64_t* num_tris) {
    if (!c || !num_tris) return RTO_E_INVALID;
    if (c->dcTris < 0) return fail(c, RTO_E_INVALID, "rto_dual_contour_device: no dual-contour list extracted");
    if (d_tris) *d_tris = c->d_dc;
    if (d_tri_cell) *d_tri_cell = c->d_dcCell;
    *num_tris = c->dcTris;
    return RTO_OK;
}

int rto_download_dual_contour(rto_context* c, float* tris, int64_t capacity, int32_t* tri_cell, int64_t* num_tris) {
    if (!c || !num_tris) return RTO_E_INVALID;
    if (c->dcTris < 0) return fail(c, RTO_E_INVALID, "rto_download_dual_contour: no dual-contour list extracted");
    *num_tris = c->dcTris;
    if (!tris && !tri_cell) return RTO_OK;
    if (capacity < c->dcTris) return fail(c, RTO_E_INVALID, "rto_download_dual_contour: capacity too small");
    if (c->dcTris == 0) return RTO_OK;
    RTO_HIP(c, hipSetDevice(c->device));
    RTO_HIP(c, hipStreamSynchronize(c->stream));
    if (tris) RTO_HIP(c, hipMemcpy(tris, c->d_dc, (size_t)c->dcTris * 12 * sizeof(float), hipMemcpyDeviceToHost));
    if (tri_cell) RTO_HIP(c, hipMemcpy(tri_cell, c->d_dcCell, (size_t)c->dcTris * sizeof(int), hipMemcpyDeviceToHost));
    return RTO_OK;
}

int rto_last_dual_contour_ms(const rto_context* c, float ms[3]) { return copy_last_ms(c, &rto_context::dcMs, ms); }

int rto_query_dual_vertices_device(rto_context* c, const int64_t* d_voxels, int64_t n, rto_dual_vertex* d_out) {
    if (!c) return RTO_E_INVALID;
    const int rc = dc_query_check(c, "rto_query_dual_vertices_device", d_voxels, n, d_out);
    if (rc != RTO_OK || n == 0) return rc;
    RTO_HIP(c, hipSetDevice(c->device));
    const int rl = dc_query_launch(c, d_voxels, n, d_out);
    if (rl != RTO_OK) return rl;
    RTO_HIP(c, hipStreamSynchronize(c->stream));
    return RTO_OK;
}

int rto_query_dual_vertices_host(rto_context* c, const int64_t* voxels, int64_t n, rto_dual_vertex* out) {
    if (!c) return RTO_E_INVALID;
    const int rc = dc_query_check(c, "rto_query_dual_vertices_host", voxels, n, out);
    if (rc != RTO_OK || n == 0) return rc;
    RTO_HIP(c, hipSetDevice(c->device));
    BuildScratch scratch(c->stream);
    int64_t* d_voxels = nullptr;
    rto_dual_vertex* d_out = nullptr;
    RTO_HIP(c, scratch.alloc(&d_voxels, (size_t)n));
    RTO_HIP(c, scratch.alloc(&d_out, (size_t)n));
    RTO_HIP(c, hipMemcpyAsync(d_voxels, voxels, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    const int rl = dc_query_launch(c, d_voxels, n, d_out);
    if (rl != RTO_OK) return rl;
    RTO_HIP(c, hipMemcpyAsync(out, d_out, (size_t)n * sizeof(rto_dual_vertex), hipMemcpyDeviceToHost, c->stream));
    RTO_HIP(c, hipStreamSynchronize(c->stream));
    return RTO_OK;
}

}  // extern "C"
