// rto_region.inc -- region queries (include/rto_hip.h, rto_query_points_*, rto_query_regions_*, rto_query_nearest_*): which leaf
// holds a point, how much solid a brush covers, how far the nearest solid is.  Included at the end of rto_api.hip, after
// rto_query.inc (whose entry shape it shares) and rto_edit.inc (whose quantisation it shares).
//
// Rule (DESIGN.md section 17), exact in integers at 1/64 voxel.  pq = floor((p - gridMin) / voxelSize * 64 + 0.5) in double, one
// IEEE operation per operator (the build has -ffp-contract=off; double division and floor are correctly rounded on the device), so
// the device's pq is the host's (rto_point_quantize, rto_brush_quantize).  Voxel i = pq >> 6.  Voxel i is covered by a brush when D[a]
// = 64 (2 i[a] + 1) - 2 cq[a] satisfies sum D^2 <= (2 eq0)^2 (SPHERE) or |D[a]| <= 2 eq[a] (BOX).  A solid leaf's closed box in
// 1/64 units is [64 x, 64 (x + size)].  The walks start at node 0, descend through isLeaf == 0 && isUniform == 0 and read the
// 60-byte array, so every resident octree is served by the same kernels; they never look at the frustum state.
//
// Widths.  Every voxel index a census looks at lies inside the brush's own bounding box, |i| <= 2^22, and |cq| <= 2^27, so D fits
// int32 and D^2 is ONE 32 x 32 -> 64 multiply (v_mad_i64_i32), not a 64 x 64 one (four 32-bit multiplies); the BOX rule needs no
// product at all (an interval per axis).  Only the per-row remainder r^2 - Dy^2 - Dz^2 and the square root's correction are int64.

namespace rto {

constexpr double kRegionLimit = 134217728.0;            // 2^27 sixty-fourths = 2^21 voxels: |pq|, |cq|, eq
constexpr double kNearestLimit = 268435456.0;           // 2^28: mq
constexpr int kRegionBlock = kWave;                      // one wave per workgroup in all three kernels

// What the kernels know of the context.  dom: the domain per axis, [lo, hi); domFromRoot: it is node 0's cube, read in the kernel.
struct RegionGeo {
    double g[3], vs;
    int domLo[3], domHi[3];
    int domFromRoot;
    int gridOk;              // gridMin finite, voxelSize finite and positive: otherwise every record is invalid
    int stackCap;            // entries of the LDS stack (per lane: points, nearest; per wave: census)
};

__device__ __forceinline__ bool region_internal(const rto_node& nd) { return nd.isLeaf == 0 && nd.isUniform == 0; }

// floor(v / vs * 64 + 0.5) of one coordinate difference or length; false when it is not a finite number within `limit`.
__device__ __forceinline__ bool region_quant(double v, double vs, double limit, bool nonNegative, long long& q) {
    const double a = v / vs;
    const double b = a * 64.0;
    const double f = floor(b + 0.5);
    const bool ok = nonNegative ? (f <= limit && v >= 0.0) : (fabs(f) <= limit);     // NaN fails both
    q = ok ? (long long)f : 0;
    return ok;
}

__device__ __forceinline__ bool region_point(const RegionGeo& G, float x, float y, float z, long long pq[3]) {
    const double p[3] = { (double)x, (double)y, (double)z };
    bool ok = G.gridOk != 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double rel = p[a] - G.g[a];
        ok = region_quant(rel, G.vs, kRegionLimit, false, pq[a]) && ok && __builtin_isfinite(p[a]);
    }
    return ok;
}

__device__ __forceinline__ void region_domain(const RegionGeo& G, const rto_node* __restrict__ nodes, long long lo[3], long long hi[3]) {
    if (G.domFromRoot) {
        const rto_node r = nodes[0];
        lo[0] = r.x; lo[1] = r.y; lo[2] = r.z;
        hi[0] = (long long)r.x + r.size; hi[1] = (long long)r.y + r.size; hi[2] = (long long)r.z + r.size;
    } else {
#pragma unroll
        for (int a = 0; a < 3; a++) { lo[a] = G.domLo[a]; hi[a] = G.domHi[a]; }
    }
}

__device__ __forceinline__ int region_log2(int v) { return v > 0 ? 31 - __builtin_clz((unsigned)v) : 0; }

// ================================================================ point location: one point per lane
// A LIFO walk over the 60-byte nodes with the stack in LDS, [entry][lane], as k_query_nodes keeps it.  Only a node whose box holds
// the voxel pushes its children, in slot order 0 .. 7: a subset of the walk rto_upload_octree bounds (walk_stack_need), hence at most
// 7 depth + 1 entries on a canonical tree and kStackCap on any accepted array.  On an octree one child per level holds the voxel.
__global__ __launch_bounds__(kRegionBlock) void k_region_points(RegionGeo G, const float* __restrict__ pts, rto_point_hit* __restrict__ out,
                                                                int64_t n, int64_t base, const rto_node* __restrict__ nodes) {
    extern __shared__ int lds_region_stack[];                    // [stackCap][lane]
    int* stack = lds_region_stack + threadIdx.x;
    const int64_t i = base + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    long long pq[3];
    int best = 0x7fffffff, bs = 0, bx = 0, by = 0, bz = 0, bsolid = 0;
    if (region_point(G, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], pq)) {
        const long long v0 = pq[0] >> 6, v1 = pq[1] >> 6, v2 = pq[2] >> 6;
        int sp = 0;
        stack[kWave * sp++] = 0;
        while (sp > 0) {
            const int idx = stack[kWave * --sp];
            const rto_node nd = nodes[idx];
            const bool in = v0 >= nd.x && v0 < (long long)nd.x + nd.size && v1 >= nd.y && v1 < (long long)nd.y + nd.size &&
                            v2 >= nd.z && v2 < (long long)nd.z + nd.size;
            if (!in) continue;
            if (!region_internal(nd)) {
                if (idx < best) { best = idx; bs = nd.size; bx = nd.x; by = nd.y; bz = nd.z; bsolid = nd.isSolid == 1 ? 1 : 0; }
                continue;
            }
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const int ch = nd.child[c];
                if (ch >= 0) stack[kWave * sp++] = ch;
            }
        }
    }
    int4* dst = reinterpret_cast<int4*>(out) + 2 * i;
    if (best != 0x7fffffff) {
        const int depth = region_log2(nodes[0].size) - region_log2(bs);
        dst[0] = make_int4(best, bsolid, bx, by);
        dst[1] = make_int4(bz, bs, depth, 0);
    } else {
        dst[0] = make_int4(-1, 0, 0, 0);
        dst[1] = make_int4(0, 0, 0, 0);
    }
}

// ================================================================ nearest solid: one point per lane
// The same walk, pruned: a popped node whose closed box is farther than the best so far (at the start: mq^2) is dropped.  The bound
// of an internal node is the distance to its own box, never larger than a descendant's, and only a STRICTLY greater bound drops a
// subtree, so every leaf at the least distance is seen and the lowest index among them wins whatever the order.  Children are pushed
// unpruned in slot order (the test comes at the pop): the stack bound is the point walk's.
__global__ __launch_bounds__(kRegionBlock) void k_region_nearest(RegionGeo G, const rto_near_point* __restrict__ pts, rto_nearest* __restrict__ out,
                                                                 int64_t n, int64_t base, const rto_node* __restrict__ nodes) {
    extern __shared__ int lds_region_stack[];                    // [stackCap][lane]
    int* stack = lds_region_stack + threadIdx.x;
    const int64_t i = base + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 p = reinterpret_cast<const float4*>(pts)[i];
    long long pq[3], mq = 0;
    bool ok = region_point(G, p.x, p.y, p.z, pq);
    long long best2 = 0x7fffffffffffffffll;                       // +inf: no limit
    if (__builtin_isinf(p.w) && p.w > 0.0f) {
    } else {
        ok = region_quant((double)p.w, G.vs, kNearestLimit, true, mq) && ok;
        best2 = mq * mq;
    }
    int bnode = -1, bs = 0;
    long long c0 = 0, c1 = 0, c2 = 0;
    if (ok) {
        int sp = 0;
        stack[kWave * sp++] = 0;
        while (sp > 0) {
            const int idx = stack[kWave * --sp];
            const rto_node nd = nodes[idx];
            const long long ext = 64ll * nd.size;
            const long long lx = 64ll * nd.x, ly = 64ll * nd.y, lz = 64ll * nd.z;
            const long long qx = min(max(pq[0], lx), lx + ext), qy = min(max(pq[1], ly), ly + ext), qz = min(max(pq[2], lz), lz + ext);
            const long long dx = pq[0] - qx, dy = pq[1] - qy, dz = pq[2] - qz;
            // a box out of int64's reach (an uploaded array with absurd coordinates) is farther than any limit: saturate per axis
            const long long kFar = 1ll << 30;
            const bool far = dx > kFar || dx < -kFar || dy > kFar || dy < -kFar || dz > kFar || dz < -kFar;
            const long long d2 = far ? 0x7fffffffffffffffll : dx * dx + dy * dy + dz * dz;
            if (d2 > best2 || far) continue;
            if (!region_internal(nd)) {
                const bool take = nd.isSolid == 1 && (d2 < best2 || bnode < 0 || idx < bnode);
                if (take) { best2 = d2; bnode = idx; bs = nd.size; c0 = qx; c1 = qy; c2 = qz; }
                continue;
            }
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const int ch = nd.child[c];
                if (ch >= 0) stack[kWave * sp++] = ch;
            }
        }
    }
    int4* dst = reinterpret_cast<int4*>(out) + 2 * i;
    if (bnode >= 0) {
        dst[0] = make_int4((int)(unsigned)(unsigned long long)best2, (int)(unsigned)((unsigned long long)best2 >> 32), bnode, bs);
        dst[1] = make_int4((int)c0, (int)c1, (int)c2, 0);
    } else {
        dst[0] = make_int4(-1, -1, -1, 0);
        dst[1] = make_int4(0, 0, 0, 0);
    }
}

// ================================================================ brush census: one wave per region
// The quantised brush of the wave.  blo / bhi: the voxels its bounding box holds, clipped to the domain, inclusive.
struct Census {
    long long r2;            // SPHERE: (2 eq0)^2
    int cq2[3];              // 2 cq: |.| <= 2^28
    int blo[3], bhi[3];
    int sphere;
};

__device__ __forceinline__ long long census_sq(int d) { return (long long)d * (long long)d; }     // one 32 x 32 -> 64 multiply

// floor(sqrt(v)), v >= 0: the double root, then corrected in integers (so its rounding never matters).
__device__ __forceinline__ long long census_isqrt(long long v) {
    long long s = (long long)sqrt((double)v);
    while (s * s > v) s--;
    while ((s + 1) * (s + 1) <= v) s++;
    return s;
}

// Covered voxels of the SPHERE inside the voxel box [lo, hi] (inclusive, inside the brush's bounding box), rows start, start + stride,
// ... of its (y, z) rows, row r at y = lo1 + r % ny, z = lo2 + r / ny, kept without a division.  A row holds the voxels with
// D0^2 <= rem = r^2 - D1^2 - D2^2, i.e. |128 i + 64 - 2 cq0| <= floor(sqrt(rem)): an interval, clipped to [lo0, hi0].
__device__ __forceinline__ long long census_rows(const Census& B, const int lo[3], const int hi[3], int start, int stride) {
    const int ny = hi[1] - lo[1] + 1, nz = hi[2] - lo[2] + 1;
    const int qs = stride / ny, rs = stride % ny;
    int y = lo[1] + start % ny, z = lo[2] + start / ny;
    const int zEnd = lo[2] + nz;
    long long count = 0;
    const long long k = (long long)B.cq2[0] - 64;
    while (z < zEnd) {
        const int Dy = 128 * y + 64 - B.cq2[1], Dz = 128 * z + 64 - B.cq2[2];
        const long long rem = B.r2 - census_sq(Dy) - census_sq(Dz);
        if (rem >= 0) {
            const long long s = census_isqrt(rem);
            const long long a = max((k - s + 127) >> 7, (long long)lo[0]), e = min((k + s) >> 7, (long long)hi[0]);
            count += e >= a ? e - a + 1 : 0;
        }
        y += rs; z += qs;
        if (y > hi[1]) { y -= ny; z++; }
    }
    return count;
}

// The squared distances, in D units, from the brush centre to the nearest and the farthest voxel centre of the box [lo, hi].
__device__ __forceinline__ void census_near_far(const Census& B, const int lo[3], const int hi[3], long long& near2, long long& far2) {
    near2 = 0; far2 = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int Dlo = 128 * lo[a] + 64 - B.cq2[a], Dhi = 128 * hi[a] + 64 - B.cq2[a];
        // D steps by 128 and is even: where the range straddles the centre the least |D| is that of the voxel nearest to it
        int nr;
        if (Dlo >= 0) nr = Dlo;
        else if (Dhi <= 0) nr = -Dhi;
        else { const int m = ((-Dlo) & 127); nr = min(m, 128 - m); }
        const int fr = max(Dlo < 0 ? -Dlo : Dlo, Dhi < 0 ? -Dhi : Dhi);
        near2 += census_sq(nr); far2 += census_sq(fr);
    }
}

constexpr int kCensusOwnRows = 8;       // a partly covered leaf with at most this many rows is counted by its own lane

// One wave per region.  The 64 lanes share one LDS stack of internal nodes.  A step pops up to POPS nodes from the top and gives
// each of their 8 children a lane (POPS = 8: all 64 lanes; POPS = 1: lanes 0 .. 7).  A lane clips its child's box to the domain and
// to the brush's bounding box (I), then:
//   I empty, or SPHERE and the nearest voxel of I is outside               the child is dropped;
//   an internal child                                                      is pushed (lanes in order, by a ballot's prefix count);
//   a solid leaf, BOX                                                      counts the volume of I (the interval product);
//   a solid leaf, SPHERE, the farthest voxel of I inside                   counts the volume of I (covered whole);
//   a solid leaf, SPHERE, otherwise                                        counts I's rows (census_rows): its own lane when they are
//                                                                          few, else the rows are dealt to the 64 lanes.
// `covered` is the same count applied to the domain's box.  Counts stay in the lanes and are reduced once, by shuffles, at the end:
// no atomics.  Stack bound.  POPS = 8 (canonical trees): popped parents keep their stack order and lanes push in lane order, so the
// stack stays sorted by level, deepest on top; a step pops all nodes of the levels above the shallowest one it touches, so afterwards
// every level holds at most the 8 x 8 children of one step: 64 (depth - 1) + 1 entries at most (internal nodes live on levels 0 ..
// depth - 1, the root alone on level 0); 64 depth + 1 are provided.  POPS = 1 (any other array): the LIFO walk in slot order that
// rto_upload_octree bounds by kStackCap, less the leaves.
template <int POPS>
__global__ __launch_bounds__(kRegionBlock) void k_region_census(RegionGeo G, const rto_brush* __restrict__ brushes, rto_region* __restrict__ out,
                                                                int64_t base, const rto_node* __restrict__ nodes) {
    extern __shared__ int lds_region_stack[];                    // [stackCap], the wave's
    const int lane = (int)threadIdx.x;
    const int64_t i = base + blockIdx.x;
    int4* dst = reinterpret_cast<int4*>(out) + 2 * i;

    // ---- the brush, quantised (wave-uniform)
    const float4* src = reinterpret_cast<const float4*>(brushes) + 2 * i;
    const float4 w0 = src[0], w1 = src[1];                        // centre xyz, extent x | extent yz, shape, op
    const float cen[3] = { w0.x, w0.y, w0.z }, ext[3] = { w0.w, w1.x, w1.y };
    const int shape = __float_as_int(w1.z);
    bool ok = G.gridOk != 0 && (shape == RTO_BRUSH_SPHERE || shape == RTO_BRUSH_BOX);
    long long cq[3], eq[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double c = (double)cen[a];
        const double rel = c - G.g[a];
        ok = region_quant(rel, G.vs, kRegionLimit, false, cq[a]) && ok && __builtin_isfinite(c);
        ok = region_quant((double)ext[a], G.vs, kRegionLimit, true, eq[a]) && ok;
    }
    if (!ok) {
        if (lane == 0) { dst[0] = make_int4(-1, -1, -1, -1); dst[1] = make_int4(0, -1, 0, 0); }
        return;
    }
    long long domLo[3], domHi[3];
    region_domain(G, nodes, domLo, domHi);
    Census B;
    B.sphere = shape == RTO_BRUSH_SPHERE ? 1 : 0;
    B.r2 = (2 * eq[0]) * (2 * eq[0]);
    bool empty = false;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const long long e = B.sphere ? eq[0] : eq[a];
        // voxels i with |64 (2 i + 1) - 2 cq| <= 2 e: cq - e - 32 <= 64 i <= cq + e - 32 (clip_brush), then the domain
        const long long lo = max((cq[a] - e - 32 + 63) >> 6, domLo[a]), hi = min((cq[a] + e - 32) >> 6, domHi[a] - 1);
        empty = empty || lo > hi;
        B.cq2[a] = (int)(2 * cq[a]); B.blo[a] = (int)lo; B.bhi[a] = (int)hi;
    }
    long long filled = 0, covered = 0;
    int leaves = 0, first = 0x7fffffff;

    if (!empty) {
        // ---- covered: the count of the domain's box, which clipped to the bounding box is the bounding box
        {
            const long long vol = (long long)(B.bhi[0] - B.blo[0] + 1) * (B.bhi[1] - B.blo[1] + 1) * (B.bhi[2] - B.blo[2] + 1);
            if (!B.sphere) covered = lane == 0 ? vol : 0;
            else {
                long long near2, far2;
                census_near_far(B, B.blo, B.bhi, near2, far2);
                if (far2 <= B.r2) covered = lane == 0 ? vol : 0;
                else if (near2 <= B.r2) covered = census_rows(B, B.blo, B.bhi, lane, kWave);
            }
        }
        // ---- filled: the walk
        int sp = 0;
        int me = lane == 0 ? 0 : -1;                             // the node this lane looks at in this step
        for (;;) {
            bool push = false, deal = false;
            int lo[3] = { 0, 0, 0 }, hi[3] = { 0, 0, 0 };
            if (me >= 0) {
                const rto_node nd = nodes[me];
                const int nx[3] = { nd.x, nd.y, nd.z };
                bool any = true;
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    lo[a] = (int)max((long long)nx[a], (long long)B.blo[a]);
                    hi[a] = (int)min((long long)nx[a] + nd.size - 1, (long long)B.bhi[a]);
                    any = any && lo[a] <= hi[a];
                }
                const bool internal = region_internal(nd);
                if (any && (internal || nd.isSolid == 1)) {
                    long long near2 = 0, far2 = 0;
                    if (B.sphere) census_near_far(B, lo, hi, near2, far2);
                    if (near2 <= B.r2) {                         // BOX: always (0 <= r2)
                        const long long vol = (long long)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);
                        if (internal) push = true;
                        else if (far2 <= B.r2) { filled += vol; leaves++; first = min(first, me); }
                        else {
                            const long long rows = (long long)(hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);
                            if (rows <= kCensusOwnRows) {
                                const long long cnt = census_rows(B, lo, hi, 0, 1);
                                filled += cnt;
                                if (cnt > 0) { leaves++; first = min(first, me); }
                            } else deal = true;
                        }
                    }
                }
            }
            // partly covered large leaves: one after the other, rows dealt to the lanes
            unsigned long long todo = __builtin_amdgcn_ballot_w64(deal);
            while (todo) {
                const int owner = __builtin_ctzll(todo);
                todo &= todo - 1;
                int l2[3], h2[3];
#pragma unroll
                for (int a = 0; a < 3; a++) { l2[a] = __shfl(lo[a], owner); h2[a] = __shfl(hi[a], owner); }
                const long long cnt = census_rows(B, l2, h2, lane, kWave);
                filled += cnt;
                const bool some = __builtin_amdgcn_ballot_w64(cnt > 0) != 0ull;
                if (some && lane == owner) { leaves++; first = min(first, me); }
            }
            // push the internal children that survive, in lane order
            const unsigned long long pm = __builtin_amdgcn_ballot_w64(push);
            if (push) lds_region_stack[sp + __builtin_popcountll(pm & ((1ull << lane) - 1ull))] = me;
            sp += __builtin_popcountll(pm);
            __syncthreads();
            if (sp == 0) break;
            const int npop = min(sp, POPS);
            const int g = lane >> 3;
            const int parent = g < npop ? lds_region_stack[sp - npop + g] : -1;
            sp -= npop;
            me = parent >= 0 ? nodes[parent].child[lane & 7] : -1;
            __syncthreads();                                     // the entries just read may be overwritten by the next pushes
        }
    }
    // ---- reduce across the wave
    for (int off = kWave / 2; off > 0; off >>= 1) {
        filled += __shfl_xor(filled, off);
        covered += __shfl_xor(covered, off);
        leaves += __shfl_xor(leaves, off);
        first = min(first, __shfl_xor(first, off));
    }
    if (lane == 0) {
        dst[0] = make_int4((int)(unsigned)(unsigned long long)filled, (int)(unsigned)((unsigned long long)filled >> 32),
                           (int)(unsigned)(unsigned long long)covered, (int)(unsigned)((unsigned long long)covered >> 32));
        dst[1] = make_int4(leaves, leaves > 0 ? first : -1, 0, 0);
    }
}

}  // namespace rto

// ---------------------------------------------------------------- host side
constexpr int64_t kRegionChunk = (int64_t)1 << 30;     // workgroups per launch

static rto::RegionGeo region_geo(const rto_context* c) {
    rto::RegionGeo G;
    std::memset(&G, 0, sizeof G);
    for (int a = 0; a < 3; a++) G.g[a] = (double)c->gridMin[a];
    G.vs = (double)c->voxelSize;
    G.gridOk = std::isfinite(G.g[0]) && std::isfinite(G.g[1]) && std::isfinite(G.g[2]) && std::isfinite(G.vs) && G.vs > 0.0 ? 1 : 0;
    G.domFromRoot = c->d_vox ? 0 : 1;
    for (int a = 0; a < 3; a++) { G.domLo[a] = 0; G.domHi[a] = c->voxDim[a]; }
    return G;
}

// A canonical tree's walks hold 7 entries per level and one (the lane stacks) or 64 per level and one (the census); any other array is
// bounded by what rto_upload_octree checked.
static bool region_canonical(const rto_context* c) { return c->canonical && c->numInternal > 0 && c->depth > 0 && c->depth <= kMaxDepth; }
static int region_lane_cap(const rto_context* c) { return region_canonical(c) ? 7 * c->depth + 1 : kStackCap; }

template <class In, class Out>
static int region_aligned(rto_context* c, const char* fn, const In* in, const Out* out) {
    if ((reinterpret_cast<uintptr_t>(in) & 15) || (reinterpret_cast<uintptr_t>(out) & 15))
        return fail(c, RTO_E_INVALID, std::string(fn) + ": the input and output buffers must be 16-byte aligned");
    return RTO_OK;
}

static int region_points(rto_context* c, const float* d_pts, int64_t n, rto_point_hit* d_hits, hipStream_t s) {
    const int rc = region_aligned(c, "rto_query_points", d_pts, d_hits);
    if (rc != RTO_OK) return rc;
    rto::RegionGeo G = region_geo(c);
    G.stackCap = region_lane_cap(c);
    const size_t lds = (size_t)G.stackCap * rto::kRegionBlock * sizeof(int);
    for (int64_t off = 0; off < n; off += kRegionChunk * rto::kRegionBlock) {
        const int64_t m = std::min(n - off, kRegionChunk * rto::kRegionBlock);
        hipLaunchKernelGGL(rto::k_region_points, dim3((unsigned)((m + rto::kRegionBlock - 1) / rto::kRegionBlock)), dim3(rto::kRegionBlock), lds, s,
                           G, d_pts, d_hits, n, off, c->d_nodes);
        RTO_HIP(c, hipGetLastError());
    }
    return RTO_OK;
}

static int region_nearest(rto_context* c, const rto_near_point* d_pts, int64_t n, rto_nearest* d_out, hipStream_t s) {
    const int rc = region_aligned(c, "rto_query_nearest", d_pts, d_out);
    if (rc != RTO_OK) return rc;
    rto::RegionGeo G = region_geo(c);
    G.stackCap = region_lane_cap(c);
    const size_t lds = (size_t)G.stackCap * rto::kRegionBlock * sizeof(int);
    for (int64_t off = 0; off < n; off += kRegionChunk * rto::kRegionBlock) {
        const int64_t m = std::min(n - off, kRegionChunk * rto::kRegionBlock);
        hipLaunchKernelGGL(rto::k_region_nearest, dim3((unsigned)((m + rto::kRegionBlock - 1) / rto::kRegionBlock)), dim3(rto::kRegionBlock), lds, s,
                           G, d_pts, d_out, n, off, c->d_nodes);
        RTO_HIP(c, hipGetLastError());
    }
    return RTO_OK;
}

static int region_census(rto_context* c, const rto_brush* d_brushes, int64_t n, rto_region* d_out, hipStream_t s) {
    const int rc = region_aligned(c, "rto_query_regions", d_brushes, d_out);
    if (rc != RTO_OK) return rc;
    rto::RegionGeo G = region_geo(c);
    const bool canon = region_canonical(c);
    G.stackCap = canon ? 64 * c->depth + 1 : kStackCap;
    const size_t lds = (size_t)G.stackCap * sizeof(int);
    for (int64_t off = 0; off < n; off += kRegionChunk) {
        const dim3 grid((unsigned)std::min(n - off, kRegionChunk));
        if (canon) hipLaunchKernelGGL(rto::k_region_census<8>, grid, dim3(rto::kRegionBlock), lds, s, G, d_brushes, d_out, off, c->d_nodes);
        else hipLaunchKernelGGL(rto::k_region_census<1>, grid, dim3(rto::kRegionBlock), lds, s, G, d_brushes, d_out, off, c->d_nodes);
        RTO_HIP(c, hipGetLastError());
    }
    return RTO_OK;
}

// The points of the location query are 12-byte records: query_entry stages n elements of its In type, so the host form hands it
// the three floats of a point as one element.
struct RegionPoint3 { float x, y, z; };

extern "C" {

int rto_point_quantize(const float p[3], const float grid_min[3], float voxel_size, int64_t pq[3]) {
    if (!p || !grid_min || !pq) return RTO_E_INVALID;
    const double vs = (double)voxel_size;
    if (!std::isfinite(vs) || !(vs > 0.0)) return RTO_E_INVALID;
    long long q[3];
    for (int a = 0; a < 3; a++) {
        const double c = (double)p[a], g = (double)grid_min[a];
        if (!std::isfinite(c) || !std::isfinite(g)) return RTO_E_INVALID;
        const double rel = c - g;                  // one IEEE operation per statement, as quantize_brush
        const double vc = rel / vs;
        const double sc = vc * 64.0;
        const double fc = std::floor(sc + 0.5);
        if (!(std::fabs(fc) <= rto::kRegionLimit)) return RTO_E_INVALID;
        q[a] = (long long)fc;
    }
    for (int a = 0; a < 3; a++) pq[a] = q[a];
    return RTO_OK;
}

int rto_query_points_device(rto_context* c, const float* d_points, int64_t n, rto_point_hit* d_hits, void* hip_stream) {
    return query_entry(c, "rto_query_points_device", RTO_QUERY_FIRST, false, nullptr, false, reinterpret_cast<const RegionPoint3*>(d_points), n, d_hits,
                       false, hip_stream, [=](const RegionPoint3* p, rto_point_hit* h, hipStream_t s) {
                           return region_points(c, reinterpret_cast<const float*>(p), n, h, s); });
}

int rto_query_points_host(rto_context* c, const float* points, int64_t n, rto_point_hit* hits) {
    return query_entry(c, "rto_query_points_host", RTO_QUERY_FIRST, false, nullptr, false, reinterpret_cast<const RegionPoint3*>(points), n, hits,
                       true, nullptr, [=](const RegionPoint3* p, rto_point_hit* h, hipStream_t s) {
                           return region_points(c, reinterpret_cast<const float*>(p), n, h, s); });
}

int rto_query_regions_device(rto_context* c, const rto_brush* d_brushes, int64_t n, rto_region* d_regions, void* hip_stream) {
    return query_entry(c, "rto_query_regions_device", RTO_QUERY_FIRST, false, nullptr, false, d_brushes, n, d_regions, false, hip_stream,
                       [=](const rto_brush* b, rto_region* o, hipStream_t s) { return region_census(c, b, n, o, s); });
}

int rto_query_regions_host(rto_context* c, const rto_brush* brushes, int64_t n, rto_region* regions) {
    return query_entry(c, "rto_query_regions_host", RTO_QUERY_FIRST, false, nullptr, false, brushes, n, regions, true, nullptr,
                       [=](const rto_brush* b, rto_region* o, hipStream_t s) { return region_census(c, b, n, o, s); });
}

int rto_query_nearest_device(rto_context* c, const rto_near_point* d_points, int64_t n, rto_nearest* d_out, void* hip_stream) {
    return query_entry(c, "rto_query_nearest_device", RTO_QUERY_FIRST, false, nullptr, false, d_points, n, d_out, false, hip_stream,
                       [=](const rto_near_point* p, rto_nearest* o, hipStream_t s) { return region_nearest(c, p, n, o, s); });
}

int rto_query_nearest_host(rto_context* c, const rto_near_point* points, int64_t n, rto_nearest* out) {
    return query_entry(c, "rto_query_nearest_host", RTO_QUERY_FIRST, false, nullptr, false, points, n, out, true, nullptr,
                       [=](const rto_near_point* p, rto_nearest* o, hipStream_t s) { return region_nearest(c, p, n, o, s); });
}

}  // extern "C"
