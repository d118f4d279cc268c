// rto_query.inc -- ray queries (include/rto_hip.h, rto_query_*): caller-supplied rays, or the renders' own pixel rays, traced
// through the whole resident octree; one rto_hit record per ray.  Included at the end of rto_api.hip.
//
// Acceptance rule (DESIGN.md section 10).  t_lo = max(t_min, 0), t_hi = min(t_max, largest float below 1e30).  A solid leaf is
// accepted when its own box and every ancestor's pass the reference's slab test (S/RT:226-236: tNear <= tFar && tFar > 0, glm
// min / max, the renders' operation order) with tNear < 1e30 (the renders' `tNear >= closestT` prune at its start value,
// S/RT:242), and tHit = max(t_lo, tNear) satisfies tHit <= tFar and tHit <= t_hi.  With (0, 1e30) this is the renders' rule.
//   FIRST   the first accepted leaf in the reference's LIFO pop order (children 7 .. 0), under its 512-pop cap (rto_render_device);
//   CLOSEST the accepted leaf of least tHit, ties to the leaf popped first (rto_render_closest_device);
//   ANY     some accepted leaf (occlusion): a hit exactly when CLOSEST has one.
// The walks ignore the frustum state: the descriptors' visibility bits are masked off and d_compact is never read.

namespace rto {

constexpr int kQueryFirst = RTO_QUERY_FIRST, kQueryClosest = RTO_QUERY_CLOSEST, kQueryAny = RTO_QUERY_ANY;

// Where the rays come from: rays[base + i] (PIXELS = false: 32-byte rto_ray records, 16-byte aligned) or the pixel
// (xy[2 (base + i)], xy[2 (base + i) + 1]) of the frame in RenderParams (PIXELS = true, generate_ray_tab).
struct QuerySrc {
    const rto_ray* rays;
    const int32_t* xy;
    rto_hit* hits;           // 16-byte aligned
    int64_t n;               // rays of the whole call
    int64_t base;            // first ray of this launch
};

// The ray of query i and its window; false: the ray is a miss whatever the tree (NaN input, t_min > t_max, pixel outside the frame).
template <bool PIXELS>
__device__ __forceinline__ bool query_ray(const RenderParams& P, const QuerySrc& Q, int64_t i, Ray& r, float& tlo, float& thi) {
    const float kBelow1e30 = __uint_as_float(0x7149f2c9u);
    if (PIXELS) {
        const int px = Q.xy[2 * i], py = Q.xy[2 * i + 1];
        if (px < 0 || px >= P.W || py < 0 || py >= P.H) return false;
        r = generate_ray_tab(P, px, py);
        tlo = 0.0f; thi = kBelow1e30;
        return true;
    }
    const float4* src = reinterpret_cast<const float4*>(Q.rays) + 2 * i;
    const float4 a = src[0], b = src[1];
    r.ox = a.x; r.oy = a.y; r.oz = a.z; r.dx = b.x; r.dy = b.y; r.dz = b.z;
    if (__builtin_isnan(a.x) || __builtin_isnan(a.y) || __builtin_isnan(a.z) || __builtin_isnan(b.x) || __builtin_isnan(b.y) ||
        __builtin_isnan(b.z) || !(a.w <= b.w))                      // NaN t_min / t_max or t_min > t_max
        return false;
    r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
    tlo = a.w > 0.0f ? a.w : 0.0f;
    thi = gmin(b.w, kBelow1e30);
    return true;
}

// Entry face of an accepted leaf: the lowest axis whose entry parameter min(t1, t2) is tNear, signed by the direction; -1 when
// tHit > tNear (the window or the origin clipped the entry).  The slab arithmetic of slab_exact.
__device__ __forceinline__ int query_face(const Geo& G, const Ray& r, int x, int y, int z, int size, float tHit) {
    const float ext = (float)size * G.vs;
    const float mnx = G.gx + (float)x * G.vs, mny = G.gy + (float)y * G.vs, mnz = G.gz + (float)z * G.vs;
    const float ex = gmin((mnx - r.ox) * r.ix, ((mnx + ext) - r.ox) * r.ix);
    const float ey = gmin((mny - r.oy) * r.iy, ((mny + ext) - r.oy) * r.iy);
    const float ez = gmin((mnz - r.oz) * r.iz, ((mnz + ext) - r.oz) * r.iz);
    const float tNear = gmax(gmax(ex, ey), ez);
    if (tHit > tNear) return -1;
    if (ex == tNear) return r.dx < 0.0f ? 1 : 0;
    if (ey == tNear) return r.dy < 0.0f ? 3 : 2;
    return r.dz < 0.0f ? 5 : 4;
}

__device__ __forceinline__ void store_hit(const QuerySrc& Q, int64_t i, bool hit, float t, int node, int face, int size, int x, int y, int z) {
    int4* dst = reinterpret_cast<int4*>(Q.hits) + 2 * i;
    if (hit) {
        dst[0] = make_int4(__float_as_int(t), node, face, size);
        dst[1] = make_int4(x, y, z, 0);
    } else {
        dst[0] = make_int4(__float_as_int(1e30f), -1, -1, 0);
        dst[1] = make_int4(0, 0, 0, 0);
    }
}

// ================================================================ canonical trees: the descriptor walk
// One ray per lane.  Per tree level and lane two LDS words: the entry the lean kernels keep (children still to pop | internal
// mask << 8, first internal child's descriptor) and the descriptor index of the node itself (a leaf's array index is
// descFirstChild[that] + child).  The 8 child verdicts of an entered node come at once from child_fail_mask_fast (waves holding a
// non-finite origin, direction or reciprocal: child_fail_mask_exact); the visibility byte of the descriptor is never looked at.
//   FIRST   children pop 7 .. 0 as in the reference.  Every entered internal node pushes its 8 children and everything pushed is
//           popped except, at a leaf, the children below the path on each level: pops = 1 + 8 entered - sum of the path's child
//           indices, and that sum is popcount(x) + 2 popcount(y) + 4 popcount(z) of the leaf's position (the path's bits).  A hit
//           past 512 pops is a miss (the render's loop ended first); past 8 entered > 511 + 7 depth no later hit can be in reach.
//   CLOSEST the ray's own octant first (k_closest_near_first's order); ANY the same order, ends at the first accepted leaf.
// desc_walk is that walk for one lane.  What a query kind adds is its leaf rule:
//   kPrune      may a box be cut by t?  Then the root, the child verdicts' far clamp and every popped box (internal ones too) are
//               held against min(closest(), t_hi) -- a child's tNear is never below its parent's; otherwise only leaves are slab-
//               tested at the pop, at the default clamps;
//   leaves(d.x) the leaf children of a descriptor that can hold a hit;
//   closest()   the t a pruning rule holds boxes against (the best hit so far);
//   leaf(..)    a popped leaf whose box passed: true when it holds an accepted hit, which the rule has then recorded;
//   kEveryLeaf  the rule wants every accepted leaf of the ray: the walk goes on past a hit in any mode, as CLOSEST does.
// BoxRule is the box queries' (the lit render's too), TriRule (rto_tri_query.inc) the triangle queries', SpanRule (rto_span.inc)
// the span queries'.

// The two LDS stacks of the calling lane: `levels` entries of each per lane, [wave][level][lane].
__device__ __forceinline__ void desc_stacks(uint2* lds, int levels, uint2*& stk, unsigned*& stkNode) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = (int)(blockDim.x >> 6);
    stk = lds + (size_t)wave * levels * kWave + lane;
    stkNode = reinterpret_cast<unsigned*>(lds + (size_t)waves * levels * kWave) + (size_t)wave * levels * kWave + lane;
}

// Their dynamic LDS for a workgroup of kBlock: 12 bytes per wave, level and lane, 61,440 B at depth 20.
static size_t desc_stack_bytes(int levels) { return (size_t)(kBlock / kWave) * levels * kWave * (sizeof(uint2) + sizeof(unsigned)); }

// What a box walk found: the accepted leaf's position and size, tHit, its child slot j in the parent whose descriptor index is
// `node` (the leaf's array index is descFirstChild[node] + j).
struct DescHit {
    bool hit;
    float t;
    int x, y, z, size, j;
    unsigned node;
};

// Solid leaves; tHit = max(t_lo, tNear) is the box's own, so CLOSEST and ANY cut every box past the best hit or the window.
template <int QMODE>
struct BoxRule {
    static constexpr bool kPrune = QMODE != kQueryFirst;
    static constexpr bool kEveryLeaf = false;
    DescHit best;
    __device__ __forceinline__ BoxRule() { best.hit = false; best.t = 1e30f; best.x = best.y = best.z = best.size = best.j = 0; best.node = 0; }
    __device__ __forceinline__ static unsigned leaves(unsigned dx) { return dx & 0xffu; }
    __device__ __forceinline__ float closest() const { return best.t; }
    // CLOSEST in the octant order: equal tHit goes to the leaf the reference's LIFO order pops first (pops_before)
    __device__ __forceinline__ bool leaf(const Ray&, float tlo, float thi, float tNear, float tFar, int x, int y, int z, int size, int j,
                                              const unsigned* node) {
        const float tHit = gmax(tlo, tNear);
        bool take = tHit <= tFar && tHit <= thi;
        if (QMODE == kQueryClosest) {
            // plain booleans, as in k_closest_near_first (a short-circuit form lost updates in this divergent loop there)
            const bool nearer = tHit < best.t;
            const bool tie = tHit == best.t;                       // only after a hit: best.t starts at 1e30 > t_hi
            const bool first = pops_before(x, y, z, best.x, best.y, best.z);
            take = take && (nearer || (tie && first));
        }
        if (take) { best.t = tHit; best.x = x; best.y = y; best.z = z; best.size = size; best.j = j; best.node = *node; }
        return take;
    }
};

// The walk of one ray (r, window [tlo, thi]) in mode QMODE under leaf rule R; true: R holds the hit.  Called by every lane of the
// wave together (the risky-ray vote is a wave ballot); `valid` false: the lane takes no part and gets a miss.
template <int QMODE, class Rule>
__device__ __forceinline__ bool desc_walk(const RenderParams& P, const Geo& G, const Ray r, float tlo, float thi, bool valid,
                                          const uint2* __restrict__ desc, uint2* stk, unsigned* stkNode, Rule& R) {
    const float kEps = __uint_as_float(1u), kBelow1e30 = __uint_as_float(0x7149f2c9u);
    bool active = false;
    if (valid) {
        float tNear, tFar, a0, a1, a2, a3, a4, a5;
        active = slab_exact(G, r, 0, 0, 0, P.rootSize, tNear, tFar, a0, a1, a2, a3, a4, a5) && !(tNear >= 1e30f);
        if (Rule::kPrune) active = active && !(tNear > thi);
    }
    const bool risky = active && !(__builtin_isfinite(r.ix) && __builtin_isfinite(r.iy) && __builtin_isfinite(r.iz) &&
                                   __builtin_isfinite(r.ox) && __builtin_isfinite(r.oy) && __builtin_isfinite(r.oz) &&
                                   __builtin_isfinite(r.dx) && __builtin_isfinite(r.dy) && __builtin_isfinite(r.dz));
    const bool anyRisky = __builtin_amdgcn_ballot_w64(risky) != 0ull;
    const unsigned sgnX = (unsigned)((int)__float_as_uint(r.ix) >> 31), sgnY = (unsigned)((int)__float_as_uint(r.iy) >> 31),
                   sgnZ = (unsigned)((int)__float_as_uint(r.iz) >> 31);
    const unsigned flip = QMODE == kQueryFirst ? 0u : ((r.dx < 0.0f ? 1u : 0u) | (r.dy < 0.0f ? 2u : 0u) | (r.dz < 0.0f ? 4u : 0u));

    bool hit = false, enter = active;
    unsigned cur = 0, lvlPending = 0;
    int cx = 0, cy = 0, cz = 0, bpos = P.depth - 1;
    int entered = 0;
    const int capEntered = kMaxTraversalSteps - 1 + 7 * P.depth;      // FIRST: 8 entered above this puts every later hit past the cap
    while (active) {
        if (enter) {
            entered++;
            if (QMODE == kQueryFirst && 8 * entered > capEntered) break;
            const uint2 d = desc[cur];
            unsigned fail8;
            if (anyRisky) fail8 = child_fail_mask_exact(G.gx, G.gy, G.gz, G.vs, r.ox, r.oy, r.oz, r.ix, r.iy, r.iz, cx, cy, cz, 1 << bpos);
            else fail8 = child_fail_mask_fast<true, false>(G.gx, G.gy, G.gz, G.vs, r.ox, r.oy, r.oz, r.ix, r.iy, r.iz, sgnX, sgnY, sgnZ,
                                                           cx, cy, cz, (float)(1 << bpos), kEps,
                                                           Rule::kPrune ? gmax(kEps, gmin(R.closest(), thi)) : kBelow1e30);   // the pop re-tests exactly
            const unsigned im = (d.x >> 8) & 0xffu;
            unsigned cand = ((Rule::leaves(d.x) | im) & 0xffu) & ~fail8;   // candidate leaves and internal children whose box the ray meets
            if (QMODE != kQueryFirst) cand = flip_children(cand, flip);
            stk[bpos * kWave] = make_uint2(cand | (im << 8), d.y);
            stkNode[bpos * kWave] = cur;
            lvlPending = cand ? (lvlPending | (1u << bpos)) : (lvlPending & ~(1u << bpos));
            enter = false;
        }
        if (lvlPending == 0) break;
        const int Lb = __builtin_ctz(lvlPending);                  // the deepest node with children left: LIFO
        const uint2 e = stk[Lb * kWave];
        const int k = QMODE == kQueryFirst ? 31 - __builtin_clz(e.x & 0xffu) : __builtin_ctz(e.x & 0xffu);
        const unsigned left = e.x ^ (1u << k);
        stk[Lb * kWave].x = left;
        if ((left & 0xffu) == 0) lvlPending &= ~(1u << Lb);
        const int j = k ^ (int)flip;
        const unsigned bit = 1u << j;
        const int h = 1 << Lb, keep = ~(2 * h - 1);
        const int chx = (cx & keep) + ((j & 1) ? h : 0), chy = (cy & keep) + ((j & 2) ? h : 0), chz = (cz & keep) + ((j & 4) ? h : 0);
        const unsigned im = (e.x >> 8) & 0xffu;
        const bool internal = (im & bit) != 0;
        float tNear = 0.0f, tFar = 0.0f;
        bool pass = true;
        if (Rule::kPrune || !internal) {
            float a0, a1, a2, a3, a4, a5;
            pass = slab_exact(G, r, chx, chy, chz, h, tNear, tFar, a0, a1, a2, a3, a4, a5) && !(tNear >= 1e30f);
            if (Rule::kPrune) pass = pass && !(tNear > gmin(R.closest(), thi));
        }
        if (!pass) continue;
        if (internal) {
            cur = e.y + (unsigned)__builtin_popcount(im & (bit - 1u));
            cx = chx; cy = chy; cz = chz; bpos = Lb - 1; enter = true;
            continue;
        }
        const bool got = R.leaf(r, tlo, thi, tNear, tFar, chx, chy, chz, h, j, stkNode + Lb * kWave);
        if (QMODE == kQueryClosest || Rule::kEveryLeaf) {
            hit = hit || got;                                      // a plain boolean: got is computed above
        } else if (got) {
            hit = true;
            if (QMODE == kQueryFirst) {
                const int pops = 1 + 8 * entered - (__builtin_popcount(chx) + 2 * __builtin_popcount(chy) + 4 * __builtin_popcount(chz));
                if (pops > kMaxTraversalSteps) hit = false;        // S/RT:254: the loop ended before this pop
            }
            break;
        }
    }
    return hit;
}

// The box walk of one lane, as k_query_desc and the lit render's kernels (rto_lit.inc) ask for it.
template <int QMODE>
__device__ __forceinline__ DescHit box_walk(const RenderParams& P, const Geo& G, const Ray r, float tlo, float thi, bool valid,
                                            const uint2* __restrict__ desc, uint2* stk, unsigned* stkNode) {
    BoxRule<QMODE> R;
    R.best.hit = desc_walk<QMODE>(P, G, r, tlo, thi, valid, desc, stk, stkNode, R);
    return R.best;
}

template <int QMODE, bool PIXELS>
__global__ __launch_bounds__(kBlock) void k_query_desc(RenderParams P, QuerySrc Q, const uint2* __restrict__ desc,
                                                       const int* __restrict__ descFirstChild) {
    extern __shared__ uint2 lds_stack[];   // [wave][level][lane] entries, then [wave][level][lane] descriptor indices
    uint2* stk;
    unsigned* stkNode;
    desc_stacks(lds_stack, P.depth, stk, stkNode);
    const int64_t i = Q.base + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const Geo G = geo_of(P);

    Ray r;
    r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
    float tlo = 0.0f, thi = 0.0f;
    const bool valid = i < Q.n && query_ray<PIXELS>(P, Q, i, r, tlo, thi);
    const DescHit w = box_walk<QMODE>(P, G, r, tlo, thi, valid, desc, stk, stkNode);
    if (i < Q.n) {
        const int node = w.hit ? descFirstChild[w.node] + w.j : -1;
        const int face = w.hit ? query_face(G, r, w.x, w.y, w.z, w.size, w.t) : -1;
        store_hit(Q, i, w.hit, w.t, node, face, w.size, w.x, w.y, w.z);
    }
}

// ================================================================ any array, or RTO_KERNEL_GENERIC: node by node
// The 60-byte array with explicit child indices and a stack of kStackCap entries in the reference's LIFO order.  rto_upload_octree
// bounds every walk that pushes children in slot order 0 .. 7 by it (walk_stack_need); a walk in another order (k_span_nodes) is
// bounded by the any-order need the upload records beside it, which its entries check before they launch.  The stack lives in LDS, [entry][lane] (conflict free), one wave per workgroup (36 KB): a private
// int[kStackCap] would be scratch memory.  FIRST is the loop of k_trace_generic, CLOSEST that of k_trace_closest (a leaf replaces the best only
// when strictly nearer: ties to the leaf popped first), ANY ends at the first accepted leaf; CLOSEST and ANY also cut nodes with
// tNear > t_hi.
constexpr int kQueryNodesBlock = kWave;
template <int QMODE, bool PIXELS>
__global__ __launch_bounds__(kQueryNodesBlock) void k_query_nodes(RenderParams P, QuerySrc Q, const rto_node* __restrict__ nodes) {
    extern __shared__ int lds_query_stack[];                     // [kStackCap][lane]
    int* stack = lds_query_stack + threadIdx.x;
    const int64_t i = Q.base + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const Geo G = geo_of(P);
    Ray r;
    float tlo = 0.0f, thi = 0.0f;
    bool hit = false;
    float closestT = 1e30f;                                        // S/RT:242
    int bnode = -1, bx = 0, by = 0, bz = 0, bs = 0;
    if (i < Q.n && query_ray<PIXELS>(P, Q, i, r, tlo, thi)) {
        int sp = 0, steps = 0;
        stack[kWave * sp++] = 0;
        while (sp > 0 && (QMODE != kQueryFirst || steps < kMaxTraversalSteps)) {
            const int nodeIdx = stack[kWave * --sp];
            steps++;
            const rto_node nd = nodes[nodeIdx];
            float tNear, tFar, a0, a1, a2, a3, a4, a5;
            if (!slab_exact(G, r, nd.x, nd.y, nd.z, nd.size, tNear, tFar, a0, a1, a2, a3, a4, a5)) continue;
            if (tNear >= closestT) continue;
            if (QMODE != kQueryFirst && tNear > thi) continue;
            if (nd.isUniform == 1 || nd.isLeaf == 1) {
                if (nd.isSolid == 1) {
                    const float tHit = gmax(tlo, tNear);
                    if (tHit < closestT && tHit <= tFar && tHit <= thi) {
                        hit = true; closestT = tHit; bnode = nodeIdx; bx = nd.x; by = nd.y; bz = nd.z; bs = nd.size;
                        if (QMODE != kQueryClosest) break;
                    }
                }
                continue;
            }
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const int ch = nd.child[c];
                if (ch >= 0) stack[kWave * sp++] = ch;
            }
        }
    }
    if (i < Q.n) store_hit(Q, i, hit, closestT, bnode, hit ? query_face(G, r, bx, by, bz, bs, closestT) : -1, bs, bx, by, bz);
}

}  // namespace rto

// ---------------------------------------------------------------- host side
constexpr int64_t kQueryChunk = (int64_t)1 << 28;       // rays per launch: 2^20 workgroups of 256 (2^22 of 64)

// Geometry of the resident octree for a launch of rays from memory (the pixel form fills the frame part with fill_params).
static void query_geometry(const rto_context* c, RenderParams& P) {
    std::memcpy(P.gridMin, c->gridMin, sizeof P.gridMin);
    P.voxelSize = c->voxelSize;
    P.rootSize = c->rootSize;
    P.depth = c->depth > 0 ? c->depth : 1;
}

static int query_check(rto_context* c, const char* fn, int mode, int64_t n, const void* in, const void* out) {
    if (mode != RTO_QUERY_FIRST && mode != RTO_QUERY_CLOSEST && mode != RTO_QUERY_ANY)
        return fail(c, RTO_E_INVALID, std::string(fn) + ": unknown mode " + std::to_string(mode));
    if (n < 0) return fail(c, RTO_E_INVALID, std::string(fn) + ": n < 0");
    if (n > 0 && (!in || !out)) return fail(c, RTO_E_INVALID, std::string(fn) + ": NULL buffer");
    return RTO_OK;
}

// The launches of one query call, box or triangle: chunks of kQueryChunk rays, the descriptor kernels (workgroups of kBlock) on a
// canonical tree unless RTO_KERNEL_GENERIC is set, the node kernels (one wave) otherwise.  launch(mode as a compile-time constant,
// desc, grid, block, lds, Q of the chunk) names the family's kernel.
template <class Launch>
static int launch_query(rto_context* c, int mode, int depth, QuerySrc Q, Launch launch) {
    const bool desc = c->canonical && c->numInternal > 0 && c->kernelMode != RTO_KERNEL_GENERIC;
    const int block = desc ? kBlock : kQueryNodesBlock;
    const size_t lds = desc ? desc_stack_bytes(depth) : (size_t)kStackCap * kQueryNodesBlock * sizeof(int);
    for (int64_t off = 0; off < Q.n; off += kQueryChunk) {
        Q.base = off;
        const dim3 grid((unsigned)((std::min(Q.n - off, kQueryChunk) + block - 1) / block));
        if (mode == RTO_QUERY_FIRST) launch(std::integral_constant<int, kQueryFirst>(), desc, grid, dim3(block), lds, Q);
        else if (mode == RTO_QUERY_CLOSEST) launch(std::integral_constant<int, kQueryClosest>(), desc, grid, dim3(block), lds, Q);
        else launch(std::integral_constant<int, kQueryAny>(), desc, grid, dim3(block), lds, Q);
        RTO_HIP(c, hipGetLastError());
    }
    return RTO_OK;
}

template <bool PIXELS>
static int launch_box_query(rto_context* c, int mode, const RenderParams& P, const QuerySrc& Q0, hipStream_t s) {
    return launch_query(c, mode, P.depth, Q0, [&](auto m, bool desc, dim3 grid, dim3 block, size_t lds, const QuerySrc& Q) {
        constexpr int M = decltype(m)::value;
        if (desc) hipLaunchKernelGGL((k_query_desc<M, PIXELS>), grid, block, lds, s, P, Q, c->d_desc, c->d_descFirstChild);
        else hipLaunchKernelGGL((k_query_nodes<M, PIXELS>), grid, block, lds, s, P, Q, c->d_nodes);
    });
}

static int query_rays(rto_context* c, int mode, const rto_ray* d_rays, int64_t n, rto_hit* d_hits, hipStream_t s) {
    if ((reinterpret_cast<uintptr_t>(d_rays) & 15) || (reinterpret_cast<uintptr_t>(d_hits) & 15))
        return fail(c, RTO_E_INVALID, "rto_query_rays: the ray and hit buffers must be 16-byte aligned");
    RenderParams P;
    std::memset(&P, 0, sizeof P);
    query_geometry(c, P);
    return launch_box_query<false>(c, mode, P, QuerySrc{ d_rays, nullptr, d_hits, n, 0 }, s);
}

static int query_pixels(rto_context* c, int mode, const rto_frame* f, const int32_t* d_xy, int64_t n, rto_hit* d_hits, hipStream_t s) {
    if (reinterpret_cast<uintptr_t>(d_hits) & 15) return fail(c, RTO_E_INVALID, "rto_query_pixels: the hit buffer must be 16-byte aligned");
    RenderParams P;
    const int rc = fill_params(c, f, nullptr, P, s);             // the renders' ray tables and inverse view: bit-identical rays
    if (rc != RTO_OK) return rc;
    return launch_box_query<true>(c, mode, P, QuerySrc{ nullptr, d_xy, d_hits, n, 0 }, s);
}

// One entry of the C ABI: `pixels` (xy pairs of `frame`) or rays, `tris` (the leaf triangles must be resident) or boxes.  The checks
// come in the order the ABI promises; n == 0 is RTO_OK whatever is resident.  run(d_in, d_hits, stream) is the device form, called
// on `stream` for a *_device entry; a *_host entry (`host`) stages `in` and the hits through stream-ordered scratch around it on
// the context's stream and waits.
template <class In, class Hit, class Run>
static int query_entry(rto_context* c, const char* fn, int mode, bool pixels, const rto_frame* frame, bool tris, const In* in, int64_t n,
                       Hit* hits, bool host, void* stream, Run run) {
    if (!c) return RTO_E_INVALID;
    int rc = query_check(c, fn, mode, n, in, hits);
    if (rc != RTO_OK || n == 0) return rc;
    if (pixels && !frame) return fail(c, RTO_E_INVALID, std::string(fn) + ": frame is NULL");
    if (tris && (c->numNodes <= 0 || !c->d_triOffset || !c->d_tris))
        return fail(c, RTO_E_NO_OCTREE, std::string(fn) + ": no leaf triangles resident (rto_build_leaf_triangles / rto_upload_leaf_triangles)");
    if (c->numNodes <= 0) return fail(c, RTO_E_NO_OCTREE, std::string(fn) + ": no octree uploaded");
    RTO_HIP(c, hipSetDevice(c->device));
    if (!host) return run(in, hits, (hipStream_t)stream);
    const size_t nIn = (size_t)n * (pixels ? 2 : 1);
    BuildScratch scratch(c->stream);
    In* d_in = nullptr;
    Hit* d_hits = nullptr;
    RTO_HIP(c, scratch.alloc(&d_in, nIn));
    RTO_HIP(c, scratch.alloc(&d_hits, (size_t)n));
    RTO_HIP(c, hipMemcpyAsync(d_in, in, nIn * sizeof(In), hipMemcpyHostToDevice, c->stream));
    if ((rc = run(d_in, d_hits, c->stream)) != RTO_OK) return rc;
    RTO_HIP(c, hipMemcpyAsync(hits, d_hits, (size_t)n * sizeof(Hit), hipMemcpyDeviceToHost, c->stream));
    RTO_HIP(c, hipStreamSynchronize(c->stream));
    return RTO_OK;
}

extern "C" {

int rto_query_rays_device(rto_context* c, int mode, const rto_ray* d_rays, int64_t n, rto_hit* d_hits, void* hip_stream) {
    return query_entry(c, "rto_query_rays_device", mode, false, nullptr, false, d_rays, n, d_hits, false, hip_stream,
                       [=](const rto_ray* r, rto_hit* h, hipStream_t s) { return query_rays(c, mode, r, n, h, s); });
}

int rto_query_rays_host(rto_context* c, int mode, const rto_ray* rays, int64_t n, rto_hit* hits) {
    return query_entry(c, "rto_query_rays_host", mode, false, nullptr, false, rays, n, hits, true, nullptr,
                       [=](const rto_ray* r, rto_hit* h, hipStream_t s) { return query_rays(c, mode, r, n, h, s); });
}

int rto_query_pixels_device(rto_context* c, int mode, const rto_frame* frame, const int32_t* d_xy, int64_t n, rto_hit* d_hits, void* hip_stream) {
    return query_entry(c, "rto_query_pixels_device", mode, true, frame, false, d_xy, n, d_hits, false, hip_stream,
                       [=](const int32_t* xy, rto_hit* h, hipStream_t s) { return query_pixels(c, mode, frame, xy, n, h, s); });
}

int rto_query_pixels_host(rto_context* c, int mode, const rto_frame* frame, const int32_t* xy, int64_t n, rto_hit* hits) {
    return query_entry(c, "rto_query_pixels_host", mode, true, frame, false, xy, n, hits, true, nullptr,
                       [=](const int32_t* d_xy, rto_hit* h, hipStream_t s) { return query_pixels(c, mode, frame, d_xy, n, h, s); });
}

}  // extern "C"
