// rto_tri_query.inc -- triangle queries (include/rto_hip.h, rto_query_triangles_*, rto_query_triangle_pixels_*): caller rays, or
// the renders' own pixel rays, against the resident leaf triangles (config 5's surface); one rto_tri_hit record per ray.  Included
// at the end of rto_api.hip, after rto_query.inc (whose ray sources, QuerySrc / query_ray, it shares).
//
// Acceptance rule (DESIGN.md section 10, "Triangle queries").  A leaf is reachable when its box and every ancestor's pass the
// reference's float32 slab test with tNear < 1e30 -- the triangle render's box rule; no window test on boxes.  A triangle of a
// reachable leaf is accepted when ray_triangle reports a hit (t > 0) and t_min <= t <= min(t_max, largest float below 1e30).
//   FIRST   the render's rule (trace_triangles): the first leaf in the reference's LIFO pop order with an accepted triangle, under
//           the 512-pop cap, and in it the least t, ties to the lowest triangle index;
//   CLOSEST least t over the accepted triangles of every reachable leaf, ties to the lowest index; no cap;
//   ANY     some accepted triangle: a hit exactly when CLOSEST has one.
// No walk prunes a box by t: a triangle's float t is not bounded below by its leaf's float tNear (a triangle on a shared leaf face
// can come out a rounding error in front of its own box; for a ray grazing its plane, Moeller-Trumbore's t carries the error of a
// small determinant), so CLOSEST visits every reachable triangle leaf.  The descriptors' visibility byte is never looked at.

namespace rto {

// ray_triangle (rto_device.hip.h) in its operation order, also returning the barycentrics u, v it computes on the way.
__device__ __forceinline__ bool ray_triangle_uv(float ox, float oy, float oz, float dx, float dy, float dz, const float* __restrict__ T,
                                                float& tOut, float& uOut, float& vOut) {
    const float v0x = T[0], v0y = T[1], v0z = T[2];
    const float e1x = T[3] - v0x, e1y = T[4] - v0y, e1z = T[5] - v0z;
    const float e2x = T[6] - v0x, e2y = T[7] - v0y, e2z = T[8] - v0z;
    const float px = dy * e2z - e2y * dz, py = dz * e2x - e2z * dx, pz = dx * e2y - e2x * dy;
    const float det = e1x * px + e1y * py + e1z * pz;
    if (__builtin_fabsf(det) < 1e-12f) return false;
    const float invDet = 1.0f / det;
    const float tx = ox - v0x, ty = oy - v0y, tz = oz - v0z;
    const float u = (tx * px + ty * py + tz * pz) * invDet;
    if (u < 0.0f || u > 1.0f) return false;
    const float qx = ty * e1z - e1y * tz, qy = tz * e1x - e1z * tx, qz = tx * e1y - e1x * ty;
    const float v = (dx * qx + dy * qy + dz * qz) * invDet;
    if (v < 0.0f || u + v > 1.0f) return false;
    const float t = (e2x * qx + e2y * qy + e2z * qz) * invDet;
    if (!(t > 0.0f)) return false;
    tOut = t; uOut = u; vOut = v;
    return true;
}

// The best accepted triangle so far: least t, ties to the lowest index.
struct TriBest {
    float t, u, v;
    int tri, leaf;
};

// Triangles k0 .. k1 - 1 of leaf `leaf` against the ray and the window [tlo, thi]; true when one of them was accepted (and is in B
// if it beats what B held).  tlo = max(t_min, 0) accepts what t_min <= t accepts: ray_triangle's t is > 0.
__device__ __forceinline__ bool tri_leaf(const float* __restrict__ tris, int k0, int k1, int leaf, const Ray& r, float tlo, float thi,
                                         TriBest& B) {
    bool got = false;
    for (int k = k0; k < k1; k++) {
        float t, u, v;
        if (!ray_triangle_uv(r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, tris + (size_t)k * 12, t, u, v)) continue;
        if (!(t >= tlo && t <= thi)) continue;
        got = true;
        if (t < B.t || (t == B.t && k < B.tri)) { B.t = t; B.u = u; B.v = v; B.tri = k; B.leaf = leaf; }
    }
    return got;
}

__device__ __forceinline__ void store_tri_hit(rto_tri_hit* __restrict__ hits, int64_t i, bool hit, const TriBest& B, const Ray& r,
                                              const float* __restrict__ tris) {
    int4* dst = reinterpret_cast<int4*>(hits) + 2 * i;
    if (hit) {
        const float* T = tris + (size_t)B.tri * 12;
        float nx = T[9], ny = T[10], nz = T[11];
        if (nx * r.dx + ny * r.dy + nz * r.dz > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }      // the renders' turn (k_trace_triangles)
        dst[0] = make_int4(__float_as_int(B.t), B.tri, B.leaf, __float_as_int(B.u));
        dst[1] = make_int4(__float_as_int(B.v), __float_as_int(nx), __float_as_int(ny), __float_as_int(nz));
    } else {
        dst[0] = make_int4(__float_as_int(1e30f), -1, -1, 0);
        dst[1] = make_int4(0, 0, 0, 0);
    }
}

// ================================================================ canonical trees: the descriptor walk
// k_query_desc's walk with the triangle render's interesting children: internal children and the leaf children that own triangles
// (descriptor bits 24..31, k_desc_trimask), minus the 8 exact verdicts of child_fail_mask_fast (child_fail_mask_exact for a wave
// holding a non-finite value) at the default clamps -- the render's box rule, whatever the mode, since no mode prunes by t.  A leaf
// child is re-tested with slab_exact when popped, then its triangles d_triOffset[leaf] .. d_triOffset[leaf + 1] are tested by its
// own lane (leaf = descFirstChild[parent's descriptor] + child).
//   FIRST   children pop 7 .. 0; the pop count of a leaf is k_query_desc's 1 + 8 entered - (popcount(x) + 2 popcount(y) +
//           4 popcount(z)); the first leaf with an accepted triangle ends the walk, a miss if it came past 512 pops.
//   CLOSEST the ray's own octant first (a convenience: the tie rule is by index, the walk exhaustive).
//   ANY     the same order, ends at the first leaf with an accepted triangle.
template <int QMODE, bool PIXELS>
__global__ __launch_bounds__(kBlock) void k_triq_desc(RenderParams P, QuerySrc Q, rto_tri_hit* __restrict__ hits,
                                                      const uint2* __restrict__ desc, const int* __restrict__ descFirstChild,
                                                      const float* __restrict__ tris, const int* __restrict__ triOffset) {
    extern __shared__ uint2 lds_stack[];   // [wave][level][lane] entries, then [wave][level][lane] descriptor indices
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = (int)(blockDim.x >> 6);
    const int levels = P.depth;
    uint2* stk = lds_stack + (size_t)wave * levels * kWave + lane;
    unsigned* stkNode = reinterpret_cast<unsigned*>(lds_stack + (size_t)waves * levels * kWave) + (size_t)wave * levels * kWave + lane;
    const int64_t i = Q.base + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const Geo G = geo_of(P);
    const float kEps = __uint_as_float(1u), kBelow1e30 = __uint_as_float(0x7149f2c9u);

    Ray r;
    r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
    float tlo = 0.0f, thi = 0.0f;
    bool active = false;
    if (i < Q.n && query_ray<PIXELS>(P, Q, i, r, tlo, thi)) {
        float tNear, tFar, a0, a1, a2, a3, a4, a5;
        active = slab_exact(G, r, 0, 0, 0, P.rootSize, tNear, tFar, a0, a1, a2, a3, a4, a5) && !(tNear >= 1e30f);
    }
    const bool risky = active && !(__builtin_isfinite(r.ix) && __builtin_isfinite(r.iy) && __builtin_isfinite(r.iz) &&
                                   __builtin_isfinite(r.ox) && __builtin_isfinite(r.oy) && __builtin_isfinite(r.oz) &&
                                   __builtin_isfinite(r.dx) && __builtin_isfinite(r.dy) && __builtin_isfinite(r.dz));
    const bool anyRisky = __builtin_amdgcn_ballot_w64(risky) != 0ull;
    const unsigned sgnX = (unsigned)((int)__float_as_uint(r.ix) >> 31), sgnY = (unsigned)((int)__float_as_uint(r.iy) >> 31),
                   sgnZ = (unsigned)((int)__float_as_uint(r.iz) >> 31);
    const unsigned flip = QMODE == kQueryFirst ? 0u : ((r.dx < 0.0f ? 1u : 0u) | (r.dy < 0.0f ? 2u : 0u) | (r.dz < 0.0f ? 4u : 0u));

    bool hit = false, enter = active;
    TriBest B;
    B.t = 1e30f; B.u = B.v = 0.0f; B.tri = -1; B.leaf = -1;
    unsigned cur = 0, lvlPending = 0;
    int cx = 0, cy = 0, cz = 0, bpos = P.depth - 1;
    int entered = 0;
    const int capEntered = kMaxTraversalSteps - 1 + 7 * P.depth;      // FIRST: 8 entered above this puts every later leaf past the cap
    while (active) {
        if (enter) {
            entered++;
            if (QMODE == kQueryFirst && 8 * entered > capEntered) break;
            const uint2 d = desc[cur];
            unsigned fail8;
            if (anyRisky) fail8 = child_fail_mask_exact(G.gx, G.gy, G.gz, G.vs, r.ox, r.oy, r.oz, r.ix, r.iy, r.iz, cx, cy, cz, 1 << bpos);
            else fail8 = child_fail_mask_fast<true, false>(G.gx, G.gy, G.gz, G.vs, r.ox, r.oy, r.oz, r.ix, r.iy, r.iz, sgnX, sgnY, sgnZ,
                                                           cx, cy, cz, (float)(1 << bpos), kEps, kBelow1e30);
            const unsigned im = (d.x >> 8) & 0xffu;
            unsigned cand = ((d.x >> 24) | im) & ~fail8 & 0xffu;     // triangle leaves and internal children whose box the ray meets
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
        if (im & bit) {
            cur = e.y + (unsigned)__builtin_popcount(im & (bit - 1u));
            cx = chx; cy = chy; cz = chz; bpos = Lb - 1; enter = true;
            continue;
        }
        {
            float tNear, tFar, a0, a1, a2, a3, a4, a5;
            if (!(slab_exact(G, r, chx, chy, chz, h, tNear, tFar, a0, a1, a2, a3, a4, a5) && !(tNear >= 1e30f))) continue;
        }
        const int leaf = descFirstChild[stkNode[Lb * kWave]] + j;
        const bool got = tri_leaf(tris, triOffset[leaf], triOffset[leaf + 1], leaf, r, tlo, thi, B);
        if (QMODE == kQueryClosest) {
            hit = hit || got;
        } else if (got) {
            hit = true;
            if (QMODE == kQueryFirst) {
                const int pops = 1 + 8 * entered - (__builtin_popcount(chx) + 2 * __builtin_popcount(chy) + 4 * __builtin_popcount(chz));
                if (pops > kMaxTraversalSteps) hit = false;        // the render's loop ended before this pop
            }
            break;
        }
    }
    if (i < Q.n) store_tri_hit(hits, i, hit, B, r, tris);
}

// ================================================================ any array, or RTO_KERNEL_GENERIC: node by node
// trace_triangles' walk over the 60-byte nodes, its stack of kStackCap entries in LDS ([entry][lane], one wave per workgroup,
// 36 KB) instead of a private int[kStackCap] in scratch.  FIRST stops at the first leaf with an accepted triangle or after 512
// pops, ANY at the first such leaf, CLOSEST walks every reachable node.
template <int QMODE, bool PIXELS>
__global__ __launch_bounds__(kQueryNodesBlock) void k_triq_nodes(RenderParams P, QuerySrc Q, rto_tri_hit* __restrict__ hits,
                                                                 const rto_node* __restrict__ nodes, const float* __restrict__ tris,
                                                                 const int* __restrict__ triOffset) {
    extern __shared__ int lds_query_stack[];                     // [kStackCap][lane]
    int* stack = lds_query_stack + threadIdx.x;
    const int64_t i = Q.base + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const Geo G = geo_of(P);
    Ray r;
    r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
    float tlo = 0.0f, thi = 0.0f;
    bool hit = false;
    TriBest B;
    B.t = 1e30f; B.u = B.v = 0.0f; B.tri = -1; B.leaf = -1;
    if (i < Q.n && query_ray<PIXELS>(P, Q, i, r, tlo, thi)) {
        int sp = 0, steps = 0;
        stack[kWave * sp++] = 0;
        while (sp > 0 && (QMODE != kQueryFirst || steps < kMaxTraversalSteps)) {
            const int nodeIdx = stack[kWave * --sp];
            steps++;
            const rto_node nd = nodes[nodeIdx];
            float tNear, tFar, a0, a1, a2, a3, a4, a5;
            if (!slab_exact(G, r, nd.x, nd.y, nd.z, nd.size, tNear, tFar, a0, a1, a2, a3, a4, a5)) continue;
            if (tNear >= 1e30f) continue;                          // the render's closestT, never lowered
            if (nd.isUniform == 1 || nd.isLeaf == 1) {
                const bool got = tri_leaf(tris, triOffset[nodeIdx], triOffset[nodeIdx + 1], nodeIdx, r, tlo, thi, B);
                hit = hit || got;
                if (got && QMODE != kQueryClosest) break;
                continue;
            }
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const int ch = nd.child[c];
                if (ch >= 0) stack[kWave * sp++] = ch;
            }
        }
    }
    if (i < Q.n) store_tri_hit(hits, i, hit, B, r, tris);
}

}  // namespace rto

// ---------------------------------------------------------------- host side
template <bool PIXELS>
static int launch_tri_query(rto_context* c, int mode, const RenderParams& P, QuerySrc Q, rto_tri_hit* hits, hipStream_t s) {
    const bool desc = c->canonical && c->numInternal > 0 && c->kernelMode != RTO_KERNEL_GENERIC;
    const size_t lds = (size_t)(kBlock / kWave) * P.depth * kWave * (sizeof(uint2) + sizeof(unsigned));   // <= 61,440 B (depth 20)
    const size_t ldsN = (size_t)kStackCap * kQueryNodesBlock * sizeof(int);
    for (int64_t off = 0; off < Q.n; off += kQueryChunk) {
        Q.base = off;
        const int64_t rays = std::min(Q.n - off, kQueryChunk);
        const dim3 grid((unsigned)((rays + kBlock - 1) / kBlock)), block(kBlock);
        const dim3 gridN((unsigned)((rays + kQueryNodesBlock - 1) / kQueryNodesBlock)), blockN(kQueryNodesBlock);
        if (desc) {
            if (mode == RTO_QUERY_FIRST) hipLaunchKernelGGL((k_triq_desc<kQueryFirst, PIXELS>), grid, block, lds, s, P, Q, hits, c->d_desc, c->d_descFirstChild, c->d_tris, c->d_triOffset);
            else if (mode == RTO_QUERY_CLOSEST) hipLaunchKernelGGL((k_triq_desc<kQueryClosest, PIXELS>), grid, block, lds, s, P, Q, hits, c->d_desc, c->d_descFirstChild, c->d_tris, c->d_triOffset);
            else hipLaunchKernelGGL((k_triq_desc<kQueryAny, PIXELS>), grid, block, lds, s, P, Q, hits, c->d_desc, c->d_descFirstChild, c->d_tris, c->d_triOffset);
        } else {
            if (mode == RTO_QUERY_FIRST) hipLaunchKernelGGL((k_triq_nodes<kQueryFirst, PIXELS>), gridN, blockN, ldsN, s, P, Q, hits, c->d_nodes, c->d_tris, c->d_triOffset);
            else if (mode == RTO_QUERY_CLOSEST) hipLaunchKernelGGL((k_triq_nodes<kQueryClosest, PIXELS>), gridN, blockN, ldsN, s, P, Q, hits, c->d_nodes, c->d_tris, c->d_triOffset);
            else hipLaunchKernelGGL((k_triq_nodes<kQueryAny, PIXELS>), gridN, blockN, ldsN, s, P, Q, hits, c->d_nodes, c->d_tris, c->d_triOffset);
        }
        RTO_HIP(c, hipGetLastError());
    }
    return RTO_OK;
}

// The checks every entry shares after query_check: something to trace against.
static int tri_query_ready(rto_context* c, const char* fn) {
    if (c->numNodes <= 0 || !c->d_triOffset || !c->d_tris)
        return fail(c, RTO_E_NO_OCTREE, std::string(fn) + ": no leaf triangles resident (rto_build_leaf_triangles / rto_upload_leaf_triangles)");
    return RTO_OK;
}

static int tri_query_rays(rto_context* c, int mode, const rto_ray* d_rays, int64_t n, rto_tri_hit* d_hits, hipStream_t s) {
    if ((reinterpret_cast<uintptr_t>(d_rays) & 15) || (reinterpret_cast<uintptr_t>(d_hits) & 15))
        return fail(c, RTO_E_INVALID, "rto_query_triangles: the ray and hit buffers must be 16-byte aligned");
    RenderParams P;
    std::memset(&P, 0, sizeof P);
    query_geometry(c, P);
    return launch_tri_query<false>(c, mode, P, QuerySrc{ d_rays, nullptr, nullptr, n, 0 }, d_hits, s);
}

static int tri_query_pixels(rto_context* c, int mode, const rto_frame* f, const int32_t* d_xy, int64_t n, rto_tri_hit* d_hits, hipStream_t s) {
    if (reinterpret_cast<uintptr_t>(d_hits) & 15) return fail(c, RTO_E_INVALID, "rto_query_triangle_pixels: the hit buffer must be 16-byte aligned");
    RenderParams P;
    const int rc = fill_params(c, f, nullptr, P, s);             // the renders' ray tables and inverse view: bit-identical rays
    if (rc != RTO_OK) return rc;
    return launch_tri_query<true>(c, mode, P, QuerySrc{ nullptr, d_xy, nullptr, n, 0 }, d_hits, s);
}

extern "C" {

int rto_query_triangles_device(rto_context* c, int mode, const rto_ray* d_rays, int64_t n, rto_tri_hit* d_hits, void* hip_stream) {
    if (!c) return RTO_E_INVALID;
    int rc = query_check(c, "rto_query_triangles_device", mode, n, d_rays, d_hits);
    if (rc != RTO_OK || n == 0) return rc;
    if ((rc = tri_query_ready(c, "rto_query_triangles_device")) != RTO_OK) return rc;
    RTO_HIP(c, hipSetDevice(c->device));
    return tri_query_rays(c, mode, d_rays, n, d_hits, (hipStream_t)hip_stream);
}

int rto_query_triangles_host(rto_context* c, int mode, const rto_ray* rays, int64_t n, rto_tri_hit* hits) {
    if (!c) return RTO_E_INVALID;
    int rc = query_check(c, "rto_query_triangles_host", mode, n, rays, hits);
    if (rc != RTO_OK || n == 0) return rc;
    if ((rc = tri_query_ready(c, "rto_query_triangles_host")) != RTO_OK) return rc;
    RTO_HIP(c, hipSetDevice(c->device));
    BuildScratch scratch(c->stream);
    rto_ray* d_rays = nullptr;
    rto_tri_hit* d_hits = nullptr;
    RTO_HIP(c, scratch.alloc(&d_rays, (size_t)n));
    RTO_HIP(c, scratch.alloc(&d_hits, (size_t)n));
    RTO_HIP(c, hipMemcpyAsync(d_rays, rays, (size_t)n * sizeof(rto_ray), hipMemcpyHostToDevice, c->stream));
    if ((rc = tri_query_rays(c, mode, d_rays, n, d_hits, c->stream)) != RTO_OK) return rc;
    RTO_HIP(c, hipMemcpyAsync(hits, d_hits, (size_t)n * sizeof(rto_tri_hit), hipMemcpyDeviceToHost, c->stream));
    RTO_HIP(c, hipStreamSynchronize(c->stream));
    return RTO_OK;
}

int rto_query_triangle_pixels_device(rto_context* c, int mode, const rto_frame* frame, const int32_t* d_xy, int64_t n,
                                     rto_tri_hit* d_hits, void* hip_stream) {
    if (!c) return RTO_E_INVALID;
    int rc = query_check(c, "rto_query_triangle_pixels_device", mode, n, d_xy, d_hits);
    if (rc != RTO_OK || n == 0) return rc;
    if (!frame) return fail(c, RTO_E_INVALID, "rto_query_triangle_pixels_device: frame is NULL");
    if ((rc = tri_query_ready(c, "rto_query_triangle_pixels_device")) != RTO_OK) return rc;
    RTO_HIP(c, hipSetDevice(c->device));
    return tri_query_pixels(c, mode, frame, d_xy, n, d_hits, (hipStream_t)hip_stream);
}

int rto_query_triangle_pixels_host(rto_context* c, int mode, const rto_frame* frame, const int32_t* xy, int64_t n, rto_tri_hit* hits) {
    if (!c) return RTO_E_INVALID;
    int rc = query_check(c, "rto_query_triangle_pixels_host", mode, n, xy, hits);
    if (rc != RTO_OK || n == 0) return rc;
    if (!frame) return fail(c, RTO_E_INVALID, "rto_query_triangle_pixels_host: frame is NULL");
    if ((rc = tri_query_ready(c, "rto_query_triangle_pixels_host")) != RTO_OK) return rc;
    RTO_HIP(c, hipSetDevice(c->device));
    BuildScratch scratch(c->stream);
    int32_t* d_xy = nullptr;
    rto_tri_hit* d_hits = nullptr;
    RTO_HIP(c, scratch.alloc(&d_xy, (size_t)n * 2));
    RTO_HIP(c, scratch.alloc(&d_hits, (size_t)n));
    RTO_HIP(c, hipMemcpyAsync(d_xy, xy, (size_t)n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if ((rc = tri_query_pixels(c, mode, frame, d_xy, n, d_hits, c->stream)) != RTO_OK) return rc;
    RTO_HIP(c, hipMemcpyAsync(hits, d_hits, (size_t)n * sizeof(rto_tri_hit), hipMemcpyDeviceToHost, c->stream));
    RTO_HIP(c, hipStreamSynchronize(c->stream));
    return RTO_OK;
}

}  // extern "C"
