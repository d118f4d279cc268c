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

// The triangle queries' leaf rule for desc_walk (rto_query.inc).  The candidate leaves of a descriptor are the ones
// that own triangles (bits 24..31, k_desc_trimask); a popped leaf whose box passes has its triangles d_triOffset[leaf] ..
// d_triOffset[leaf + 1] tested by its own lane.  No box is pruned by t (the header says why): every mode walks with the render's box
// rule at the default clamps and CLOSEST visits every reachable triangle leaf -- in the ray's own octant order, a convenience only:
// the tie rule is by index.
struct TriRule {
    static constexpr bool kPrune = false;
    static constexpr bool kEveryLeaf = false;
    const int* __restrict__ descFirstChild;
    const float* __restrict__ tris;
    const int* __restrict__ triOffset;
    TriBest B;
    __device__ __forceinline__ TriRule(const int* dfc, const float* t, const int* off) : descFirstChild(dfc), tris(t), triOffset(off) {
        B.t = 1e30f; B.u = B.v = 0.0f; B.tri = -1; B.leaf = -1;
    }
    __device__ __forceinline__ static unsigned leaves(unsigned dx) { return dx >> 24; }
    __device__ __forceinline__ float closest() const { return 1e30f; }      // never read: kPrune is false
    __device__ __forceinline__ bool leaf(const Ray& r, float tlo, float thi, float, float, int, int, int, int, int j, const unsigned* node) {
        const int leaf = descFirstChild[*node] + j;
        return tri_leaf(tris, triOffset[leaf], triOffset[leaf + 1], leaf, r, tlo, thi, B);
    }
};

// Canonical trees: desc_walk under TriRule.  FIRST is the render's rule (trace_triangles' pop order and 512-pop cap).
template <int QMODE, bool PIXELS>
__global__ __launch_bounds__(kBlock) void k_triq_desc(RenderParams P, QuerySrc Q, rto_tri_hit* __restrict__ hits,
                                                      const uint2* __restrict__ desc, const int* __restrict__ descFirstChild,
                                                      const float* __restrict__ tris, const int* __restrict__ triOffset) {
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
    TriRule R(descFirstChild, tris, triOffset);
    const bool hit = desc_walk<QMODE>(P, G, r, tlo, thi, valid, desc, stk, stkNode, R);
    if (i < Q.n) store_tri_hit(hits, i, hit, R.B, r, tris);
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
static int launch_tri_query(rto_context* c, int mode, const RenderParams& P, const QuerySrc& Q0, rto_tri_hit* hits, hipStream_t s) {
    return launch_query(c, mode, P.depth, Q0, [&](auto m, bool desc, dim3 grid, dim3 block, size_t lds, const QuerySrc& Q) {
        constexpr int M = decltype(m)::value;
        if (desc) hipLaunchKernelGGL((k_triq_desc<M, PIXELS>), grid, block, lds, s, P, Q, hits, c->d_desc, c->d_descFirstChild, c->d_tris, c->d_triOffset);
        else hipLaunchKernelGGL((k_triq_nodes<M, PIXELS>), grid, block, lds, s, P, Q, hits, c->d_nodes, c->d_tris, c->d_triOffset);
    });
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
    return query_entry(c, "rto_query_triangles_device", mode, false, nullptr, true, d_rays, n, d_hits, false, hip_stream,
                       [=](const rto_ray* r, rto_tri_hit* h, hipStream_t s) { return tri_query_rays(c, mode, r, n, h, s); });
}

int rto_query_triangles_host(rto_context* c, int mode, const rto_ray* rays, int64_t n, rto_tri_hit* hits) {
    return query_entry(c, "rto_query_triangles_host", mode, false, nullptr, true, rays, n, hits, true, nullptr,
                       [=](const rto_ray* r, rto_tri_hit* h, hipStream_t s) { return tri_query_rays(c, mode, r, n, h, s); });
}

int rto_query_triangle_pixels_device(rto_context* c, int mode, const rto_frame* frame, const int32_t* d_xy, int64_t n,
                                     rto_tri_hit* d_hits, void* hip_stream) {
    return query_entry(c, "rto_query_triangle_pixels_device", mode, true, frame, true, d_xy, n, d_hits, false, hip_stream,
                       [=](const int32_t* xy, rto_tri_hit* h, hipStream_t s) { return tri_query_pixels(c, mode, frame, xy, n, h, s); });
}

int rto_query_triangle_pixels_host(rto_context* c, int mode, const rto_frame* frame, const int32_t* xy, int64_t n, rto_tri_hit* hits) {
    return query_entry(c, "rto_query_triangle_pixels_host", mode, true, frame, true, xy, n, hits, true, nullptr,
                       [=](const int32_t* d_xy, rto_tri_hit* h, hipStream_t s) { return tri_query_pixels(c, mode, frame, d_xy, n, h, s); });
}

}  // extern "C"
