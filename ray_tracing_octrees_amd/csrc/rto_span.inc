// rto_span.inc -- span queries (include/rto_hip.h, rto_query_spans_*, rto_query_span_pixels_*): how much solid a ray passes
// through.  Caller rays, or the renders' own pixel rays, through the whole resident octree; one rto_span record per ray.  Included at
// the end of rto_api.hip, after rto_query.inc (whose ray sources, walk, box rule and entries it shares).
//
// Rule (DESIGN.md section 15).  The window and the acceptance of a solid leaf are the box queries': t_lo = max(t_min, 0), t_hi =
// min(t_max, largest float below 1e30); the leaf's box and every ancestor's pass the float32 slab test with tNear < 1e30, and tIn =
// max(t_lo, tNear) satisfies tIn <= tFar and tIn <= t_hi.  An accepted leaf contributes tOut - tIn with tOut = min(tFar, t_hi), one
// float32 subtraction, >= 0.  The record sums the contributions of every accepted leaf in visit order (depth first, a node's
// children in slots i ^ flip for i = 0 .. 7, flip = the sign bits of d), counts them, keeps the least tIn and the greatest tOut, and
// carries CLOSEST's leaf and face.  Boxes are cut by t_hi alone: a child's tNear is never below its parent's, so a box with tNear >
// t_hi holds no leaf with tIn <= t_hi; nothing is cut against t_lo, the exact test at the pop decides.

namespace rto {

// desc_walk's leaf rule for spans.  Every solid leaf is a candidate, closest() bounds nothing (boxes see t_hi only), and leaf(..)
// accumulates: the walk never ends on a leaf (kEveryLeaf).  The CLOSEST part of the record is BoxRule<CLOSEST>'s own update.
struct SpanRule {
    static constexpr bool kPrune = true;
    static constexpr bool kEveryLeaf = true;
    BoxRule<kQueryClosest> box;
    float length, tExit;
    int count;
    __device__ __forceinline__ SpanRule() : length(0.0f), tExit(-1.0f), count(0) {}
    __device__ __forceinline__ static unsigned leaves(unsigned dx) { return dx & 0xffu; }
    __device__ __forceinline__ float closest() const { return 1e30f; }
    __device__ __forceinline__ bool leaf(const Ray& r, float tlo, float thi, float tNear, float tFar, int x, int y, int z, int size, int j,
                                         const unsigned* node) {
        // plain booleans and selects, as in BoxRule: no short-circuit update inside the divergent loop
        const float tIn = gmax(tlo, tNear);
        const bool acc = tIn <= tFar && tIn <= thi;
        const float tOut = gmin(tFar, thi);
        const float sum = length + (tOut - tIn);
        length = acc ? sum : length;
        tExit = acc ? gmax(tExit, tOut) : tExit;                   // tOut >= tIn >= 0 > the start value
        count += acc ? 1 : 0;
        box.leaf(r, tlo, thi, tNear, tFar, x, y, z, size, j, node);
        return acc;
    }
};

__device__ __forceinline__ void store_span(rto_span* __restrict__ spans, int64_t i, const SpanRule& R, int node, int face) {
    int4* dst = reinterpret_cast<int4*>(spans) + 2 * i;
    if (R.count > 0) dst[0] = make_int4(__float_as_int(R.length), __float_as_int(R.box.best.t), __float_as_int(R.tExit), R.count);
    else dst[0] = make_int4(0, __float_as_int(1e30f), __float_as_int(1e30f), 0);
    dst[1] = make_int4(R.count > 0 ? node : -1, R.count > 0 ? face : -1, 0, 0);
}

// Canonical trees: desc_walk in octant order under SpanRule, the LDS stacks sized by the tree's depth as in k_query_desc.
template <bool PIXELS>
__global__ __launch_bounds__(kBlock) void k_span_desc(RenderParams P, QuerySrc Q, rto_span* __restrict__ spans,
                                                      const uint2* __restrict__ desc, const int* __restrict__ descFirstChild) {
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
    SpanRule R;
    desc_walk<kQueryAny>(P, G, r, tlo, thi, valid, desc, stk, stkNode, R);
    if (i < Q.n) {
        const DescHit& w = R.box.best;
        const bool hit = R.count > 0;
        store_span(spans, i, R, hit ? descFirstChild[w.node] + w.j : -1, hit ? query_face(G, r, w.x, w.y, w.z, w.size, w.t) : -1);
    }
}

// Any array, one-node trees, RTO_KERNEL_GENERIC: the 60-byte nodes one by one, the stack of kStackCap entries in LDS ([entry][lane],
// one wave per workgroup) as in k_query_nodes.  Children are pushed in slots (7 .. 0) ^ flip, so they pop in slots (0 .. 7) ^ flip:
// desc_walk's visit order, hence the same float sum.  The tests of a popped node are desc_walk's pruning ones.
template <bool PIXELS>
__global__ __launch_bounds__(kQueryNodesBlock) void k_span_nodes(RenderParams P, QuerySrc Q, rto_span* __restrict__ spans,
                                                                 const rto_node* __restrict__ nodes) {
    extern __shared__ int lds_query_stack[];                     // [kStackCap][lane]
    int* stack = lds_query_stack + threadIdx.x;
    const int64_t i = Q.base + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const Geo G = geo_of(P);
    Ray r;
    r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
    float tlo = 0.0f, thi = 0.0f;
    SpanRule R;
    if (i < Q.n && query_ray<PIXELS>(P, Q, i, r, tlo, thi)) {
        const int flip = (r.dx < 0.0f ? 1 : 0) | (r.dy < 0.0f ? 2 : 0) | (r.dz < 0.0f ? 4 : 0);
        int sp = 0;
        stack[kWave * sp++] = 0;
        while (sp > 0) {
            const unsigned nodeIdx = (unsigned)stack[kWave * --sp];
            const rto_node nd = nodes[nodeIdx];
            float tNear, tFar, a0, a1, a2, a3, a4, a5;
            if (!slab_exact(G, r, nd.x, nd.y, nd.z, nd.size, tNear, tFar, a0, a1, a2, a3, a4, a5)) continue;
            if (tNear >= 1e30f || tNear > thi) continue;
            if (nd.isUniform == 1 || nd.isLeaf == 1) {
                if (nd.isSolid == 1) R.leaf(r, tlo, thi, tNear, tFar, nd.x, nd.y, nd.z, nd.size, 0, &nodeIdx);
                continue;
            }
            const int* __restrict__ child = nodes[nodeIdx].child;      // read by slot from memory: a register array indexed by c ^ flip would be scratch
#pragma unroll
            for (int c = 7; c >= 0; c--) {
                const int ch = child[c ^ flip];
                if (ch >= 0) stack[kWave * sp++] = ch;
            }
        }
    }
    if (i < Q.n) {
        const DescHit& w = R.box.best;
        const bool hit = R.count > 0;
        store_span(spans, i, R, (int)w.node, hit ? query_face(G, r, w.x, w.y, w.z, w.size, w.t) : -1);
    }
}

}  // namespace rto

// ---------------------------------------------------------------- host side
// The span walk has one order, the octant one: launch_query is asked for it under the mode that names that order.
constexpr int kSpanWalk = RTO_QUERY_ANY;

// k_span_nodes pushes a node's children in the ray's octant order, not in slot order as every other node walk does, so
// rto_upload_octree's bound on the stack (walk_stack_need in slot order) does not cover it.  A canonical tree holds at most 7 entries
// per level of its 20 at most in any order; for any other array the upload also recorded the need under the worst order, and an
// array past kStackCap there is refused here instead of walked.
template <bool PIXELS>
static int launch_span_query(rto_context* c, const RenderParams& P, const QuerySrc& Q0, rto_span* spans, hipStream_t s) {
    if (!c->canonical && c->anyOrderStackNeed > kStackCap)
        return fail(c, RTO_E_UNSUPPORTED, "rto_query_spans: a walk of this array in a ray's octant order could hold more than " +
                                              std::to_string(kStackCap) + " stack entries");
    return launch_query(c, kSpanWalk, P.depth, Q0, [&](auto, bool desc, dim3 grid, dim3 block, size_t lds, const QuerySrc& Q) {
        if (desc) hipLaunchKernelGGL((k_span_desc<PIXELS>), grid, block, lds, s, P, Q, spans, c->d_desc, c->d_descFirstChild);
        else hipLaunchKernelGGL((k_span_nodes<PIXELS>), grid, block, lds, s, P, Q, spans, c->d_nodes);
    });
}

static int span_rays(rto_context* c, const rto_ray* d_rays, int64_t n, rto_span* d_spans, hipStream_t s) {
    if ((reinterpret_cast<uintptr_t>(d_rays) & 15) || (reinterpret_cast<uintptr_t>(d_spans) & 15))
        return fail(c, RTO_E_INVALID, "rto_query_spans: the ray and span buffers must be 16-byte aligned");
    RenderParams P;
    std::memset(&P, 0, sizeof P);
    query_geometry(c, P);
    return launch_span_query<false>(c, P, QuerySrc{ d_rays, nullptr, nullptr, n, 0 }, d_spans, s);
}

static int span_pixels(rto_context* c, const rto_frame* f, const int32_t* d_xy, int64_t n, rto_span* d_spans, hipStream_t s) {
    if (reinterpret_cast<uintptr_t>(d_spans) & 15) return fail(c, RTO_E_INVALID, "rto_query_span_pixels: the span buffer must be 16-byte aligned");
    RenderParams P;
    const int rc = fill_params(c, f, nullptr, P, s);             // the renders' ray tables and inverse view: bit-identical rays
    if (rc != RTO_OK) return rc;
    return launch_span_query<true>(c, P, QuerySrc{ nullptr, d_xy, nullptr, n, 0 }, d_spans, s);
}

extern "C" {

int rto_query_spans_device(rto_context* c, const rto_ray* d_rays, int64_t n, rto_span* d_spans, void* hip_stream) {
    return query_entry(c, "rto_query_spans_device", kSpanWalk, false, nullptr, false, d_rays, n, d_spans, false, hip_stream,
                       [=](const rto_ray* r, rto_span* o, hipStream_t s) { return span_rays(c, r, n, o, s); });
}

int rto_query_spans_host(rto_context* c, const rto_ray* rays, int64_t n, rto_span* spans) {
    return query_entry(c, "rto_query_spans_host", kSpanWalk, false, nullptr, false, rays, n, spans, true, nullptr,
                       [=](const rto_ray* r, rto_span* o, hipStream_t s) { return span_rays(c, r, n, o, s); });
}

int rto_query_span_pixels_device(rto_context* c, const rto_frame* frame, const int32_t* d_xy, int64_t n, rto_span* d_spans, void* hip_stream) {
    return query_entry(c, "rto_query_span_pixels_device", kSpanWalk, true, frame, false, d_xy, n, d_spans, false, hip_stream,
                       [=](const int32_t* xy, rto_span* o, hipStream_t s) { return span_pixels(c, frame, xy, n, o, s); });
}

int rto_query_span_pixels_host(rto_context* c, const rto_frame* frame, const int32_t* xy, int64_t n, rto_span* spans) {
    return query_entry(c, "rto_query_span_pixels_host", kSpanWalk, true, frame, false, xy, n, spans, true, nullptr,
                       [=](const int32_t* d_xy, rto_span* o, hipStream_t s) { return span_pixels(c, frame, d_xy, n, o, s); });
}

}  // extern "C"
