// rto_lit.inc -- the lit render (include/rto_hip.h, rto_render_lit_*): the box render's frame with a shadow ray and ambient
// occlusion per hit pixel, all on the device.  Included at the end of rto_api.hip, after rto_query.inc (box_walk: desc_walk under the box rule).
// It also holds the frame pass, the pieces its kernels share with rto_tri_lit.inc and rto_field_view.inc -- on the device
// kLargestBelow1e30, rooted_box_walk, tile_pixel, lit_append, LitSpace, lit_ao_entry and lit_settle; on the host frame_bound_check,
// frame_tree_check, lit_check, lit_reserve, render_lit_frame and lit_entry.
//
// Rule (DESIGN.md section 12).  The primary hit is the FIRST box query on the frame's pixel ray; the secondary origin is the hit
// point p = o + d tHit with its coordinate on the entry face's axis a replaced by the leaf's own plane + sigma eps (sigma = +1 for
// an odd face, eps = voxelSize 1e-3 + 2^-18 max|p|); shadow and AO rays are ANY queries from there, (0, 1e30) towards the light and
// (0, ao_radius] along the table directions.  Colour: d = S ? ndotl : 0, amb = 0.1 A, (d + amb, 0.8 d + amb, 0.6 d + amb, 1).
//
// Kernels (one stream, no host step):
//   k_lit_primary    one lane per pixel, 8x8 tiles per wave: the FIRST walk, the Lambert term and the secondary origin.  Pixels
//                    without secondary rays (sky, camera inside a solid leaf, no term asked for) are written at once; the others
//                    are compacted (one ballot and one atomic per wave) into 32-byte records.
//   k_lit_secondary  persistent waves over the secondary rays of the compacted hits: the shadow rays first, one per hit, then,
//                    from the next multiple of 64, K AO rays per hit in adjacent lanes.  Each ray is built in registers from its
//                    record (no ray is stored) and walked by box_walk<ANY>.  A hit's verdicts are summed in the wave (ballot +
//                    popcount over its lanes) and added to its counter with one atomic per piece (+1 << 16 per piece); the
//                    piece that completes the count shades the pixel.

namespace rto {

constexpr int kLitMaxSamples = RTO_AO_MAX_SAMPLES;

// The AO table: entry i = cosine-weighted Hammersley, u = (i + 0.5) / 64, phi = 2 pi (bitrev6(i) + 0.5) / 64,
// (sqrt(u) cos phi, sqrt(u) sin phi, sqrt(1 - u)) computed in double and rounded once (tests/lit_ref.py restates it).
#define RTO_AO_TABLE \
    0x1.699a42p-4f, 0x1.1c3af6p-8f, 0x1.fdfefep-1f, -0x1.392832p-3f, -0x1.ec4d26p-8f, 0x1.f9f6e4p-1f, \
    -0x1.3dc778p-7f, 0x1.9448b2p-3f, 0x1.f5e68p-1f, 0x1.78005ap-7f, -0x1.de5af2p-3f, 0x1.f1cd9cp-1f, \
    0x1.6cb20ap-3f, 0x1.926124p-3f, 0x1.edac06p-1f, -0x1.932f9ep-3f, -0x1.bcd8e2p-3f, 0x1.e9818p-1f, \
    -0x1.e39994p-3f, 0x1.b64f36p-3f, 0x1.e54dd4p-1f, 0x1.03bc1cp-2f, -0x1.d6d1ep-3f, 0x1.e110c4p-1f, \
    0x1.515ap-2f, 0x1.3f1c5ep-3f, 0x1.dcca0ep-1f, -0x1.64a4e4p-2f, -0x1.515c36p-3f, 0x1.d8796ep-1f, \
    -0x1.62abfep-3f, 0x1.76f1fep-2f, 0x1.d41eap-1f, 0x1.732d4ap-3f, -0x1.8864d2p-2f, 0x1.cfb95cp-1f, \
    0x1.30eafap-3f, 0x1.aa181ep-2f, 0x1.cb4952p-1f, -0x1.3ce146p-3f, -0x1.bacf62p-2f, 0x1.c6ce32p-1f, \
    -0x1.caeae2p-2f, 0x1.486818p-3f, 0x1.c247a8p-1f, 0x1.da7a7ap-2f, -0x1.538accp-3f, 0x1.bdb55cp-1f, \
    0x1.f85b48p-2f, 0x1.f956c6p-4f, 0x1.b916eep-1f, -0x1.03b528p-1f, -0x1.0436a8p-3f, 0x1.b46bfcp-1f, \
    -0x1.0b8b7ep-3f, 0x1.0b0658p-1f, 0x1.afb42p-1f, 0x1.12ae42p-3f, -0x1.12258ep-1f, 0x1.aaeeeap-1f, \
    0x1.29f20cp-2f, 0x1.f1179p-2f, 0x1.a61be6p-1f, -0x1.31203ep-2f, -0x1.fd1266p-2f, 0x1.a13a9cp-1f, \
    -0x1.04635ap-1f, 0x1.382428p-2f, 0x1.9c4a8ap-1f, 0x1.0a1c92p-1f, -0x1.3f0098p-2f, 0x1.974b24p-1f, \
    0x1.fce2e6p-2f, 0x1.796a74p-2f, 0x1.923bd8p-1f, -0x1.03957ep-1f, -0x1.810a8ap-2f, 0x1.8d1c0cp-1f, \
    -0x1.8884b4p-2f, 0x1.089ff8p-1f, 0x1.87eb1ap-1f, 0x1.8fdb16p-2f, -0x1.0d9252p-1f, 0x1.82a85p-1f, \
    0x1.911028p-4f, 0x1.51f7eep-1f, 0x1.7d52f2p-1f, -0x1.9809e4p-4f, -0x1.57d8bcp-1f, 0x1.77ea36p-1f, \
    -0x1.5da04p-1f, 0x1.9ee59cp-4f, 0x1.726d42p-1f, 0x1.634fb2p-1f, -0x1.a5a4c6p-4f, 0x1.6cdb2cp-1f, \
    0x1.68e838p-1f, 0x1.ac48bcp-4f, 0x1.6732f8p-1f, -0x1.6e6aep-1f, -0x1.b2d2bcp-4f, 0x1.617398p-1f, \
    -0x1.b943eep-4f, 0x1.73d89ep-1f, 0x1.5b9be6p-1f, 0x1.bf9d64p-4f, -0x1.79325ep-1f, 0x1.55aaap-1f, \
    0x1.cca9c6p-2f, 0x1.3690f2p-1f, 0x1.4f9e6cp-1f, -0x1.d2ee56p-2f, -0x1.3acab2p-1f, 0x1.4975cep-1f, \
    -0x1.3ef61ep-1f, 0x1.d91da4p-2f, 0x1.432f24p-1f, 0x1.4313c2p-1f, -0x1.df3882p-2f, 0x1.3cc8aap-1f, \
    0x1.5d58e8p-1f, 0x1.a2c80cp-2f, 0x1.364064p-1f, -0x1.61a248p-1f, -0x1.a7eb88p-2f, 0x1.2f9422p-1f, \
    -0x1.acff42p-2f, 0x1.65de84p-1f, 0x1.28c17cp-1f, 0x1.b203c8p-2f, -0x1.6a0e12p-1f, 0x1.21c5b8p-1f, \
    0x1.9ef1fep-3f, 0x1.9e237ap-1f, 0x1.1a9dc8p-1f, -0x1.a394e8p-3f, -0x1.a2c418p-1f, 0x1.13464p-1f, \
    -0x1.a757c2p-1f, 0x1.a82adap-3f, 0x1.0bbb3p-1f, 0x1.abdee4p-1f, -0x1.acb43ep-3f, 0x1.03f82p-1f, \
    0x1.a3a774p-1f, 0x1.2c4f2ep-2f, 0x1.f7efbep-2f, -0x1.a7f558p-1f, -0x1.2f63b4p-2f, 0x1.e768d4p-2f, \
    -0x1.32704ep-2f, 0x1.ac3828p-1f, 0x1.d64d52p-2f, 0x1.357536p-2f, -0x1.b0703ap-1f, 0x1.c48c6p-2f, \
    0x1.8c89p-2f, 0x1.a3339ap-1f, 0x1.b211b2p-2f, -0x1.904b3cp-2f, -0x1.a72cd6p-1f, 0x1.9ec474p-2f, \
    -0x1.ab1c9cp-1f, 0x1.940482p-2f, 0x1.8a85c2p-2f, 0x1.af032cp-1f, -0x1.97b516p-2f, 0x1.752e5p-2f, \
    0x1.64722ep-1f, 0x1.431058p-1f, 0x1.5e8adep-2f, -0x1.67962ap-1f, -0x1.45e908p-1f, 0x1.465656p-2f, \
    -0x1.48bb68p-1f, 0x1.6ab32ep-1f, 0x1.2c2fc6p-2f, 0x1.4b87a2p-1f, -0x1.6dc96cp-1f, 0x1.0f876cp-2f, \
    0x1.86d114p-5f, 0x1.f1341cp-1f, 0x1.deeea2p-3f, -0x1.8a088ap-5f, -0x1.f54bbcp-1f, 0x1.94c584p-3f, \
    -0x1.f95aep-1f, 0x1.8d3956p-5f, 0x1.3988e2p-3f, 0x1.fd61bcp-1f, -0x1.90639ep-5f, 0x1.6a09e6p-4f
__constant__ float kAoDirDev[3 * kLitMaxSamples] = { RTO_AO_TABLE };

__device__ __forceinline__ unsigned lit_mix32(unsigned v) {
    v ^= v >> 16; v *= 0x7feb352du; v ^= v >> 15; v *= 0x846ca68bu; v ^= v >> 16;
    return v;
}

__device__ __forceinline__ float4 lit_color(float ndotl, bool S, float A) {
    const float d = S ? ndotl : 0.0f, amb = 0.1f * A;
    return make_float4(1.0f * d + amb, 0.8f * d + amb, 0.6f * d + amb, 1.0f);
}

struct LitArgs {
    int4* rec;               // per compacted hit: {so.x, so.y, so.z, ndotl}, {pixel, face | shadow cast << 3, hash, 0}
    unsigned* acc;           // per compacted hit: verdicts (occ + 256 shadow blocked) | pieces done << 16
    unsigned* count;         // hits compacted (zeroed in front of the frame)
    float4* rgba;
    int* vis;                // may be null
    int shadow, K;
    float radius;            // AO window's t_hi: min(ao_radius, largest float below 1e30)
    unsigned seed;
    int rootLeaf;            // 1: the tree is one leaf, nodes[0] (no descriptors): its box is the whole walk
    const rto_node* nodes;
};

__device__ __forceinline__ void lit_store(const LitArgs& L, unsigned pix, float4 c, int v) {
    L.rgba[pix] = c;
    if (L.vis) L.vis[pix] = v;
}

// ---------------------------------------------------------------- the frame pass
// What the kernels of the lit render, of its triangle form (rto_tri_lit.inc) and of the field views (rto_field_view.inc) share
// (DESIGN.md section 12): the open window's far end, the walk of a tree that may be one leaf, a lane's pixel and ray, the
// compaction of the hits, and the dense space of the secondary rays with the AO entry of a ray and the settling of a hit.

constexpr float kLargestBelow1e30 = __builtin_bit_cast(float, 0x7149f2c9u);   // t_hi of the open window (0, 1e30)

// box_walk in the window [tlo, thi], or for a tree that is one leaf (rootLeaf: nodes[0], no descriptors) the root's own test: the
// slab test with tNear < 1e30 (and, outside FIRST, tNear <= t_hi), then tHit = max(t_lo, tNear) <= tFar and <= t_hi if the leaf
// is solid -- what the walk of a one-node array does under every rule.  rootLeaf is the same for every lane, so the ballot inside
// the walk still sees the whole wave.
template <int QMODE>
__device__ __forceinline__ DescHit rooted_box_walk(const RenderParams& P, const Geo& G, const Ray r, float tlo, float thi, bool valid,
                                                   int rootLeaf, const rto_node* nodes, const uint2* __restrict__ desc, uint2* stk,
                                                   unsigned* stkNode) {
    if (!rootLeaf) return box_walk<QMODE>(P, G, r, tlo, thi, valid, desc, stk, stkNode);
    DescHit w;
    w.hit = false; w.t = 1e30f; w.x = w.y = w.z = 0; w.size = P.rootSize; w.j = 0; w.node = 0;
    if (valid && nodes[0].isSolid == 1) {
        float tNear, tFar, a0, a1, a2, a3, a4, a5;
        bool pass = slab_exact(G, r, 0, 0, 0, P.rootSize, tNear, tFar, a0, a1, a2, a3, a4, a5) && !(tNear >= 1e30f);
        if (QMODE != kQueryFirst) pass = pass && !(tNear > thi);
        const float tHit = gmax(tlo, tNear);
        if (pass && tHit <= tFar && tHit <= thi) { w.hit = true; w.t = tHit; }
    }
    return w;
}

// The calling lane's pixel of its wave's 8x8 tile and, inside the frame, the pixel's ray (all zero outside).
struct TilePixel {
    int px, py;
    bool in;
    Ray r;
};
__device__ __forceinline__ TilePixel tile_pixel(const RenderParams& P) {
    const int lane = threadIdx.x & 63;
    const int tile = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    const int tx = tile % P.tilesX, ty = tile / P.tilesX;
    TilePixel t;
    t.px = tx * 8 + (lane & 7); t.py = ty * 8 + (lane >> 3);
    t.in = ty < P.tilesY && t.px < P.W && t.py < P.H;
    t.r.ox = t.r.oy = t.r.oz = t.r.dx = t.r.dy = t.r.dz = t.r.ix = t.r.iy = t.r.iz = 0.0f;
    if (t.in) t.r = generate_ray_tab(P, t.px, t.py);
    return t;
}

// The hits of a wave are compacted (one ballot and one atomic per wave; every lane calls): a lane with `need` takes the next
// record, writes its origin so, ndotl, pixel and hash with the family's own words y and w, and zeroes its counter.
__device__ __forceinline__ void lit_append(const LitArgs& L, bool need, int px, int py, unsigned pix, float sx, float sy, float sz,
                                           float ndotl, int y, int w) {
    const int lane = threadIdx.x & 63;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(need);
    if (m == 0ull) return;
    const int leader = __builtin_ctzll(m);
    unsigned base = 0;
    if (lane == leader) base = atomicAdd(L.count, (unsigned)__builtin_popcountll(m));
    base = __shfl(base, leader);
    if (!need) return;
    const unsigned h = lit_mix32(((unsigned)px * 0x8da6b343u) ^ ((unsigned)py * 0xd8163841u) ^ (L.seed * 0xcb1ab31fu));
    const unsigned idx = base + (unsigned)__builtin_popcountll(m & ((1ull << lane) - 1ull));
    L.rec[2 * (size_t)idx] = make_int4(__float_as_int(sx), __float_as_int(sy), __float_as_int(sz), __float_as_int(ndotl));
    L.rec[2 * (size_t)idx + 1] = make_int4((int)pix, y, (int)h, w);
    L.acc[idx] = 0u;
}

// The dense space of a frame's secondary rays: nS shadow rays, one per hit, then from the next multiple of 64 (AO rays never
// share a wave with shadow rays) K AO rays per hit in adjacent lanes.  total + 64 < 2^32: the host bounds pixels * (K + 1) + 128.
struct LitSpace {
    unsigned nS, aoBase, total, stride;
    __device__ __forceinline__ LitSpace(unsigned nh, int shadow, unsigned K)
        : nS(shadow ? nh : 0u), aoBase((nS + 63u) & ~63u), total(aoBase + nh * K), stride(gridDim.x * blockDim.x) {}
    // a wave's next base, one grid further: the step never wraps, a wave whose next base would reach total (or pass 2^32) ends instead
    __device__ __forceinline__ unsigned next(unsigned base) const { return total - base > stride ? base + stride : total; }
};

// Sample s of K of the hit with hash h: its AO table entry, x and y negated by bits 6 and 7 of h.
__device__ __forceinline__ float3 lit_ao_entry(unsigned h, unsigned s, unsigned K) {
    const unsigned e = (h + (unsigned)kLitMaxSamples * s / K) & 63u;
    const float t0 = kAoDirDev[3 * e], t1 = kAoDirDev[3 * e + 1], t2 = kAoDirDev[3 * e + 2];
    return make_float3((h & 64u) ? -t0 : t0, (h & 128u) ? -t1 : t1, t2);
}

// The verdicts of hit `hi` in the wave at `base` (bm: the ballot of its rays that hit), for the lane of ray g: this hit's lanes in
// this wave are [segLo, segHi); the first of them adds the piece (+1 << 16) and the wave's verdicts, and the piece that completes
// the count (shadowPiece: the frame has a shadow piece per hit) shades the pixel.  E: rec, acc, rgba, vis and K.
__device__ __forceinline__ void lit_settle(const LitArgs& E, unsigned K, bool shadowRay, bool shadowPiece, unsigned base, int lane,
                                           unsigned g, unsigned hi, unsigned aoBase, unsigned long long bm) {
    const unsigned first = aoBase + hi * K;                         // its AO rays: [first, first + K)
    unsigned segLo = g, contrib;
    if (shadowRay) {
        contrib = ((bm >> lane) & 1ull) ? 256u : 0u;
    } else {
        segLo = first > base ? first : base;
        const unsigned segHi = first + K < base + 64u ? first + K : base + 64u;
        const unsigned l0 = segLo - base, l1 = segHi - base;
        const unsigned long long mask = (l1 - l0 == 64u ? ~0ull : ((1ull << (l1 - l0)) - 1ull)) << l0;
        contrib = (unsigned)__builtin_popcountll(bm & mask);
    }
    if (g != segLo) return;
    const unsigned pieces = (shadowPiece ? 1u : 0u) + (E.K > 0 ? ((first + K - 1u) >> 6) - (first >> 6) + 1u : 0u);
    const unsigned old = atomicAdd(E.acc + hi, contrib + (1u << 16));
    if ((old >> 16) + 1u != pieces) return;
    const unsigned verdict = (old + contrib) & 0xffffu;
    const int occ = (int)(verdict & 0xffu);
    const bool blocked = (verdict & 256u) != 0;
    const float A = E.K > 0 ? (float)(E.K - occ) / (float)E.K : 1.0f;
    lit_store(E, (unsigned)E.rec[2 * (size_t)hi + 1].x, lit_color(__int_as_float(E.rec[2 * (size_t)hi].w), !blocked, A), occ + (blocked ? 256 : 0));
}

// ---------------------------------------------------------------- the lit render's kernels
__global__ __launch_bounds__(kBlock) void k_lit_primary(RenderParams P, LitArgs L, const uint2* __restrict__ desc) {
    extern __shared__ uint2 lds_stack[];
    uint2* stk;
    unsigned* stkNode;
    desc_stacks(lds_stack, P.depth, stk, stkNode);
    const Geo G = geo_of(P);
    const TilePixel t = tile_pixel(P);
    const Ray r = t.r;
    const DescHit w = rooted_box_walk<kQueryFirst>(P, G, r, 0.0f, kLargestBelow1e30, t.in, L.rootLeaf, L.nodes, desc, stk, stkNode);

    int face = -1;
    float ndotl = 0.0f;
    if (w.hit) {
        face = query_face(G, r, w.x, w.y, w.z, w.size, w.t);
        ndotl = shade_term(P, G, r, w.x, w.y, w.z, w.size);
    }
    const bool cast = L.shadow != 0 && face >= 0 && ndotl > 0.0f;
    const bool need = face >= 0 && (cast || L.K > 0);
    const unsigned pix = (unsigned)t.py * (unsigned)P.W + (unsigned)t.px;   // < 2^32 (lit_check)
    if (t.in && !need) lit_store(L, pix, w.hit ? lit_color(ndotl, true, 1.0f) : make_float4(0.f, 0.f, 0.f, 1.f), w.hit ? 0 : -1);

    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    if (need) {
        // the secondary origin: p in shade_term's operation order, axis a snapped to the leaf's own plane, pushed out by eps
        const float hx = r.ox + r.dx * w.t, hy = r.oy + r.dy * w.t, hz = r.oz + r.dz * w.t;
        const float hm = gmax(gmax(__builtin_fabsf(hx), __builtin_fabsf(hy)), __builtin_fabsf(hz));
        const float eps = G.vs * 1e-3f + hm * 0x1p-18f;
        const int a = face >> 1;
        const bool up = (face & 1) != 0;
        const float ext = (float)w.size * G.vs;
        const float g0 = a == 0 ? G.gx : (a == 1 ? G.gy : G.gz);
        const int c0 = a == 0 ? w.x : (a == 1 ? w.y : w.z);
        const float mn = g0 + (float)c0 * G.vs;
        const float plane = up ? (mn + ext) + eps : mn - eps;
        sx = a == 0 ? plane : hx; sy = a == 1 ? plane : hy; sz = a == 2 ? plane : hz;
    }
    lit_append(L, need, t.px, t.py, pix, sx, sy, sz, ndotl, face | (cast ? 8 : 0), 0);
}

__global__ __launch_bounds__(kBlock) void k_lit_secondary(RenderParams P, LitArgs L, const uint2* __restrict__ desc) {
    extern __shared__ uint2 lds_stack[];
    uint2* stk;
    unsigned* stkNode;
    desc_stacks(lds_stack, P.depth, stk, stkNode);
    const Geo G = geo_of(P);
    const int lane = threadIdx.x & 63;
    const unsigned nh = *L.count;
    const unsigned K = (unsigned)L.K;
    const LitSpace sp(nh, L.shadow, K);
    for (unsigned base = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < sp.total; base = sp.next(base)) {
        const unsigned g = base + lane;
        const bool isShadow = g < sp.nS, isAo = g >= sp.aoBase && g < sp.total;
        unsigned hi = 0, s = 0;
        if (isShadow) hi = g;
        else if (isAo) { hi = (g - sp.aoBase) / K; s = g - sp.aoBase - hi * K; }
        Ray r;
        r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
        bool valid = false;
        float thi = 0.0f;
        if (isShadow || isAo) {
            const int4 o = L.rec[2 * (size_t)hi];
            const int4 b = L.rec[2 * (size_t)hi + 1];
            r.ox = __int_as_float(o.x); r.oy = __int_as_float(o.y); r.oz = __int_as_float(o.z);
            if (isShadow) {
                valid = (b.y & 8) != 0;
                r.dx = P.lightNeg[0]; r.dy = P.lightNeg[1]; r.dz = P.lightNeg[2];
                r.ix = P.lightInv[0]; r.iy = P.lightInv[1]; r.iz = P.lightInv[2];
                thi = kLargestBelow1e30;
            } else {
                valid = true;
                const float3 e = lit_ao_entry((unsigned)b.z, s, K);
                const int face = b.y & 7, a = face >> 1;
                const float u = e.x, v = e.y, n = (face & 1) ? e.z : -e.z;
                r.dx = a == 0 ? n : (a == 1 ? v : u);
                r.dy = a == 0 ? u : (a == 1 ? n : v);
                r.dz = a == 0 ? v : (a == 1 ? u : n);
                r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
                thi = L.radius;
            }
        }
        const DescHit w = rooted_box_walk<kQueryAny>(P, G, r, 0.0f, thi, valid, L.rootLeaf, L.nodes, desc, stk, stkNode);
        const unsigned long long bm = __builtin_amdgcn_ballot_w64(valid && w.hit);
        if (isShadow || isAo) lit_settle(L, K, isShadow, L.shadow != 0, base, lane, g, hi, sp.aoBase, bm);
    }
}

}  // namespace rto

// ---------------------------------------------------------------- host side
static const float kAoDirHost[3 * RTO_AO_MAX_SAMPLES] = { RTO_AO_TABLE };
#undef RTO_AO_TABLE

// The frame's size under a pass of raysPerPixel rays per pixel (perPixel: that factor as the message names it): ray and tile-lane
// indices are 32-bit.
static int frame_bound_check(rto_context* c, const std::string& name, const rto_frame* f, int raysPerPixel, const char* perPixel = "") {
    if (f->width <= 0 || f->height <= 0) return fail(c, RTO_E_INVALID, name + ": width/height must be positive");
    const uint64_t pixels = (uint64_t)f->width * (uint64_t)f->height;
    const uint64_t tileLanes = 64u * (uint64_t)((f->width + 7) / 8) * (uint64_t)((f->height + 7) / 8);
    if (pixels * (uint64_t)raysPerPixel + 128u >= ((uint64_t)1 << 32) || tileLanes + 256u >= ((uint64_t)1 << 32))
        return fail(c, RTO_E_INVALID, name + ": the frame is too large: width * height" + perPixel + " + 128 and 64 lanes per 8x8 "
                                      "tile must stay below 2^32");
    return RTO_OK;
}

// What a frame pass walks: an octree (needGrid: one built from a resident voxel grid) that is one leaf or has a descriptor tree;
// `needs` is the text of the last refusal.
static int frame_tree_check(rto_context* c, const std::string& name, bool needGrid, const char* needs) {
    if (c->numNodes <= 0) return fail(c, RTO_E_NO_OCTREE, name + ": no octree uploaded");
    if (needGrid && !c->d_vox) return fail(c, RTO_E_UNSUPPORTED, name + ": the octree came from rto_upload_octree: no voxel grid is resident");
    if (c->numNodes > 1 && !(c->canonical && c->numInternal > 0)) return fail(c, RTO_E_UNSUPPORTED, name + needs);
    return RTO_OK;
}

static int lit_check(rto_context* c, const char* fn, const rto_frame* f, const rto_lighting* L, const void* rgba) {
    const std::string name(fn);
    if (!f || !L || !rgba) return fail(c, RTO_E_INVALID, name + ": NULL frame, lighting or output");
    if (L->reserved != 0) return fail(c, RTO_E_INVALID, name + ": lighting.reserved must be 0");
    if (L->ao_samples < 0 || L->ao_samples > RTO_AO_MAX_SAMPLES)
        return fail(c, RTO_E_INVALID, name + ": ao_samples must be in 0.." + std::to_string(RTO_AO_MAX_SAMPLES));
    if (L->ao_samples > 0 && !(std::isfinite(L->ao_radius) && L->ao_radius > 0.0f))
        return fail(c, RTO_E_INVALID, name + ": ao_radius must be a finite positive number");
    const float* d = L->light_dir;
    if (!(std::isfinite(d[0]) && std::isfinite(d[1]) && std::isfinite(d[2])) || (d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f))
        return fail(c, RTO_E_INVALID, name + ": light_dir must be finite and non-zero");
    const rtmath::vec3 l = rtmath::normalize(rtmath::vec3(d[0], d[1], d[2]));
    if (!(std::isfinite(l.x) && std::isfinite(l.y) && std::isfinite(l.z)) || (l.x == 0.0f && l.y == 0.0f && l.z == 0.0f))
        return fail(c, RTO_E_INVALID, name + ": light_dir cannot be normalised in float");
    const int rc = frame_bound_check(c, name, f, L->ao_samples + 1, " * (ao_samples + 1)");
    if (rc != RTO_OK) return rc;
    return frame_tree_check(c, name, false, ": the lit render needs a canonical octree (descriptor tree); this array was uploaded in another order");
}

// The work buffers of a lit frame of `pixels` pixels (32-byte records, verdict counters, the hit count), kept on the context and
// grown with the frame; the triangle form (rto_tri_lit.inc) shares them: its records are 32 bytes too.
static int lit_reserve(rto_context* c, const char* fn, size_t pixels, hipStream_t s) {
    if (c->litCap < pixels || !c->d_litCount) {
        if (stream_is_capturing(s))
            return fail(c, RTO_E_UNSUPPORTED, std::string(fn) + ": a larger frame allocates its work buffers; render one such frame "
                                              "before hipStreamBeginCapture");
        (void)hipFree(c->d_litRec); c->d_litRec = nullptr;           // hipFree waits for the device: no frame still reads them
        (void)hipFree(c->d_litAcc); c->d_litAcc = nullptr;
        c->litCap = 0;
        RTO_HIP(c, hipMalloc(&c->d_litRec, pixels * 2 * sizeof(int4)));
        RTO_HIP(c, hipMalloc(&c->d_litAcc, pixels * sizeof(unsigned)));
        if (!c->d_litCount) RTO_HIP(c, hipMalloc(&c->d_litCount, sizeof(unsigned)));
        c->litCap = pixels;
    }
    return RTO_OK;
}

// One lit frame of either family on stream s: the light into the frame's parameters, the work buffers (`fn` names the family in
// their refusal), the zeroed hit count, then primary(grid, block, lds, P, A) over the frame's tiles and, where a term asks for
// rays, secondary(grid, block, lds, P, A) with persistent waves over the most rays the frame can have.
template <class Primary, class Secondary>
static int render_lit_frame(rto_context* c, const char* fn, const rto_frame* f, const rto_lighting* Lt, float4* d_rgba, int32_t* d_vis,
                            hipStream_t s, Primary primary, Secondary secondary) {
    RenderParams P;
    int rc = fill_params(c, f, nullptr, P, s);
    if (rc != RTO_OK) return rc;
    const rtmath::vec3 l = rtmath::normalize(rtmath::vec3(Lt->light_dir[0], Lt->light_dir[1], Lt->light_dir[2]));   // fill_params' order
    P.lightNeg[0] = -l.x; P.lightNeg[1] = -l.y; P.lightNeg[2] = -l.z;
    for (int a = 0; a < 3; a++) { const volatile float q = 1.0f / P.lightNeg[a]; P.lightInv[a] = q; }
    const size_t pixels = (size_t)P.W * (size_t)P.H;                 // lit_check bounded pixels * (K + 1) + 128 below 2^32
    if ((rc = lit_reserve(c, fn, pixels, s)) != RTO_OK) return rc;
    LitArgs A;
    A.rec = c->d_litRec; A.acc = c->d_litAcc; A.count = c->d_litCount;
    A.rgba = d_rgba; A.vis = d_vis;
    A.shadow = Lt->shadow != 0 ? 1 : 0;
    A.K = Lt->ao_samples;
    A.radius = std::min(Lt->ao_radius, kLargestBelow1e30);
    A.seed = Lt->seed;
    A.rootLeaf = c->numNodes == 1 ? 1 : 0;
    A.nodes = c->d_nodes;
    const size_t lds = desc_stack_bytes(P.depth);
    RTO_HIP(c, hipMemsetAsync(c->d_litCount, 0, sizeof(unsigned), s));
    const int64_t tiles = (int64_t)P.tilesX * P.tilesY;
    primary(dim3((unsigned)((tiles + kBlock / kWave - 1) / (kBlock / kWave))), dim3(kBlock), lds, P, A);
    RTO_HIP(c, hipGetLastError());
    if (A.shadow || A.K > 0) {
        const int64_t most = (int64_t)pixels * (A.K + A.shadow) + 64;
        const int64_t blocks = std::min<int64_t>((int64_t)c->numCUs * 8, (most + kBlock - 1) / kBlock);
        secondary(dim3((unsigned)blocks), dim3(kBlock), lds, P, A);
        RTO_HIP(c, hipGetLastError());
    }
    return RTO_OK;
}

static int render_lit(rto_context* c, const rto_frame* f, const rto_lighting* Lt, float4* d_rgba, int32_t* d_vis, hipStream_t s) {
    return render_lit_frame(c, "rto_render_lit_device", f, Lt, d_rgba, d_vis, s,
        [&](dim3 grid, dim3 block, size_t lds, const RenderParams& P, const LitArgs& A) { hipLaunchKernelGGL(k_lit_primary, grid, block, lds, s, P, A, c->d_desc); },
        [&](dim3 grid, dim3 block, size_t lds, const RenderParams& P, const LitArgs& A) { hipLaunchKernelGGL(k_lit_secondary, grid, block, lds, s, P, A, c->d_desc); });
}

// One lit entry of the C ABI, in the manner of query_entry: lit_check, then (`tris`) the resident leaf triangles.  A *_device entry
// checks its buffers' alignment and calls render(c, frame, lighting, rgba, vis, stream) on `stream`; a *_host entry (`host`)
// renders on the context's stream into stream-ordered scratch, copies out and waits.
template <class Render>
static int lit_entry(rto_context* c, const char* fn, bool tris, const rto_frame* frame, const rto_lighting* lighting, void* rgba, int32_t* vis,
                     bool host, void* stream, Render render) {
    if (!c) return RTO_E_INVALID;
    int rc = lit_check(c, fn, frame, lighting, rgba);
    if (rc != RTO_OK) return rc;
    if (tris && (!c->d_triOffset || !c->d_tris))
        return fail(c, RTO_E_NO_OCTREE, std::string(fn) + ": no leaf triangles resident (rto_build_leaf_triangles / rto_upload_leaf_triangles)");
    if (!host && ((reinterpret_cast<uintptr_t>(rgba) & 15) || (reinterpret_cast<uintptr_t>(vis) & 3)))
        return fail(c, RTO_E_INVALID, std::string(fn) + ": d_rgba must be 16-byte and d_vis 4-byte aligned");
    RTO_HIP(c, hipSetDevice(c->device));
    if (!host) return render(c, frame, lighting, reinterpret_cast<float4*>(rgba), vis, (hipStream_t)stream);
    const size_t pixels = (size_t)frame->width * (size_t)frame->height;
    BuildScratch scratch(c->stream);
    float4* d_rgba = nullptr;
    int32_t* d_vis = nullptr;
    RTO_HIP(c, scratch.alloc(&d_rgba, pixels));
    if (vis) RTO_HIP(c, scratch.alloc(&d_vis, pixels));
    if ((rc = render(c, frame, lighting, d_rgba, d_vis, c->stream)) != RTO_OK) return rc;
    RTO_HIP(c, hipMemcpyAsync(rgba, d_rgba, pixels * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    if (vis) RTO_HIP(c, hipMemcpyAsync(vis, d_vis, pixels * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    RTO_HIP(c, hipStreamSynchronize(c->stream));
    return RTO_OK;
}

extern "C" {

int rto_ao_directions(float* out) {
    if (!out) return RTO_E_INVALID;
    std::memcpy(out, kAoDirHost, sizeof kAoDirHost);
    return RTO_OK;
}

int rto_render_lit_device(rto_context* c, const rto_frame* frame, const rto_lighting* lighting, void* d_rgba, int32_t* d_vis,
                          void* hip_stream) {
    return lit_entry(c, "rto_render_lit_device", false, frame, lighting, d_rgba, d_vis, false, hip_stream, render_lit);
}

int rto_render_lit_host(rto_context* c, const rto_frame* frame, const rto_lighting* lighting, float* host_rgba, int32_t* host_vis) {
    return lit_entry(c, "rto_render_lit_host", false, frame, lighting, host_rgba, host_vis, true, nullptr, render_lit);
}

}  // extern "C"
