// rto_tri_lit.inc -- the lit render of the triangle surface (include/rto_hip.h, rto_render_lit_triangles_*): the triangle render's
// frame with a shadow ray and ambient occlusion per hit pixel, all on the device.  Included at the end of rto_api.hip, after
// rto_tri_query.inc (TriRule: desc_walk under the triangle rule) and rto_lit.inc (LitArgs, lit_color, lit_mix32, the AO table, the
// work buffers and the checks, all shared).
//
// Rule (DESIGN.md section 14).  The primary hit is the FIRST triangle query on the frame's pixel ray; n is the stored face normal
// turned against the ray; the secondary origin is the triangle render's: p = o + d t put back on the triangle's plane and pushed
// out along n, so = p + n (eps - (p - v0) . n), eps = voxelSize 1e-3 + 2^-18 max|p|.  Shadow and AO rays are ANY triangle queries
// from there, (0, 1e30) towards the light and (0, ao_radius] along the table directions carried into the frame (U, V, n) of Duff
// et al.; a secondary ray with a non-finite origin or direction component is a miss.  Colour and vis are the lit render's.
//
// Kernels (one stream, no host step), the shape of rto_lit.inc:
//   k_trilit_primary    one lane per pixel, 8x8 tiles per wave: the FIRST walk, the Lambert term and the secondary origin.  Pixels
//                       without secondary rays are written at once; the others are compacted (one ballot and one atomic per wave)
//                       into 32-byte records {so, ndotl}, {pixel, triangle, hash, turned | shadow cast << 1}.
//   k_trilit_secondary  persistent waves over the dense ray space (shadow rays, then from the next multiple of 64 K AO rays per
//                       hit in adjacent lanes).  An AO lane reloads the stored normal of the record's triangle (12 bytes of a row
//                       the primary walk has just read) and turns it by the record's bit; verdicts are summed per hit in the wave
//                       and added with one atomic per piece; the piece that completes the count shades the pixel.

namespace rto {

struct TriLitScene {
    const int* __restrict__ descFirstChild;
    const float* __restrict__ tris;
    const int* __restrict__ triOffset;
};

constexpr int kTriLitTurned = 1, kTriLitCast = 2;

__device__ __forceinline__ bool trilit_finite3(float x, float y, float z) {
    return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
}

__global__ __launch_bounds__(kBlock) void k_trilit_primary(RenderParams P, LitArgs L, TriLitScene S, const uint2* __restrict__ desc) {
    extern __shared__ uint2 lds_stack[];
    uint2* stk;
    unsigned* stkNode;
    desc_stacks(lds_stack, P.depth, stk, stkNode);
    const Geo G = geo_of(P);
    const int lane = threadIdx.x & 63;
    const int tile = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    const int tx = tile % P.tilesX, ty = tile / P.tilesX;
    const int px = tx * 8 + (lane & 7), py = ty * 8 + (lane >> 3);
    const bool valid = ty < P.tilesY && px < P.W && py < P.H;
    Ray r;
    r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
    if (valid) r = generate_ray_tab(P, px, py);
    // a tree that is one leaf owns no triangles (and has no descriptors): nobody walks
    TriRule R(S.descFirstChild, S.tris, S.triOffset);
    const bool hit = desc_walk<kQueryFirst>(P, G, r, 0.0f, __uint_as_float(0x7149f2c9u), valid && !L.rootLeaf, desc, stk, stkNode, R);

    float nx = 0.0f, ny = 0.0f, nz = 0.0f, ndotl = 0.0f;
    bool turned = false;
    if (hit) {
        const float* T = S.tris + (size_t)R.B.tri * 12;
        nx = T[9]; ny = T[10]; nz = T[11];
        turned = nx * r.dx + ny * r.dy + nz * r.dz > 0.0f;          // the renders' turn (k_trace_triangles)
        if (turned) { nx = -nx; ny = -ny; nz = -nz; }
        ndotl = gmax(0.0f, nx * P.lightNeg[0] + ny * P.lightNeg[1] + nz * P.lightNeg[2]);
    }
    const bool cast = L.shadow != 0 && hit && ndotl > 0.0f;
    const bool need = hit && (cast || L.K > 0);
    const unsigned pix = (unsigned)py * (unsigned)P.W + (unsigned)px;   // < 2^32 (lit_check)
    if (valid && !need) lit_store(L, pix, hit ? lit_color(ndotl, true, 1.0f) : make_float4(0.f, 0.f, 0.f, 1.f), hit ? 0 : -1);

    const unsigned long long m = __builtin_amdgcn_ballot_w64(need);
    if (m == 0ull) return;
    const int leader = __builtin_ctzll(m);
    unsigned base = 0;
    if (lane == leader) base = atomicAdd(L.count, (unsigned)__builtin_popcountll(m));
    base = __shfl(base, leader);
    if (!need) return;
    // the secondary origin, k_trace_triangles' shadow origin: back on the hit triangle's plane, then the offset along n
    const float* v0 = S.tris + (size_t)R.B.tri * 12;
    const float hx = r.ox + r.dx * R.B.t, hy = r.oy + r.dy * R.B.t, hz = r.oz + r.dz * R.B.t;
    const float hm = gmax(gmax(__builtin_fabsf(hx), __builtin_fabsf(hy)), __builtin_fabsf(hz));
    const float hb = (P.voxelSize * 1e-3f + hm * 0x1p-18f) - ((hx - v0[0]) * nx + (hy - v0[1]) * ny + (hz - v0[2]) * nz);
    const float sx = hx + nx * hb, sy = hy + ny * hb, sz = hz + nz * hb;
    const unsigned h = lit_mix32(((unsigned)px * 0x8da6b343u) ^ ((unsigned)py * 0xd8163841u) ^ (L.seed * 0xcb1ab31fu));
    const unsigned idx = base + (unsigned)__builtin_popcountll(m & ((1ull << lane) - 1ull));
    L.rec[2 * (size_t)idx] = make_int4(__float_as_int(sx), __float_as_int(sy), __float_as_int(sz), __float_as_int(ndotl));
    L.rec[2 * (size_t)idx + 1] = make_int4((int)pix, R.B.tri, (int)h, (turned ? kTriLitTurned : 0) | (cast ? kTriLitCast : 0));
    L.acc[idx] = 0u;
}

// The pointers and K of k_trilit_secondary's first argument, read again from the kernel-argument segment (LitArgs is the kernel's first
// parameter: offset 0).  The shading behind the walk is their only other use; held in scalar registers across the walk they were
// spilled, and a volatile read is not hoisted in front of it.
__device__ __forceinline__ LitArgs trilit_args_again() {
    typedef const volatile __attribute__((address_space(4))) LitArgs* KernArgs;
    KernArgs k = (KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
    LitArgs E;
    E.rec = k->rec; E.acc = k->acc; E.rgba = k->rgba; E.vis = k->vis; E.K = k->K;
    return E;
}

__global__ __launch_bounds__(kBlock) void k_trilit_secondary(LitArgs L, RenderParams P, TriLitScene S, const uint2* __restrict__ desc) {
    extern __shared__ uint2 lds_stack[];
    uint2* stk;
    unsigned* stkNode;
    desc_stacks(lds_stack, P.depth, stk, stkNode);
    const Geo G = geo_of(P);
    const int lane = threadIdx.x & 63;
    const unsigned nh = (unsigned)__builtin_amdgcn_readfirstlane((int)*L.count);   // wave-uniform: the ray space's bounds stay in scalar registers
    const unsigned K = (unsigned)L.K;
    const unsigned nS = L.shadow ? nh : 0u;
    const unsigned aoBase = (nS + 63u) & ~63u;                      // AO rays never share a wave with shadow rays
    const unsigned total = aoBase + nh * K;                         // + 64 < 2^32: the host bounds pixels * (K + 1) + 128
    const unsigned stride = gridDim.x * blockDim.x, kNone = ~0u;
    // the step never wraps: a wave whose next base would reach total (or pass 2^32) ends instead
    for (unsigned base = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * blockDim.x + (threadIdx.x & ~63u))); base < total;
         base = total - base > stride ? base + stride : total) {
        // aoBase is a multiple of 64: a wave holds shadow rays or AO rays, never both
        const bool shadowWave = base < aoBase;
        const unsigned g = base + lane;
        const bool in = g < (shadowWave ? nS : total);
        unsigned hi = g;                                            // the ray's hit record; kNone behind the walk: a lane without a ray
        Ray r;
        r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
        bool valid = false;
        float thi = __uint_as_float(0x7149f2c9u);
        if (shadowWave) {
            if (in) {
                const int4 o = L.rec[2 * (size_t)hi];
                r.ox = __int_as_float(o.x); r.oy = __int_as_float(o.y); r.oz = __int_as_float(o.z);
                valid = (L.rec[2 * (size_t)hi + 1].w & kTriLitCast) != 0;
            }
            r.dx = P.lightNeg[0]; r.dy = P.lightNeg[1]; r.dz = P.lightNeg[2];
            r.ix = P.lightInv[0]; r.iy = P.lightInv[1]; r.iz = P.lightInv[2];
        } else {
            hi = (g - aoBase) / K;
            if (in) {
                const unsigned s = g - aoBase - hi * K;
                const int4 o = L.rec[2 * (size_t)hi];
                const int4 b = L.rec[2 * (size_t)hi + 1];
                r.ox = __int_as_float(o.x); r.oy = __int_as_float(o.y); r.oz = __int_as_float(o.z);
                const unsigned h = (unsigned)b.z;
                const unsigned e = (h + (unsigned)kLitMaxSamples * s / K) & 63u;
                const float t0 = kAoDirDev[3 * e], t1 = kAoDirDev[3 * e + 1], tz = kAoDirDev[3 * e + 2];
                const float tx = (h & 64u) ? -t0 : t0, ty = (h & 128u) ? -t1 : t1;
                const float* T = S.tris + (size_t)b.y * 12;
                float nx = T[9], ny = T[10], nz = T[11];
                if (b.w & kTriLitTurned) { nx = -nx; ny = -ny; nz = -nz; }
                // the branch-free orthonormal frame around n (Duff et al.), one operation per operator
                const float sg = nz < 0.0f ? -1.0f : 1.0f;
                const float a = -1.0f / (sg + nz);
                const float bb = (nx * ny) * a;
                const float ux = 1.0f + ((sg * nx) * nx) * a, uy = sg * bb, uz = (-sg) * nx;
                const float vx = bb, vy = sg + (ny * ny) * a, vz = -ny;
                r.dx = (tx * ux + ty * vx) + tz * nx;
                r.dy = (tx * uy + ty * vy) + tz * ny;
                r.dz = (tx * uz + ty * vz) + tz * nz;
                r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
                valid = true;
            }
            thi = L.radius;
        }
        valid = valid && trilit_finite3(r.ox, r.oy, r.oz) && trilit_finite3(r.dx, r.dy, r.dz);
        if (!in) hi = kNone;                                        // fewer than 2^32 - 1 records: the host bounds the frame
        TriRule R(S.descFirstChild, S.tris, S.triOffset);
        const bool hit = desc_walk<kQueryAny>(P, G, r, 0.0f, thi, valid, desc, stk, stkNode, R);      // a lane that is not valid gets a miss
        const unsigned long long bm = __builtin_amdgcn_ballot_w64(hit);
        if (hi == kNone) continue;
        // this hit's lanes in this wave, [segLo, segHi): the first of them adds the piece (+1 << 16) and the wave's verdicts
        const unsigned first = aoBase + hi * K;                     // its AO rays: [first, first + K)
        unsigned segLo = g, contrib;
        if (shadowWave) {
            contrib = ((bm >> lane) & 1ull) ? 256u : 0u;
        } else {
            segLo = first > base ? first : base;
            const unsigned segHi = first + K < base + 64u ? first + K : base + 64u;
            const unsigned l0 = segLo - base, l1 = segHi - base;
            const unsigned long long mask = (l1 - l0 == 64u ? ~0ull : ((1ull << (l1 - l0)) - 1ull)) << l0;
            contrib = (unsigned)__builtin_popcountll(bm & mask);
        }
        if (g != segLo) continue;
        const LitArgs E = trilit_args_again();
        const unsigned pieces = (aoBase ? 1u : 0u) + (E.K > 0 ? ((first + K - 1u) >> 6) - (first >> 6) + 1u : 0u);
        const unsigned old = atomicAdd(E.acc + hi, contrib + (1u << 16));
        if ((old >> 16) + 1u != pieces) continue;
        const unsigned verdict = (old + contrib) & 0xffffu;
        const int occ = (int)(verdict & 0xffu);
        const bool blocked = (verdict & 256u) != 0;
        const float A = E.K > 0 ? (float)(E.K - occ) / (float)E.K : 1.0f;
        lit_store(E, (unsigned)E.rec[2 * (size_t)hi + 1].x, lit_color(__int_as_float(E.rec[2 * (size_t)hi].w), !blocked, A), occ + (blocked ? 256 : 0));
    }
}

// trilit_args_again reads offset 0 of the kernel-argument segment as a LitArgs: a reorder of the parameters must not build.
template <class F> struct TriLitFirstParam;
template <class A, class... Rest> struct TriLitFirstParam<void (*)(A, Rest...)> { using type = A; };
static_assert(std::is_same<TriLitFirstParam<decltype(&k_trilit_secondary)>::type, LitArgs>::value,
              "k_trilit_secondary's first parameter must be the LitArgs that trilit_args_again re-reads at offset 0");

}  // namespace rto

// ---------------------------------------------------------------- host side
static int tri_lit_check(rto_context* c, const char* fn, const rto_frame* f, const rto_lighting* L, const void* rgba) {
    const int rc = lit_check(c, fn, f, L, rgba);
    if (rc != RTO_OK) return rc;
    if (!c->d_triOffset || !c->d_tris)
        return fail(c, RTO_E_NO_OCTREE, std::string(fn) + ": no leaf triangles resident (rto_build_leaf_triangles / rto_upload_leaf_triangles)");
    return RTO_OK;
}

static int render_tri_lit(rto_context* c, const rto_frame* f, const rto_lighting* Lt, float4* d_rgba, int32_t* d_vis, hipStream_t s) {
    RenderParams P;
    int rc = fill_params(c, f, nullptr, P, s);
    if (rc != RTO_OK) return rc;
    const rtmath::vec3 l = rtmath::normalize(rtmath::vec3(Lt->light_dir[0], Lt->light_dir[1], Lt->light_dir[2]));   // fill_params' order
    P.lightNeg[0] = -l.x; P.lightNeg[1] = -l.y; P.lightNeg[2] = -l.z;
    for (int a = 0; a < 3; a++) { const volatile float q = 1.0f / P.lightNeg[a]; P.lightInv[a] = q; }
    const size_t pixels = (size_t)P.W * (size_t)P.H;                 // lit_check bounded pixels * (K + 1) + 128 below 2^32
    if ((rc = lit_reserve(c, "rto_render_lit_triangles_device", pixels, s)) != RTO_OK) return rc;
    LitArgs A;
    A.rec = c->d_litRec; A.acc = c->d_litAcc; A.count = c->d_litCount;
    A.rgba = d_rgba; A.vis = d_vis;
    A.shadow = Lt->shadow != 0 ? 1 : 0;
    A.K = Lt->ao_samples;
    A.radius = std::min(Lt->ao_radius, __builtin_bit_cast(float, 0x7149f2c9u));
    A.seed = Lt->seed;
    A.rootLeaf = c->numNodes == 1 ? 1 : 0;
    A.nodes = c->d_nodes;
    const TriLitScene S{ c->d_descFirstChild, c->d_tris, c->d_triOffset };
    const size_t lds = desc_stack_bytes(P.depth);
    RTO_HIP(c, hipMemsetAsync(c->d_litCount, 0, sizeof(unsigned), s));
    const int64_t tiles = (int64_t)P.tilesX * P.tilesY;
    hipLaunchKernelGGL(k_trilit_primary, dim3((unsigned)((tiles + kBlock / kWave - 1) / (kBlock / kWave))), dim3(kBlock), lds, s, P, A, S, c->d_desc);
    RTO_HIP(c, hipGetLastError());
    if (A.shadow || A.K > 0) {
        const int64_t most = (int64_t)pixels * (A.K + A.shadow) + 64;
        const int64_t blocks = std::min<int64_t>((int64_t)c->numCUs * 8, (most + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(k_trilit_secondary, dim3((unsigned)blocks), dim3(kBlock), lds, s, A, P, S, c->d_desc);
        RTO_HIP(c, hipGetLastError());
    }
    return RTO_OK;
}

extern "C" {

int rto_render_lit_triangles_device(rto_context* c, const rto_frame* frame, const rto_lighting* lighting, void* d_rgba, int32_t* d_vis,
                                    void* hip_stream) {
    if (!c) return RTO_E_INVALID;
    int rc = tri_lit_check(c, "rto_render_lit_triangles_device", frame, lighting, d_rgba);
    if (rc != RTO_OK) return rc;
    if ((reinterpret_cast<uintptr_t>(d_rgba) & 15) || (reinterpret_cast<uintptr_t>(d_vis) & 3))
        return fail(c, RTO_E_INVALID, "rto_render_lit_triangles_device: d_rgba must be 16-byte and d_vis 4-byte aligned");
    RTO_HIP(c, hipSetDevice(c->device));
    return render_tri_lit(c, frame, lighting, reinterpret_cast<float4*>(d_rgba), d_vis, (hipStream_t)hip_stream);
}

int rto_render_lit_triangles_host(rto_context* c, const rto_frame* frame, const rto_lighting* lighting, float* host_rgba,
                                  int32_t* host_vis) {
    if (!c) return RTO_E_INVALID;
    int rc = tri_lit_check(c, "rto_render_lit_triangles_host", frame, lighting, host_rgba);
    if (rc != RTO_OK) return rc;
    return lit_frame_to_host(c, frame, host_rgba, host_vis, [=](float4* d_rgba, int32_t* d_vis) { return render_tri_lit(c, frame, lighting, d_rgba, d_vis, c->stream); });
}

}  // extern "C"
