// rto_tri_lit.inc -- the lit render of the triangle surface (include/rto_hip.h, rto_render_lit_triangles_*): the triangle render's
// frame with a shadow ray and ambient occlusion per hit pixel, all on the device.  Included at the end of rto_api.hip, after
// rto_tri_query.inc (TriRule: desc_walk under the triangle rule) and rto_lit.inc.  From rto_lit.inc: LitArgs, lit_color, lit_store,
// the AO table, and the frame pass -- tile_pixel and lit_append in the primary kernel, LitSpace, lit_ao_entry and lit_settle in the
// secondary one, render_lit_frame (the work buffers with it) and lit_entry (the checks with it) on the host.  Its own: the triangle
// rule's walk, the turned normal, the origin, the tangent frame and the shape of k_trilit_secondary.
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
    const TilePixel t = tile_pixel(P);
    const Ray r = t.r;
    // a tree that is one leaf owns no triangles (and has no descriptors): nobody walks
    TriRule R(S.descFirstChild, S.tris, S.triOffset);
    const bool hit = desc_walk<kQueryFirst>(P, G, r, 0.0f, kLargestBelow1e30, t.in && !L.rootLeaf, desc, stk, stkNode, R);

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
    const unsigned pix = (unsigned)t.py * (unsigned)P.W + (unsigned)t.px;   // < 2^32 (lit_check)
    if (t.in && !need) lit_store(L, pix, hit ? lit_color(ndotl, true, 1.0f) : make_float4(0.f, 0.f, 0.f, 1.f), hit ? 0 : -1);

    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    if (need) {
        // the secondary origin, k_trace_triangles' shadow origin: back on the hit triangle's plane, then the offset along n
        const float* v0 = S.tris + (size_t)R.B.tri * 12;
        const float hx = r.ox + r.dx * R.B.t, hy = r.oy + r.dy * R.B.t, hz = r.oz + r.dz * R.B.t;
        const float hm = gmax(gmax(__builtin_fabsf(hx), __builtin_fabsf(hy)), __builtin_fabsf(hz));
        const float hb = (P.voxelSize * 1e-3f + hm * 0x1p-18f) - ((hx - v0[0]) * nx + (hy - v0[1]) * ny + (hz - v0[2]) * nz);
        sx = hx + nx * hb; sy = hy + ny * hb; sz = hz + nz * hb;
    }
    lit_append(L, need, t.px, t.py, pix, sx, sy, sz, ndotl, R.B.tri, (turned ? kTriLitTurned : 0) | (cast ? kTriLitCast : 0));
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
    const LitSpace sp(nh, L.shadow, K);
    const unsigned kNone = ~0u;
    for (unsigned base = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * blockDim.x + (threadIdx.x & ~63u))); base < sp.total;
         base = sp.next(base)) {
        // aoBase is a multiple of 64: a wave holds shadow rays or AO rays, never both
        const bool shadowWave = base < sp.aoBase;
        const unsigned g = base + lane;
        const bool in = g < (shadowWave ? sp.nS : sp.total);
        unsigned hi = g;                                            // the ray's hit record; kNone behind the walk: a lane without a ray
        Ray r;
        r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
        bool valid = false;
        float thi = kLargestBelow1e30;
        if (shadowWave) {
            if (in) {
                const int4 o = L.rec[2 * (size_t)hi];
                r.ox = __int_as_float(o.x); r.oy = __int_as_float(o.y); r.oz = __int_as_float(o.z);
                valid = (L.rec[2 * (size_t)hi + 1].w & kTriLitCast) != 0;
            }
            r.dx = P.lightNeg[0]; r.dy = P.lightNeg[1]; r.dz = P.lightNeg[2];
            r.ix = P.lightInv[0]; r.iy = P.lightInv[1]; r.iz = P.lightInv[2];
        } else {
            hi = (g - sp.aoBase) / K;
            if (in) {
                const unsigned s = g - sp.aoBase - hi * K;
                const int4 o = L.rec[2 * (size_t)hi];
                const int4 b = L.rec[2 * (size_t)hi + 1];
                r.ox = __int_as_float(o.x); r.oy = __int_as_float(o.y); r.oz = __int_as_float(o.z);
                const float3 e = lit_ao_entry((unsigned)b.z, s, K);
                const float tx = e.x, ty = e.y, tz = e.z;
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
        if (hi != kNone) lit_settle(trilit_args_again(), K, shadowWave, sp.aoBase != 0, base, lane, g, hi, sp.aoBase, bm);
    }
}

// trilit_args_again reads offset 0 of the kernel-argument segment as a LitArgs: a reorder of the parameters must not build.
template <class F> struct TriLitFirstParam;
template <class A, class... Rest> struct TriLitFirstParam<void (*)(A, Rest...)> { using type = A; };
static_assert(std::is_same<TriLitFirstParam<decltype(&k_trilit_secondary)>::type, LitArgs>::value,
              "k_trilit_secondary's first parameter must be the LitArgs that trilit_args_again re-reads at offset 0");

}  // namespace rto

// ---------------------------------------------------------------- host side
static int render_tri_lit(rto_context* c, const rto_frame* f, const rto_lighting* Lt, float4* d_rgba, int32_t* d_vis, hipStream_t s) {
    const TriLitScene S{ c->d_descFirstChild, c->d_tris, c->d_triOffset };
    return render_lit_frame(c, "rto_render_lit_triangles_device", f, Lt, d_rgba, d_vis, s,
        [&](dim3 grid, dim3 block, size_t lds, const RenderParams& P, const LitArgs& A) { hipLaunchKernelGGL(k_trilit_primary, grid, block, lds, s, P, A, S, c->d_desc); },
        [&](dim3 grid, dim3 block, size_t lds, const RenderParams& P, const LitArgs& A) { hipLaunchKernelGGL(k_trilit_secondary, grid, block, lds, s, A, P, S, c->d_desc); });
}

extern "C" {

int rto_render_lit_triangles_device(rto_context* c, const rto_frame* frame, const rto_lighting* lighting, void* d_rgba, int32_t* d_vis,
                                    void* hip_stream) {
    return lit_entry(c, "rto_render_lit_triangles_device", true, frame, lighting, d_rgba, d_vis, false, hip_stream, render_tri_lit);
}

int rto_render_lit_triangles_host(rto_context* c, const rto_frame* frame, const rto_lighting* lighting, float* host_rgba,
                                  int32_t* host_vis) {
    return lit_entry(c, "rto_render_lit_triangles_host", true, frame, lighting, host_rgba, host_vis, true, nullptr, render_tri_lit);
}

}  // extern "C"
