// rto_mesh.inc -- mesh extraction (include/rto_hip.h, rto_extract_mesh): the triangle list the reference's renderOctree
// (453-skeleton/main.cpp:95-208) makes for its MarchingCubes and VoxelCube display modes -- a depth-first walk that drops every
// subtree whose box fails Frustum::testAABB and runs a Renderer on every surviving leaf -- from the resident octree, without a walk.
// Included at the end of rto_api.hip.
//
// Rule (DESIGN.md section 16).  A leaf is emitted when its box and every ancestor's pass node_visible() (testAABB != -1 on the
// planes and margin given; no planes: every leaf).  MC: the leaf's resident triangles, unchanged.  CUBES: addBlockFaces
// (453-skeleton/Renderer.cpp:64-98) on a solid leaf -- faces +X, -X, +Y, -Y, +Z, -Z, each exposed when the ONE voxel beyond its
// centre is outside the grid's dims or EMPTY -- two triangles per face.  Order: depth first, children in slots 0..7.
//
// Shape.  (1) One thread per node counts what its leaf emits; the ancestors of a leaf are its own corner with the low bits
// cleared, so the whole chain of box tests is ALU work.  (2) The array stores the tree level by level and the 8 children of a node
// side by side: one launch per level bottom-up sums every node's children, one per level top-down hands every child its parent's
// offset plus its earlier siblings' sums -- a depth-first ranking with no sort.  (3) MC: one thread per resident triangle finds its
// leaf in tri_offset and copies three float4; CUBES: one thread per leaf writes its faces.  No atomics decide the order.

namespace rto {

struct MeshLevels {
    int start[kMaxDepth + 2];      // first node of level l (size rootSize >> l); -1: no such level
    int unordered;                 // 1: the sizes do not fall monotonically along the array
};

// Where the levels begin.  Both entry points' arrays list the root, then its children, then theirs: sizes never grow along the array.
__global__ __launch_bounds__(kBlock) void k_mesh_levels(const rto_node* __restrict__ nodes, int64_t n, int rootSize, MeshLevels* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int size = nodes[i].size;
    const int prev = i > 0 ? nodes[i - 1].size : 0x7fffffff;
    if (size == prev) return;
    const int level = __clz(size) - __clz(rootSize);
    if (size > prev || size <= 0 || level < 0 || level > kMaxDepth) out->unordered = 1;
    else out->start[level] = (int)i;
}

struct MeshParams {
    CullParams C;
    int cull;                      // 0: every leaf is visible
    int rootSize;
    int dimX, dimY, dimZ;          // CUBES: the resident grid's dims
};

// renderOctree's descent seen from the leaf: its box, then the boxes of edge 2 size, 4 size, .. rootSize that hold it.
__device__ __forceinline__ bool mesh_chain_visible(const CullParams& C, int x, int y, int z, int size, int rootSize) {
    bool vis = node_visible(C, x, y, z, size);
    for (int s = size << 1; vis && s <= rootSize; s <<= 1) {
        const int m = ~(s - 1);
        vis = node_visible(C, x & m, y & m, z & m, s);
    }
    return vis;
}

// checkFace (Renderer.cpp:77-82): outside the dims or EMPTY
__device__ __forceinline__ unsigned mesh_face_open(const MeshParams& P, const uint8_t* __restrict__ vox, int x, int y, int z) {
    if (x < 0 || y < 0 || z < 0 || x >= P.dimX || y >= P.dimY || z >= P.dimZ) return 1u;
    return vox[((size_t)z * P.dimY + y) * (size_t)P.dimX + x] == 0 ? 1u : 0u;
}

constexpr unsigned kMeshTooMany = 0x80000000u;       // a subtree's sum saturates here: more than 2^31 - 1 triangles is refused
constexpr unsigned kMeshNoOffset = 0xffffffffu;      // off[] of a node the top-down pass never reached (no real offset: the total is below 2^31)

// One thread per node: the triangles its leaf emits (0 for every other node; the ranking passes overwrite the internal ones).
// It also starts the offsets: 0 at the root, kMeshNoOffset everywhere else.  Only k_mesh_offset_level replaces that mark, and it
// descends from the root through nodes that are not terminal, so a leaf that the array holds but the tree does not reach -- the
// canonical check looks at every internal node's children, not at reachability -- keeps it and is skipped by the emit kernels: its
// count is in no ancestor's sum, hence not in the buffer's size.
template <int KIND>
__global__ __launch_bounds__(kBlock) void k_mesh_count(MeshParams P, const rto_node* __restrict__ nodes, int64_t n, const int* __restrict__ triOffset,
                                                      const uint8_t* __restrict__ vox, unsigned* __restrict__ cnt, unsigned* __restrict__ off,
                                                      uint8_t* __restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const rto_node* nd = nodes + i;
    const int x = nd->x, y = nd->y, z = nd->z, size = nd->size;
    unsigned c = 0u, m = 0u;
    if (nd->isLeaf == 1) {
        if (KIND == RTO_MESH_MC) c = (unsigned)(triOffset[i + 1] - triOffset[i]);
        else if (nd->isSolid == 1) {
            const int h = size / 2;
            m = mesh_face_open(P, vox, x + size, y + h, z + h) | mesh_face_open(P, vox, x - 1, y + h, z + h) << 1 |
                mesh_face_open(P, vox, x + h, y + size, z + h) << 2 | mesh_face_open(P, vox, x + h, y - 1, z + h) << 3 |
                mesh_face_open(P, vox, x + h, y + h, z + size) << 4 | mesh_face_open(P, vox, x + h, y + h, z - 1) << 5;
            c = 2u * (unsigned)__popc(m);
        }
        if (c != 0u && P.cull != 0 && !mesh_chain_visible(P.C, x, y, z, size, P.rootSize)) { c = 0u; m = 0u; }
    }
    cnt[i] = c;
    off[i] = i == 0 ? 0u : kMeshNoOffset;
    if (KIND == RTO_MESH_CUBES) mask[i] = (uint8_t)m;
}

// Bottom-up, one level: an internal node's count = the sum of its 8 children (side by side), in 64 bits, saturated.
__global__ __launch_bounds__(kBlock) void k_mesh_sum_level(const rto_node* __restrict__ nodes, int first, int count, unsigned* __restrict__ cnt) {
    const int j = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (j >= count) return;
    const rto_node* nd = nodes + first + j;
    if (nd->isLeaf == 1 || nd->isUniform == 1) return;
    const unsigned* ch = cnt + nd->child[0];
    unsigned long long s = 0ull;
#pragma unroll
    for (int k = 0; k < 8; k++) s += ch[k];
    cnt[first + j] = s > (unsigned long long)kMeshTooMany ? kMeshTooMany : (unsigned)s;
}

// Top-down, one level: child k starts where its parent does, after its siblings 0 .. k - 1.
__global__ __launch_bounds__(kBlock) void k_mesh_offset_level(const rto_node* __restrict__ nodes, int first, int count, const unsigned* __restrict__ cnt,
                                                             unsigned* __restrict__ off) {
    const int j = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (j >= count) return;
    const rto_node* nd = nodes + first + j;
    if (nd->isLeaf == 1 || nd->isUniform == 1) return;
    const int c0 = nd->child[0];
    unsigned base = off[first + j];
    if (base == kMeshNoOffset) return;                  // an internal node the tree does not reach: its subtree keeps the mark
#pragma unroll
    for (int k = 0; k < 8; k++) {
        off[c0 + k] = base;
        base += cnt[c0 + k];
    }
}

// MC: one thread per resident triangle.  Its leaf is the last node whose range starts at or before it; a leaf that emits copies
// its range to off[leaf], three 16-byte loads and stores per triangle.
__global__ __launch_bounds__(kBlock) void k_mesh_emit_mc(const float4* __restrict__ src, const int* __restrict__ triOffset, const rto_node* __restrict__ nodes, int numNodes,
                                                        int numTris, const unsigned* __restrict__ cnt, const unsigned* __restrict__ off,
                                                        float4* __restrict__ dst, int* __restrict__ triNode) {
    const int t = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (t >= numTris) return;
    int lo = 0, hi = numNodes;                         // the first p with triOffset[p] > t: in [1, numNodes]
    while (lo < hi) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (triOffset[mid] > t) hi = mid; else lo = mid + 1;
    }
    const int leaf = lo - 1;
    if (cnt[leaf] == 0u || nodes[leaf].isLeaf != 1) return;      // culled, or an uploaded range on a node that is no leaf
    const unsigned base = off[leaf];
    if (base == kMeshNoOffset) return;                           // a leaf the tree does not reach
    const size_t d = (size_t)base + (size_t)(t - triOffset[leaf]);
    const float4 a = src[3 * (size_t)t], b = src[3 * (size_t)t + 1], c = src[3 * (size_t)t + 2];
    dst[3 * d] = a; dst[3 * d + 1] = b; dst[3 * d + 2] = c;
    triNode[d] = leaf;
}

// The four corners of a face in addFace*'s order (Renderer.cpp:100-153), 3 bits each (bit a: the max corner's coordinate on
// axis a), v0 lowest; faces +X, -X, +Y, -Y, +Z, -Z.
__device__ __forceinline__ constexpr unsigned mesh_face_corners(int f) {
    return f == 0 ? (1u | 3u << 3 | 7u << 6 | 5u << 9) : f == 1 ? (0u | 4u << 3 | 6u << 6 | 2u << 9) :
           f == 2 ? (2u | 6u << 3 | 7u << 6 | 3u << 9) : f == 3 ? (0u | 1u << 3 | 5u << 6 | 4u << 9) :
           f == 4 ? (4u | 6u << 3 | 7u << 6 | 5u << 9) : (0u | 1u << 3 | 3u << 6 | 2u << 9);
}

// CUBES: one thread per leaf with an exposed face; addQuad(v0, v1, v3, v2): triangles (v0, v1, v3) and (v3, v1, v2).
__global__ __launch_bounds__(kBlock) void k_mesh_emit_cubes(MeshParams P, const rto_node* __restrict__ nodes, int64_t n, const uint8_t* __restrict__ mask,
                                                           const unsigned* __restrict__ off, float4* __restrict__ dst, int* __restrict__ triNode) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const unsigned m = mask[i];
    if (m == 0u || off[i] == kMeshNoOffset) return;              // nothing exposed or culled; or a leaf the tree does not reach
    const rto_node* nd = nodes + i;
    const float vs = P.C.voxelSize;
    const float ext = (float)nd->size * vs;
    const float lo[3] = { P.C.gridMin[0] + (float)nd->x * vs, P.C.gridMin[1] + (float)nd->y * vs, P.C.gridMin[2] + (float)nd->z * vs };
    const float hi[3] = { lo[0] + ext, lo[1] + ext, lo[2] + ext };
    size_t d = off[i];
#pragma unroll
    for (int f = 0; f < 6; f++) {
        if (!((m >> f) & 1u)) continue;
        const unsigned q = mesh_face_corners(f);
        float v[4][3];
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int a = 0; a < 3; a++) v[k][a] = ((q >> (3 * k + a)) & 1u) ? hi[a] : lo[a];
        const float nx = f == 0 ? 1.0f : f == 1 ? -1.0f : 0.0f, ny = f == 2 ? 1.0f : f == 3 ? -1.0f : 0.0f, nz = f == 4 ? 1.0f : f == 5 ? -1.0f : 0.0f;
        float4* o = dst + 3 * d;
        o[0] = make_float4(v[0][0], v[0][1], v[0][2], v[1][0]);
        o[1] = make_float4(v[1][1], v[1][2], v[3][0], v[3][1]);
        o[2] = make_float4(v[3][2], nx, ny, nz);
        o[3] = make_float4(v[3][0], v[3][1], v[3][2], v[1][0]);
        o[4] = make_float4(v[1][1], v[1][2], v[2][0], v[2][1]);
        o[5] = make_float4(v[2][2], nx, ny, nz);
        triNode[d] = (int)i; triNode[d + 1] = (int)i;
        d += 2;
    }
}

}  // namespace rto

// ---------------------------------------------------------------- host side
// First node of every level of the resident array, made once per array (one launch, one small read-back).
static int mesh_levels(rto_context* c, hipStream_t s) {
    if (c->meshLevels > 0) return RTO_OK;
    if (c->numNodes == 1) { c->meshLevelStart[0] = 0; c->meshLevelStart[1] = 1; c->meshLevels = 1; return RTO_OK; }
    rto::MeshLevels L;
    {
        BuildScratch scratch(s);
        rto::MeshLevels* d_levels = nullptr;
        RTO_HIP(c, scratch.alloc(&d_levels, 1));
        RTO_HIP(c, hipMemsetAsync(d_levels, 0xff, sizeof L, s));
        hipLaunchKernelGGL(rto::k_mesh_levels, dim3((unsigned)((c->numNodes + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, c->d_nodes, c->numNodes,
                           c->rootSize, d_levels);
        RTO_HIP(c, hipGetLastError());
        RTO_HIP(c, hipMemcpyAsync(&L, d_levels, sizeof L, hipMemcpyDeviceToHost, s));
        RTO_HIP(c, hipStreamSynchronize(s));
    }
    int levels = 0;
    while (levels <= kMaxDepth && L.start[levels] >= 0) levels++;
    bool ordered = L.unordered != 1 && levels > 0 && L.start[0] == 0;
    for (int l = levels; l <= kMaxDepth; l++) ordered = ordered && L.start[l] < 0;       // no level missing in between
    for (int l = 1; l < levels; l++) ordered = ordered && L.start[l] > L.start[l - 1];
    if (!ordered)
        return fail(c, RTO_E_UNSUPPORTED, "rto_extract_mesh: the array does not store the tree level by level (root, its children, theirs, ...)");
    for (int l = 0; l < levels; l++) c->meshLevelStart[l] = L.start[l];
    c->meshLevelStart[levels] = (int)c->numNodes;
    c->meshLevels = levels;
    return RTO_OK;
}

extern "C" {

int rto_frustum_planes(const float view[16], float fov_deg, float aspect, float planes[24]) {
    if (!view || !planes) return RTO_E_INVALID;
    const rtmath::mat4 proj = rtmath::perspective(rtmath::radians(fov_deg), aspect, 0.01f, 5000.f);
    const rtmath::mat4 vp = proj * rtmath::mat4::from(view);
    rtmath::frustum_planes(vp, planes);
    return RTO_OK;
}

int rto_extract_mesh(rto_context* c, int kind, const rto_mesh_cull* cull, int64_t* num_tris) {
    if (!c) return RTO_E_INVALID;
    if (kind != RTO_MESH_MC && kind != RTO_MESH_CUBES) return fail(c, RTO_E_INVALID, "rto_extract_mesh: unknown kind");
    if (!num_tris) return fail(c, RTO_E_INVALID, "rto_extract_mesh: num_tris is NULL");
    if (cull) {
        bool finite = std::isfinite(cull->margin);
        for (int i = 0; i < 24; i++) finite = finite && std::isfinite(cull->planes[i]);
        if (!finite) return fail(c, RTO_E_INVALID, "rto_extract_mesh: a plane or the margin is not finite");
    }
    if (c->numNodes <= 0) return fail(c, RTO_E_NO_OCTREE, "rto_extract_mesh: no octree uploaded");
    if (!c->canonical && c->numNodes > 1)
        return fail(c, RTO_E_UNSUPPORTED, "rto_extract_mesh: the resident array is not a canonical octree");
    if (kind == RTO_MESH_MC && !c->d_triOffset)
        return fail(c, RTO_E_NO_OCTREE, "rto_extract_mesh: no leaf triangles resident (rto_build_leaf_triangles / rto_upload_leaf_triangles)");
    if (kind == RTO_MESH_CUBES && !c->d_vox)
        return fail(c, RTO_E_UNSUPPORTED, "rto_extract_mesh: the octree came from rto_upload_octree: no voxel grid is resident");
    RTO_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    { const int rc = mesh_levels(c, s); if (rc != RTO_OK) return rc; }
    const int64_t n = c->numNodes;
    const int levels = c->meshLevels;

    rto::MeshParams P;
    std::memset(&P, 0, sizeof P);
    if (cull) { std::memcpy(P.C.planes, cull->planes, sizeof P.C.planes); P.C.margin = cull->margin; P.cull = 1; }
    std::memcpy(P.C.gridMin, c->gridMin, sizeof P.C.gridMin);
    P.C.voxelSize = c->voxelSize;
    P.rootSize = c->rootSize;
    P.dimX = c->voxDim[0]; P.dimY = c->voxDim[1]; P.dimZ = c->voxDim[2];

    // count + cull: events 0 .. 1; ranking passes: events 1 .. 2; emit: events 3 .. 4, begun after the count's read-back and
    // the output buffer's growth, which belong to the call's wall time and to no phase
    StreamEvents<5> events;
    RTO_HIP(c, events.create());

    BuildScratch scratch(s);
    unsigned *d_cnt = nullptr, *d_off = nullptr;
    uint8_t* d_mask = nullptr;
    RTO_HIP(c, scratch.alloc(&d_cnt, (size_t)n));
    RTO_HIP(c, scratch.alloc(&d_off, (size_t)n));
    if (kind == RTO_MESH_CUBES) RTO_HIP(c, scratch.alloc(&d_mask, (size_t)n));
    const unsigned nb = (unsigned)((n + kBlock - 1) / kBlock);

    // ---- count + cull
    RTO_HIP(c, events.record(0, s));
    if (kind == RTO_MESH_MC)
        hipLaunchKernelGGL(rto::k_mesh_count<RTO_MESH_MC>, dim3(nb), dim3(kBlock), 0, s, P, c->d_nodes, n, c->d_triOffset, (const uint8_t*)nullptr, d_cnt, d_off, d_mask);
    else
        hipLaunchKernelGGL(rto::k_mesh_count<RTO_MESH_CUBES>, dim3(nb), dim3(kBlock), 0, s, P, c->d_nodes, n, (const int*)nullptr, c->d_vox, d_cnt, d_off, d_mask);
    RTO_HIP(c, hipGetLastError());
    RTO_HIP(c, events.record(1, s));

    // ---- depth-first ranks: the deepest level holds leaves only
    for (int l = levels - 2; l >= 0; l--) {
        const int first = c->meshLevelStart[l], count = c->meshLevelStart[l + 1] - first;
        hipLaunchKernelGGL(rto::k_mesh_sum_level, dim3((unsigned)((count + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, c->d_nodes, first, count, d_cnt);
    }
    for (int l = 0; l <= levels - 2; l++) {
        const int first = c->meshLevelStart[l], count = c->meshLevelStart[l + 1] - first;
        hipLaunchKernelGGL(rto::k_mesh_offset_level, dim3((unsigned)((count + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, c->d_nodes, first, count, d_cnt, d_off);
    }
    RTO_HIP(c, hipGetLastError());
    RTO_HIP(c, events.record(2, s));
    unsigned total = 0;
    RTO_HIP(c, hipMemcpyAsync(&total, d_cnt, sizeof total, hipMemcpyDeviceToHost, s));     // the one read-back: it sizes the output
    RTO_HIP(c, hipStreamSynchronize(s));
    if (total >= rto::kMeshTooMany) return fail(c, RTO_E_UNSUPPORTED, "rto_extract_mesh: more than 2^31 - 1 triangles");

    // ---- emit into a buffer of the context's own (the previous mesh lives until here)
    if ((int64_t)total > c->meshCap || !c->d_mesh) {
        float4* d_new = nullptr;
        int* d_newNode = nullptr;
        const size_t cap = total ? total : 1;
        RTO_HIP(c, hipMalloc(&d_new, cap * 3 * sizeof(float4)));
        if (hipMalloc(&d_newNode, cap * sizeof(int)) != hipSuccess) { (void)hipFree(d_new); return fail(c, RTO_E_HIP, "rto_extract_mesh: out of device memory"); }
        (void)hipFree(c->d_mesh); (void)hipFree(c->d_meshNode);
        c->d_mesh = d_new; c->d_meshNode = d_newNode; c->meshCap = (int64_t)cap;
    }
    RTO_HIP(c, events.record(3, s));
    if (total > 0) {
        if (kind == RTO_MESH_MC)
            hipLaunchKernelGGL(rto::k_mesh_emit_mc, dim3((unsigned)((c->numTris + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                               reinterpret_cast<const float4*>(c->d_tris), c->d_triOffset, c->d_nodes, (int)n, (int)c->numTris, d_cnt, d_off, c->d_mesh, c->d_meshNode);
        else
            hipLaunchKernelGGL(rto::k_mesh_emit_cubes, dim3(nb), dim3(kBlock), 0, s, P, c->d_nodes, n, d_mask, d_off, c->d_mesh, c->d_meshNode);
        RTO_HIP(c, hipGetLastError());
    }
    RTO_HIP(c, events.record(4, s));
    RTO_HIP(c, hipStreamSynchronize(s));
    c->meshTris = (int64_t)total;
    RTO_HIP(c, events.elapsed(0, 1, &c->meshMs[0]));
    RTO_HIP(c, events.elapsed(1, 2, &c->meshMs[1]));
    RTO_HIP(c, events.elapsed(3, 4, &c->meshMs[2]));
    *num_tris = (int64_t)total;
    return RTO_OK;
}

int rto_mesh_device(rto_context* c, void** d_tris, int32_t** d_tri_node, int64_t* num_tris) {
    if (!c || !num_tris) return RTO_E_INVALID;
    if (c->meshTris < 0) return fail(c, RTO_E_INVALID, "rto_mesh_device: no mesh extracted");
    if (d_tris) *d_tris = c->d_mesh;
    if (d_tri_node) *d_tri_node = c->d_meshNode;
    *num_tris = c->meshTris;
    return RTO_OK;
}

int rto_download_mesh(rto_context* c, float* tris, int64_t capacity, int32_t* tri_node, int64_t* num_tris) {
    if (!c || !num_tris) return RTO_E_INVALID;
    if (c->meshTris < 0) return fail(c, RTO_E_INVALID, "rto_download_mesh: no mesh extracted");
    *num_tris = c->meshTris;
    if (!tris && !tri_node) return RTO_OK;
    if (capacity < c->meshTris) return fail(c, RTO_E_INVALID, "rto_download_mesh: capacity too small");
    if (c->meshTris == 0) return RTO_OK;
    RTO_HIP(c, hipSetDevice(c->device));
    RTO_HIP(c, hipStreamSynchronize(c->stream));
    if (tris) RTO_HIP(c, hipMemcpy(tris, c->d_mesh, (size_t)c->meshTris * 12 * sizeof(float), hipMemcpyDeviceToHost));
    if (tri_node) RTO_HIP(c, hipMemcpy(tri_node, c->d_meshNode, (size_t)c->meshTris * sizeof(int), hipMemcpyDeviceToHost));
    return RTO_OK;
}

int rto_last_mesh_ms(const rto_context* c, float ms[3]) { return copy_last_ms(c, &rto_context::meshMs, ms); }

}  // extern "C"
