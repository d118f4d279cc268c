// rto_voxel_walk.inc -- the voxel walk of a frame's pixel rays through an int32 volume of the resident grid, and the brick table that
// lets it skip: what the field projections (rto_project.inc) and the field composites (rto_composite.inc) share.  Included at the
// end of rto_api.hip, after rto_field_view.inc (work_buffer) and ahead of the two.
//
// Rule (DESIGN.md section 28).  The planes of a moving axis a are P(j) = gridMin[a] + (float)j * voxelSize, j = 0 .. dim[a], met at
// T(j) = (P(j) - o[a]) * inv[a]; the events are the planes with T > 0 in (T, axis) order, one axis' equal T in its direction of
// travel; the walk is the start state and the state after every event; the visited voxels are the states inside the box.  Floats
// decide that set and nothing else.  The kernel never sorts: T is monotone along an axis, so the walk is a merge of three sorted
// sequences, a state is found by rank (how many planes of an axis are ordered before a key) and a brick is left by its smallest
// leaving plane.
//
//   k_project_bricks  one wave per run of 8 bricks along x: lane l reads column x = 64 run + l of the run's 8 x 8 (y, z) rows (256
//                     bytes a load, the volume once), keeps the largest key and the largest ~key of its valued voxels, and groups
//                     of 8 lanes fold them (lane_xor) into one 8-byte record per brick; 0 = no valued voxel.
//   VoxelWalk         one pixel's walk: enter() by rank, then per trip leave_brick() or step(), and advance().  A march keeps its
//                     own loop: what it does with a brick's record, what it does with a voxel, and when it stops.

namespace rto {

constexpr unsigned kProjectStill = 0x7fffffffu;      // the "next event" of an axis that has none: above the bits of every T > 0

// The grid and box part of a march's arguments (walk_box fills it).
struct WalkBox {
    const int* volume;       // dimZ x dimY x dimX, x fastest
    int dim[3];
    int lo[3], hi[3];        // the box [lo, hi): the clip box or the grid
    int nbx, nby;            // bricks along x and y
    int validLo, validHi;
    int useTable;            // 0: rto_debug_set_projection_table(ctx, 0), no brick is skipped
    const uint2* bricks;     // (largest key, largest ~key) per brick
};

__global__ __launch_bounds__(kBlock) void k_project_bricks(const int* __restrict__ volume, int dimX, int dimY, int dimZ, int nbx, int nby,
                                                           int runsX, unsigned waves, int validLo, int validHi, uint2* __restrict__ bricks) {
    const unsigned w = blockIdx.x * (unsigned)(kBlock / kWave) + (threadIdx.x >> 6);      // wave-uniform
    if (w >= waves) return;
    const int lane = threadIdx.x & 63;
    const int rx = (int)(w % (unsigned)runsX);
    const unsigned row = w / (unsigned)runsX;
    const int by = (int)(row % (unsigned)nby), bz = (int)(row / (unsigned)nby);
    const int x = rx * 64 + lane;
    const int y1 = min(by * 8 + 8, dimY), z1 = min(bz * 8 + 8, dimZ);
    unsigned kMax = 0u, kInv = 0u;
    if (x < dimX) {
        const int outside = validLo - 1;                 // representable (valid_lo > INT32_MIN + 1) and not valued
        for (int z = bz * 8; z < z1; z++) {
            const int* row = volume + ((size_t)z * (size_t)dimY + (size_t)(by * 8)) * (size_t)dimX + (size_t)x;
            int v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = by * 8 + k < y1 ? row[(size_t)k * (size_t)dimX] : outside;   // eight loads in flight
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const bool valued = v[k] >= validLo && v[k] <= validHi;
                const unsigned key = (unsigned)v[k] ^ 0x80000000u;
                kMax = valued && key > kMax ? key : kMax;
                kInv = valued && ~key > kInv ? ~key : kInv;
            }
        }
    }
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) {              // the 8 lanes of a brick
        const unsigned a = lane_xor(kMax, off), b = lane_xor(kInv, off);
        kMax = a > kMax ? a : kMax;
        kInv = b > kInv ? b : kInv;
    }
    const int bx = rx * 8 + (lane >> 3);
    if ((lane & 7) == 0 && bx < nbx) bricks[((size_t)bz * (size_t)nby + (size_t)by) * (size_t)nbx + (size_t)bx] = make_uint2(kMax, kInv);
}

// One axis of a pixel's walk.  A moving axis at coordinate c meets plane c + up next, at `next` (the bits of its T, which is
// positive: unsigned order is float order); a still axis never moves and holds kProjectStill.
struct ProjectAxis {
    float o, inv, g;
    int dim, lo, hi;
    int c, up, step;
    unsigned next;
    bool moving;
};

// T of plane j: one convert, multiply, add, subtract, multiply
__device__ __forceinline__ float project_t(const ProjectAxis& A, float vs, int j) { return ((A.g + (float)j * vs) - A.o) * A.inv; }

__device__ __forceinline__ void project_arm(ProjectAxis& A, float vs) {
    A.next = A.moving ? __float_as_uint(project_t(A, vs, A.c + A.up)) : kProjectStill;
}

__device__ __forceinline__ void project_step(ProjectAxis& A, float vs) {
    A.c += A.step;
    project_arm(A, vs);
}

// How many planes of a moving axis, in its direction of travel, come before the key: T <= t when incl, else T < t.  T is
// monotone in that direction, so the count is a binary search.
__device__ __forceinline__ int project_rank(const ProjectAxis& A, float vs, float t, bool incl) {
    int a = 0, b = A.dim + 1;
    while (a < b) {
        const int mid = (a + b) >> 1;
        const float tm = project_t(A, vs, A.up ? mid : A.dim - mid);
        if (incl ? tm <= t : tm < t) a = mid + 1; else b = mid;
    }
    return a;
}

// The axis before the walk: what it is, the T of the planes that bring it into the box and out of it, and whether it can be
// inside at all (a still axis: its one coordinate; a moving one: the leaving plane still ahead).
__device__ __forceinline__ bool project_axis_init(ProjectAxis& A, float vs, float o, float inv, float g, int dim, int lo, int hi,
                                                  float& tIn, float& tOut, bool& needIn) {
    A.o = o; A.inv = inv; A.g = g; A.dim = dim; A.lo = lo; A.hi = hi;
    A.moving = __builtin_isfinite(inv);
    A.up = inv > 0.0f ? 1 : 0;
    A.step = A.moving ? (A.up ? 1 : -1) : 0;
    A.c = 0; A.next = kProjectStill;
    tIn = tOut = 0.0f; needIn = false;
    if (!A.moving) {
        const float q = __builtin_floorf((o - g) / vs);
        const bool in = q >= (float)lo && q < (float)hi;
        if (in) A.c = (int)q;
        return in;
    }
    tIn = project_t(A, vs, A.up ? lo : hi);
    tOut = project_t(A, vs, A.up ? hi : lo);
    needIn = tIn > 0.0f;
    return tOut > 0.0f;
}

__device__ __forceinline__ bool project_inside(const ProjectAxis& A) { return A.c >= A.lo && A.c < A.hi; }

// The plane through which a moving axis leaves its brick, and the coordinate behind it.
__device__ __forceinline__ int project_brick_exit(const ProjectAxis& A) {
    const int b = A.c >> 3;
    return A.up ? min(b * 8 + 8, A.dim) : b * 8;
}

// Axis B, which is not the axis of the key (t, B before the key's axis when `first`), crosses every plane ordered before the key.
// Inside a brick that is at most 7 planes.
__device__ __forceinline__ void project_catch_up(ProjectAxis& B, float vs, unsigned t, bool first) {
    for (int i = 0; i < 8 && (B.next < t || (first && B.next == t)); i++) project_step(B, vs);
}

// One pixel's walk.
struct VoxelWalk {
    ProjectAxis X, Y, Z;
    int nbx, nby;
    int budget;              // no walk has more states: a loop that cannot hang whatever the floats do

    // The start state; false: the pixel is a miss, no voxel is visited.
    __device__ __forceinline__ bool enter(const Geo& G, const Ray& r, bool inFrame, const WalkBox& B) {
        float inX, inY, inZ, outX, outY, outZ;
        bool needX, needY, needZ;
        bool alive = inFrame && __builtin_isfinite(r.ox) && __builtin_isfinite(r.oy) && __builtin_isfinite(r.oz);
        const bool okX = project_axis_init(X, G.vs, r.ox, r.ix, G.gx, B.dim[0], B.lo[0], B.hi[0], inX, outX, needX);
        const bool okY = project_axis_init(Y, G.vs, r.oy, r.iy, G.gy, B.dim[1], B.lo[1], B.hi[1], inY, outY, needY);
        const bool okZ = project_axis_init(Z, G.vs, r.oz, r.iz, G.gz, B.dim[2], B.lo[2], B.hi[2], inZ, outZ, needZ);
        alive = alive && okX && okY && okZ && (X.moving || Y.moving || Z.moving);
        // the entry: the largest entering event in (T, axis) order (axis 3, T 0: none, the walk starts inside); it must come before
        // every other axis' leaving event
        float eT = 0.0f;
        int eAxis = 3;
        if (needX) { eT = inX; eAxis = 0; }
        if (needY && (eAxis == 3 || inY >= eT)) { eT = inY; eAxis = 1; }
        if (needZ && (eAxis == 3 || inZ >= eT)) { eT = inZ; eAxis = 2; }
        if (eAxis != 3) {
            if (X.moving && eAxis != 0) alive = alive && eT < outX;                       // x comes before the entry's axis on a tie
            if (Y.moving && eAxis != 1) alive = alive && (eT < outY || (eT == outY && eAxis < 1));
            if (Z.moving && eAxis != 2) alive = alive && (eT < outZ || (eT == outZ && eAxis < 2));
        }
        if (alive) {
            if (X.moving) { X.c = eAxis == 0 ? (X.up ? X.lo : X.hi - 1) : (X.up ? project_rank(X, G.vs, eT, 0 < eAxis) - 1 : X.dim - project_rank(X, G.vs, eT, 0 < eAxis)); }
            if (Y.moving) { Y.c = eAxis == 1 ? (Y.up ? Y.lo : Y.hi - 1) : (Y.up ? project_rank(Y, G.vs, eT, 1 < eAxis) - 1 : Y.dim - project_rank(Y, G.vs, eT, 1 < eAxis)); }
            if (Z.moving) { Z.c = eAxis == 2 ? (Z.up ? Z.lo : Z.hi - 1) : (Z.up ? project_rank(Z, G.vs, eT, 2 < eAxis) - 1 : Z.dim - project_rank(Z, G.vs, eT, 2 < eAxis)); }
            project_arm(X, G.vs); project_arm(Y, G.vs); project_arm(Z, G.vs);
            alive = project_inside(X) && project_inside(Y) && project_inside(Z);
        }
        nbx = B.nbx; nby = B.nby;
        budget = B.dim[0] + B.dim[1] + B.dim[2] + 4;
        return alive;
    }

    __device__ __forceinline__ int brick() const { return ((Z.c >> 3) * nby + (Y.c >> 3)) * nbx + (X.c >> 3); }
    __device__ __forceinline__ int voxel() const { return (Z.c * Y.dim + Y.c) * X.dim + X.c; }      // < 2^31 (the family's check)

    // The brick's exit event: the smallest (T, axis) among its leaving planes; the other axes cross what comes before it.  On copies
    // of the axes: the three arms end alike, and merged through `this` ahead of inlining they would keep the axes in memory.
    __device__ __forceinline__ void leave_brick(float vs) {
        ProjectAxis x = X, y = Y, z = Z;
        const int jx = project_brick_exit(x), jy = project_brick_exit(y), jz = project_brick_exit(z);
        const unsigned tx = x.moving ? __float_as_uint(project_t(x, vs, jx)) : kProjectStill;
        const unsigned ty = y.moving ? __float_as_uint(project_t(y, vs, jy)) : kProjectStill;
        const unsigned tz = z.moving ? __float_as_uint(project_t(z, vs, jz)) : kProjectStill;
        if (tx <= ty && tx <= tz) {
            project_catch_up(y, vs, tx, false); project_catch_up(z, vs, tx, false);
            x.c = x.up ? jx : jx - 1; project_arm(x, vs);
        } else if (ty <= tz) {
            project_catch_up(x, vs, ty, true); project_catch_up(z, vs, ty, false);
            y.c = y.up ? jy : jy - 1; project_arm(y, vs);
        } else {
            project_catch_up(x, vs, tz, true); project_catch_up(y, vs, tz, true);
            z.c = z.up ? jz : jz - 1; project_arm(z, vs);
        }
        X = x; Y = y; Z = z;
    }

    // The next event of the three.
    __device__ __forceinline__ void step(float vs) {
        if (X.next <= Y.next && X.next <= Z.next) project_step(X, vs);
        else if (Y.next <= Z.next) project_step(Y, vs);
        else project_step(Z, vs);
    }

    // Is the new state a voxel of the walk?
    __device__ __forceinline__ bool advance() { return project_inside(X) && project_inside(Y) && project_inside(Z) && --budget > 0; }
};

}  // namespace rto

// ---------------------------------------------------------------- host side
constexpr const char* kBrickTableRefusal = ": a larger grid allocates the brick table; project one frame of it before hipStreamBeginCapture";

static int walk_nbz(const WalkBox& B) { return (B.dim[2] + 7) / 8; }

// The box of a frame's marches from the context and the family's struct V (clip, clip_lo, clip_hi, valid_lo, valid_hi), with the
// brick table reserved: it is kept on the context, grows with the grid, and a call that grows it must not be stream-captured.
// The projections' timer is made with it, for a composite too: the other family's first frame of the grid may then be captured.
template <class V>
static int walk_box(rto_context* c, const char* fn, const V* v, const int* volume, hipStream_t s, WalkBox& B) {
    B.volume = volume;
    for (int a = 0; a < 3; a++) {
        B.dim[a] = c->voxDim[a];
        B.lo[a] = v->clip ? v->clip_lo[a] : 0;
        B.hi[a] = v->clip ? v->clip_hi[a] : c->voxDim[a];
    }
    B.nbx = (B.dim[0] + 7) / 8; B.nby = (B.dim[1] + 7) / 8;
    B.validLo = v->valid_lo; B.validHi = v->valid_hi;
    B.useTable = c->pjTable ? 1 : 0;
    int rc = work_buffer(c, c->d_pjBricks, c->pjBrickCap, (size_t)B.nbx * (size_t)B.nby * (size_t)walk_nbz(B), s, fn, kBrickTableRefusal);
    if (rc == RTO_OK) rc = stage_events(c, c->pjEv, s, fn, kBrickTableRefusal);
    B.bricks = c->d_pjBricks;
    return rc;
}

// The frame's brick table, which walk_box reserved: k_project_bricks over the whole grid.
static hipError_t walk_bricks_launch(rto_context* c, const WalkBox& B, hipStream_t s) {
    const int runsX = (B.nbx + 7) / 8;
    const int64_t waves = (int64_t)runsX * B.nby * walk_nbz(B);     // < 2^31 / 512 + ...: the grid has fewer than 2^31 voxels
    const dim3 grid((unsigned)((waves + kBlock / kWave - 1) / (kBlock / kWave)));
    hipLaunchKernelGGL(k_project_bricks, grid, dim3(kBlock), 0, s, B.volume, B.dim[0], B.dim[1], B.dim[2], B.nbx, B.nby, runsX, (unsigned)waves,
                       B.validLo, B.validHi, c->d_pjBricks);
    return hipGetLastError();
}
