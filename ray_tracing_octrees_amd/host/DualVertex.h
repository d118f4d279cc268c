// DualVertex.h -- the dual-contouring rule's arithmetic, shared word for word by the CPU form
// (DualContouring.cpp) and the kernels (csrc/rto_dc.inc): the vertex of one voxel and the finish of one triangle.  Restated from the
// reference's gatherHermiteData(size = 1) / calculateIntersection / generateDualVertex / QEFSolver
// (453-skeleton/AdaptiveDualContouringRenderer.cpp:49-161, 1090-1357) and glm 0.9.9.7's operation order.  All floats are float32,
// one IEEE operation per operator, in the order written; both builds pass -ffp-contract=off.  Comparisons the reference makes
// against a double literal are made in double.
//
// `Solid` is any callable bool(int x, int y, int z) that answers false outside the grid.  The points of a voxel are walked twice
// (sums; then the plane or the QEF) instead of being stored: no array is indexed by a variable, so the kernels need no scratch.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define RTO_DC_HD __host__ __device__ __forceinline__
#else
#define RTO_DC_HD inline
#endif

namespace rto_dc {

struct Grid {
    int dimX, dimY, dimZ;
    float minX, minY, minZ;
    float vs;
};

struct V3 { float x, y, z; };

RTO_DC_HD float dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
RTO_DC_HD V3 scale3(V3 a, float s) { return V3{ a.x * s, a.y * s, a.z * s }; }
RTO_DC_HD V3 normalize3(V3 a) { return scale3(a, 1.0f / sqrtf(dot3(a, a))); }                  // glm: v * inversesqrt(dot(v, v))
RTO_DC_HD float fmin2(float x, float y) { return y < x ? y : x; }                             // glm::min
RTO_DC_HD float fmax2(float x, float y) { return x < y ? y : x; }                             // glm::max, std::max
RTO_DC_HD float clamp1(float v, float lo, float hi) { return fmin2(fmax2(v, lo), hi); }

// The Hermite point of the sign change between voxel (x, y, z) and its neighbour along axis d (0, 1, 2); f2: is the neighbour solid.
template <class Solid> RTO_DC_HD void hermite(const Solid& solid, const Grid& g, int x, int y, int z, int d, bool f2, V3* pos, V3* nrm) {
    const int ex = d == 0 ? 1 : 0, ey = d == 1 ? 1 : 0, ez = d == 2 ? 1 : 0;
    const float p1x = g.minX + (float)x * g.vs, p1y = g.minY + (float)y * g.vs, p1z = g.minZ + (float)z * g.vs;
    const float p2x = g.minX + (float)(x + ex) * g.vs, p2y = g.minY + (float)(y + ey) * g.vs, p2z = g.minZ + (float)(z + ez) * g.vs;
    pos->x = p1x + 0.5f * (p2x - p1x); pos->y = p1y + 0.5f * (p2y - p1y); pos->z = p1z + 0.5f * (p2z - p1z);
    // central differences of the +-1 scalar (solid: -1) perpendicular to the edge, at voxel 1
    const float gx = ex ? 0.0f : (solid(x + 1, y, z) ? -1.0f : 1.0f) - (solid(x - 1, y, z) ? -1.0f : 1.0f);
    const float gy = ey ? 0.0f : (solid(x, y + 1, z) ? -1.0f : 1.0f) - (solid(x, y - 1, z) ? -1.0f : 1.0f);
    const float gz = ez ? 0.0f : (solid(x, y, z + 1) ? -1.0f : 1.0f) - (solid(x, y, z - 1) ? -1.0f : 1.0f);
    V3 n{ gx, gy, gz };
    const float fx = (float)ex, fy = (float)ey, fz = (float)ez;
    if ((double)dot3(n, n) < 1e-10) n = V3{ fx, fy, fz };
    else n = normalize3(n);
    const bool withEdge = n.x * fx + n.y * fy + n.z * fz > 0.0f;
    if (withEdge == f2) n = V3{ -n.x, -n.y, -n.z };
    *nrm = n;
}

// Has voxel (x, y, z) at least one Hermite point?  (x, y, z) inside the grid.
template <class Solid> RTO_DC_HD bool has_point(const Solid& solid, const Grid& g, int x, int y, int z) {
    const int x1 = x + 1 < g.dimX - 1 ? x + 1 : g.dimX - 1, y1 = y + 1 < g.dimY - 1 ? y + 1 : g.dimY - 1, z1 = z + 1 < g.dimZ - 1 ? z + 1 : g.dimZ - 1;
    bool any = false;
    for (int zz = z; zz <= z1; zz++)
        for (int yy = y; yy <= y1; yy++)
            for (int xx = x; xx <= x1; xx++) {
                const bool cur = solid(xx, yy, zz);
                if (xx + 1 < g.dimX && solid(xx + 1, yy, zz) != cur) any = true;
                if (yy + 1 < g.dimY && solid(xx, yy + 1, zz) != cur) any = true;
                if (zz + 1 < g.dimZ && solid(xx, yy, zz + 1) != cur) any = true;
            }
    return any;
}

RTO_DC_HD bool entry_ok(float v) { return !__builtin_isnan(v) && !__builtin_isinf(v) && !((double)fabsf(v) > 1e6); }

// What the second walk of a voxel's points does with each of them.
enum { kWalkSums = 0, kWalkPlane = 1, kWalkQef = 2 };

struct Walk {
    int n;                         // points
    V3 mass, avg;                  // kWalkSums: the summed positions and normals
    V3 axis; V3 plane; int planeN; // kWalkPlane: the snapped axis; the summed aligned positions and their number
    float a00, a01, a02, a11, a12, a22;   // kWalkQef: AtA (symmetric: n.x * n.y and n.y * n.x are one product)
    V3 atb;
};

template <int MODE, class Solid> RTO_DC_HD void walk(const Solid& solid, const Grid& g, int x, int y, int z, Walk* w) {
    const int x1 = x + 1 < g.dimX - 1 ? x + 1 : g.dimX - 1, y1 = y + 1 < g.dimY - 1 ? y + 1 : g.dimY - 1, z1 = z + 1 < g.dimZ - 1 ? z + 1 : g.dimZ - 1;
    for (int zz = z; zz <= z1; zz++)
        for (int yy = y; yy <= y1; yy++)
            for (int xx = x; xx <= x1; xx++) {
                const bool cur = solid(xx, yy, zz);
                for (int d = 0; d < 3; d++) {
                    const int nx = xx + (d == 0 ? 1 : 0), ny = yy + (d == 1 ? 1 : 0), nz = zz + (d == 2 ? 1 : 0);
                    if (nx >= g.dimX || ny >= g.dimY || nz >= g.dimZ) continue;
                    const bool nxt = solid(nx, ny, nz);
                    if (cur == nxt) continue;
                    V3 p, n;
                    hermite(solid, g, xx, yy, zz, d, nxt, &p, &n);
                    if (MODE == kWalkSums) {
                        w->mass.x += p.x; w->mass.y += p.y; w->mass.z += p.z;
                        w->avg.x += n.x; w->avg.y += n.y; w->avg.z += n.z;
                        w->n++;
                    } else if (MODE == kWalkPlane) {
                        if (dot3(normalize3(n), w->axis) > 0.7f) {
                            w->plane.x += p.x; w->plane.y += p.y; w->plane.z += p.z;
                            w->planeN++;
                        }
                    } else {
                        const V3 u = normalize3(n);                         // addPoint's second normalisation
                        w->a00 += u.x * u.x; w->a01 += u.x * u.y; w->a02 += u.x * u.z;
                        w->a11 += u.y * u.y; w->a12 += u.y * u.z; w->a22 += u.z * u.z;
                        const float dd = -dot3(u, p);
                        w->atb.x += u.x * dd; w->atb.y += u.y * dd; w->atb.z += u.z * dd;
                    }
                }
            }
}

// Branches of the rule, for the fixture maker's census.
enum { kBranchNoPoint = 0, kBranchFewPoints = 1, kBranchPlane = 2, kBranchQef = 3, kBranchMassPoint = 4 };

// The vertex of voxel (x, y, z), inside the grid.  Returns the number of Hermite points; *branch (may be null) names the way taken.
template <class Solid> RTO_DC_HD int vertex(const Solid& solid, const Grid& g, int x, int y, int z, V3* out, int* branch = nullptr) {
    const V3 centre{ (g.minX + (float)x * g.vs) + 0.5f * g.vs, (g.minY + (float)y * g.vs) + 0.5f * g.vs, (g.minZ + (float)z * g.vs) + 0.5f * g.vs };
    Walk w;
    w.n = 0; w.planeN = 0;
    w.mass = w.avg = w.axis = w.plane = w.atb = V3{ 0.0f, 0.0f, 0.0f };
    w.a00 = w.a01 = w.a02 = w.a11 = w.a12 = w.a22 = 0.0f;
    walk<kWalkSums>(solid, g, x, y, z, &w);
    if (w.n == 0) {
        *out = centre;
        if (branch) *branch = kBranchNoPoint;
        return 0;
    }
    const float half = g.vs * 0.5f, inset = g.vs * 0.001f;
    const V3 lo{ (centre.x - half) + inset, (centre.y - half) + inset, (centre.z - half) + inset };
    const V3 hi{ (centre.x + half) - inset, (centre.y + half) - inset, (centre.z + half) - inset };
    const float fn = (float)w.n;
    const V3 mass{ w.mass.x / fn, w.mass.y / fn, w.mass.z / fn };
    V3 avg = w.avg;
    if (sqrtf(dot3(avg, avg)) > 0.0001f) {
        avg = normalize3(avg);
        const float ax = fabsf(avg.x), ay = fabsf(avg.y), az = fabsf(avg.z);
        const float mc = fmax2(fmax2(ax, ay), az);
        if (mc > 0.85f) {
            if (ax == mc) w.axis = V3{ avg.x > 0.0f ? 1.0f : -1.0f, 0.0f, 0.0f };
            else if (ay == mc) w.axis = V3{ 0.0f, avg.y > 0.0f ? 1.0f : -1.0f, 0.0f };
            else w.axis = V3{ 0.0f, 0.0f, avg.z > 0.0f ? 1.0f : -1.0f };
            walk<kWalkPlane>(solid, g, x, y, z, &w);
            if (w.planeN > 0) {
                const float pn = (float)w.planeN;
                const V3 pp{ w.plane.x / pn, w.plane.y / pn, w.plane.z / pn };
                const float d = -dot3(w.axis, pp);
                const float t = -(dot3(w.axis, centre) + d);
                out->x = clamp1(centre.x + t * w.axis.x, lo.x, hi.x);
                out->y = clamp1(centre.y + t * w.axis.y, lo.y, hi.y);
                out->z = clamp1(centre.z + t * w.axis.z, lo.z, hi.z);
                if (branch) *branch = kBranchPlane;
                return w.n;
            }
        }
    }
    V3 sol = mass;                                           // QEFSolver::solve's masspoint: the same sums, the same division
    int way = kBranchFewPoints;
    if (w.n > 2) {
        way = kBranchMassPoint;
        walk<kWalkQef>(solid, g, x, y, z, &w);
        const float m00 = w.a00 + 0.3f, m11 = w.a11 + 0.3f, m22 = w.a22 + 0.3f;
        const float m01 = w.a01, m02 = w.a02, m12 = w.a12, m10 = w.a01, m20 = w.a02, m21 = w.a12;
        // glm::determinant, then glm::inverse, which forms the determinant again
        const float det = m00 * (m11 * m22 - m21 * m12) - m10 * (m01 * m22 - m21 * m02) + m20 * (m01 * m12 - m11 * m02);
        if (!((double)fabsf(det) < 1e-10)) {
            const float ood = 1.0f / det;
            const float i00 = (m11 * m22 - m21 * m12) * ood, i10 = -(m10 * m22 - m20 * m12) * ood, i20 = (m10 * m21 - m20 * m11) * ood;
            const float i01 = -(m01 * m22 - m21 * m02) * ood, i11 = (m00 * m22 - m20 * m02) * ood, i21 = -(m00 * m21 - m20 * m01) * ood;
            const float i02 = (m01 * m12 - m11 * m02) * ood, i12 = -(m00 * m12 - m10 * m02) * ood, i22 = (m00 * m11 - m10 * m01) * ood;
            const bool ok = entry_ok(i00) && entry_ok(i01) && entry_ok(i02) && entry_ok(i10) && entry_ok(i11) && entry_ok(i12) &&
                            entry_ok(i20) && entry_ok(i21) && entry_ok(i22);
            if (ok) {
                V3 s{ i00 * w.atb.x + i10 * w.atb.y + i20 * w.atb.z, i01 * w.atb.x + i11 * w.atb.y + i21 * w.atb.z,
                      i02 * w.atb.x + i12 * w.atb.y + i22 * w.atb.z };
                s = V3{ mass.x + 0.7f * (s.x - mass.x), mass.y + 0.7f * (s.y - mass.y), mass.z + 0.7f * (s.z - mass.z) };
                if (!__builtin_isnan(s.x) && !__builtin_isnan(s.y) && !__builtin_isnan(s.z)) {
                    const V3 df{ mass.x - s.x, mass.y - s.y, mass.z - s.z };
                    const float cell = hi.x - lo.x;
                    if (dot3(df, df) < cell * cell) {
                        const float k1 = 1.0f - 0.2f;
                        sol = V3{ s.x * k1 + mass.x * 0.2f, s.y * k1 + mass.y * 0.2f, s.z * k1 + mass.z * 0.2f };
                        way = kBranchQef;
                    }
                }
            }
        }
    }
    const float k9 = 1.0f - 0.1f;
    out->x = clamp1(sol.x, lo.x, hi.x) * k9 + mass.x * 0.1f;
    out->y = clamp1(sol.y, lo.y, hi.y) * k9 + mass.y * 0.1f;
    out->z = clamp1(sol.z, lo.z, hi.z) * k9 + mass.z * 0.1f;
    if (branch) *branch = way;
    return w.n;
}

// The finish of one triangle (a, b, c): the squared length of cross(b - a, c - a) and its normal, negated when `invert`; where
// that length is 0 or not finite the normal is (+0, +0, +0) and the function answers false (a degenerate triangle).
RTO_DC_HD bool triangle_normal(V3 a, V3 b, V3 c, bool invert, V3* n, float* l2out) {
    const float ax = b.x - a.x, ay = b.y - a.y, az = b.z - a.z;
    const float bx = c.x - a.x, by = c.y - a.y, bz = c.z - a.z;
    const V3 cr{ ay * bz - by * az, az * bx - bz * ax, ax * by - bx * ay };                    // glm::cross
    const float l2 = dot3(cr, cr);
    *l2out = l2;
    if (l2 > 0.0f && !__builtin_isinf(l2) && !__builtin_isnan(l2)) {
        V3 u = scale3(cr, 1.0f / sqrtf(l2));
        if (invert) u = V3{ -u.x, -u.y, -u.z };
        *n = u;
        return true;
    }
    *n = V3{ 0.0f, 0.0f, 0.0f };
    return false;
}
// buildTrianglesCPU's test: 0.5f * length(cross) > 1e-6, the literal a double.
RTO_DC_HD bool area_kept(float l2) { return (double)(0.5f * sqrtf(l2)) > 1e-6; }

// The four voxels of the face of cell (x, y, z) towards +axis, in the reference's order V00, V01, V11, V10, as offsets from the cell:
// bit 0, 1, 2 of entry q: +1 in x, y, z.  Triangles: (V00, V01, V11) then (V00, V11, V10).
RTO_DC_HD int face_corner(int axis, int q) {
    // axis 0: 0, +y, +x+y, +x; axis 1: 0, +x, +x+y, +y; axis 2: 0, +y, +y+z, +z
    const unsigned packed = axis == 0 ? 0x1320u : axis == 1 ? 0x2310u : 0x4620u;
    return (int)((packed >> (4 * q)) & 7u);
}

}  // namespace rto_dc
