"""The dual-contouring rule in numpy float32, every voxel at once: one array operation per operator of the
rule, in the order written (numpy neither contracts nor reorders).  The up to 24 Hermite points of a voxel -- 2 x 2 x 2 gathered
voxels, z slowest, times the +X, +Y, +Z neighbour -- are 24 masked slots walked in that order.  Independent of the C++ and HIP
forms; tests/golden/make_golden_dc.py holds it against the reference's own compiled functions, byte for byte.

    vertices(vox, gmin, vs)            -> verts (dz, dy, dx, 3) float32, points (dz, dy, dx) int32, branch (dz, dy, dx) int8
    extract(vox, gmin, vs, area_rule, clip) -> tris (n, 12) float32, tri_cell (n,) int32, summary dict
"""
from __future__ import annotations

import numpy as np

F = np.float32
AREA_REFERENCE, AREA_NONE = 0, 1
# the ways through the vertex rule
B_NO_POINT, B_FEW_POINTS, B_PLANE, B_QEF, B_MASS_POINT = 0, 1, 2, 3, 4
BRANCH_NAMES = ("no point", "at most 2 points", "snap with a plane", "QEF accepted", "mass-point fallback")


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _normalize(v):
    inv = F(1.0) / np.sqrt(_dot(v, v))
    return [v[0] * inv, v[1] * inv, v[2] * inv]


def _clamp(v, lo, hi):
    m = np.where(v < lo, lo, v)              # glm::max(x, lo)
    return np.where(hi < m, hi, m)           # glm::min(.., hi)


def vertices(vox, gmin, vs, with_dominant=False):
    vox = np.asarray(vox, np.uint8)
    dz, dy, dx = vox.shape
    gmin = np.asarray(gmin, F)
    vs = F(vs)
    P = np.zeros((dz + 6, dy + 6, dx + 6), bool)          # solid, false outside the grid
    P[3:-3, 3:-3, 3:-3] = vox == 1
    Z, Y, X = np.indices((dz, dy, dx))
    dims = (dx, dy, dz)

    def solid(x, y, z):
        return P[z + 3, y + 3, x + 3]

    def world(c, a):
        return gmin[a] + c.astype(F) * vs

    slots = []
    with np.errstate(all="ignore"):
        for oz in (0, 1):
            for oy in (0, 1):
                for ox in (0, 1):
                    u = (X + ox, Y + oy, Z + oz)
                    inside = (u[0] <= dx - 1) & (u[1] <= dy - 1) & (u[2] <= dz - 1)
                    cur = solid(*u)
                    for d in range(3):
                        e = [1 if a == d else 0 for a in range(3)]
                        w = tuple(u[a] + e[a] for a in range(3))
                        valid = inside & (w[d] < dims[d])
                        nxt = solid(*w)
                        mask = valid & (cur != nxt)
                        pos = []
                        for a in range(3):
                            p1, p2 = world(u[a], a), world(w[a], a)
                            pos.append(p1 + F(0.5) * (p2 - p1))
                        g = []
                        for a in range(3):
                            if a == d:
                                g.append(np.zeros(X.shape, F))
                                continue
                            up = tuple(u[b] + (1 if b == a else 0) for b in range(3))
                            dn = tuple(u[b] - (1 if b == a else 0) for b in range(3))
                            g.append(np.where(solid(*up), F(-1), F(1)).astype(F) - np.where(solid(*dn), F(-1), F(1)).astype(F))
                        l2 = _dot(g, g)
                        small = l2.astype(np.float64) < 1e-10
                        gn = _normalize(g)
                        ef = [F(v) for v in e]
                        n = [np.where(small, ef[a], gn[a]).astype(F) for a in range(3)]
                        along = (n[0] * ef[0] + n[1] * ef[1]) + n[2] * ef[2]
                        flip = (along > 0) == nxt
                        n = [np.where(flip, -n[a], n[a]) for a in range(3)]
                        slots.append((mask, pos, n))

        zero = np.zeros(X.shape, F)
        count = np.zeros(X.shape, np.int32)
        mass = [zero.copy() for _ in range(3)]
        avg = [zero.copy() for _ in range(3)]
        for mask, pos, n in slots:
            for a in range(3):
                mass[a] = np.where(mask, mass[a] + pos[a], mass[a])
                avg[a] = np.where(mask, avg[a] + n[a], avg[a])
            count += mask
        centre = [(world(c, a)) + F(0.5) * vs for a, c in enumerate((X, Y, Z))]
        half, inset = vs * F(0.5), vs * F(0.001)
        lo = [(centre[a] - half) + inset for a in range(3)]
        hi = [(centre[a] + half) - inset for a in range(3)]
        fn = count.astype(F)
        mp = [mass[a] / fn for a in range(3)]

        long_enough = np.sqrt(_dot(avg, avg)) > F(0.0001)
        an = _normalize(avg)
        ab = [np.abs(an[a]) for a in range(3)]
        mc = np.maximum(np.maximum(ab[0], ab[1]), ab[2])
        dominant = long_enough & (mc > F(0.85)) & (count > 0)
        isx = ab[0] == mc
        isy = ~isx & (ab[1] == mc)
        isz = ~isx & ~isy
        axis = [np.where(isx, np.where(an[0] > 0, F(1), F(-1)), F(0)).astype(F),
                np.where(isy, np.where(an[1] > 0, F(1), F(-1)), F(0)).astype(F),
                np.where(isz, np.where(an[2] > 0, F(1), F(-1)), F(0)).astype(F)]
        plane = [zero.copy() for _ in range(3)]
        plane_n = np.zeros(X.shape, np.int32)
        for mask, pos, n in slots:
            aligned = mask & (_dot(_normalize(n), axis) > F(0.7))
            for a in range(3):
                plane[a] = np.where(aligned, plane[a] + pos[a], plane[a])
            plane_n += aligned
        use_plane = dominant & (plane_n > 0)
        pn = plane_n.astype(F)
        pp = [plane[a] / pn for a in range(3)]
        dpl = -_dot(axis, pp)
        t = -(_dot(axis, centre) + dpl)
        plane_v = [_clamp(centre[a] + t * axis[a], lo[a], hi[a]) for a in range(3)]

        # QEFSolver
        A = {k: zero.copy() for k in ("00", "01", "02", "11", "12", "22")}
        atb = [zero.copy() for _ in range(3)]
        for mask, pos, n in slots:
            u = _normalize(n)
            for k, (i, j) in (("00", (0, 0)), ("01", (0, 1)), ("02", (0, 2)), ("11", (1, 1)), ("12", (1, 2)), ("22", (2, 2))):
                A[k] = np.where(mask, A[k] + u[i] * u[j], A[k])
            dd = -_dot(u, pos)
            for a in range(3):
                atb[a] = np.where(mask, atb[a] + u[a] * dd, atb[a])
        m00, m11, m22 = A["00"] + F(0.3), A["11"] + F(0.3), A["22"] + F(0.3)
        m01 = m10 = A["01"]
        m02 = m20 = A["02"]
        m12 = m21 = A["12"]
        det = m00 * (m11 * m22 - m21 * m12) - m10 * (m01 * m22 - m21 * m02) + m20 * (m01 * m12 - m11 * m02)
        assert not (np.abs(det).astype(np.float64) < 1e-10).any()      # the branch no input takes
        ood = F(1.0) / det
        i00 = (m11 * m22 - m21 * m12) * ood
        i10 = -(m10 * m22 - m20 * m12) * ood
        i20 = (m10 * m21 - m20 * m11) * ood
        i01 = -(m01 * m22 - m21 * m02) * ood
        i11 = (m00 * m22 - m20 * m02) * ood
        i21 = -(m00 * m21 - m20 * m01) * ood
        i02 = (m01 * m12 - m11 * m02) * ood
        i12 = -(m00 * m12 - m10 * m02) * ood
        i22 = (m00 * m11 - m10 * m01) * ood
        for inv in (i00, i10, i20, i01, i11, i21, i02, i12, i22):
            assert np.isfinite(inv).all() and not (np.abs(inv).astype(np.float64) > 1e6).any()      # nor this one
        s = [(i00 * atb[0] + i10 * atb[1]) + i20 * atb[2], (i01 * atb[0] + i11 * atb[1]) + i21 * atb[2],
             (i02 * atb[0] + i12 * atb[1]) + i22 * atb[2]]
        s = [mp[a] + F(0.7) * (s[a] - mp[a]) for a in range(3)]
        df = [mp[a] - s[a] for a in range(3)]
        cell = hi[0] - lo[0]
        near = ~(np.isnan(s[0]) | np.isnan(s[1]) | np.isnan(s[2])) & (_dot(df, df) < cell * cell)
        accepted = (count > 2) & near
        k1 = F(1.0) - F(0.2)
        mixed = [s[a] * k1 + mp[a] * F(0.2) for a in range(3)]
        sol = [np.where(accepted, mixed[a], mp[a]) for a in range(3)]
        k9 = F(1.0) - F(0.1)
        qef_v = [_clamp(sol[a], lo[a], hi[a]) * k9 + mp[a] * F(0.1) for a in range(3)]

        none = count == 0
        verts = np.stack([np.where(none, centre[a], np.where(use_plane, plane_v[a], qef_v[a])).astype(F) for a in range(3)], axis=-1)
    branch = np.where(none, B_NO_POINT, np.where(use_plane, B_PLANE, np.where(count <= 2, B_FEW_POINTS,
                      np.where(accepted, B_QEF, B_MASS_POINT)))).astype(np.int8)
    if with_dominant:
        return verts, count, branch, (dominant & ~use_plane)
    return verts, count, branch


def extract(vox, gmin, vs, area_rule=AREA_REFERENCE, clip=None, verts=None, points=None):
    vox = np.asarray(vox, np.uint8)
    dz, dy, dx = vox.shape
    if verts is None:
        verts, points, _ = vertices(vox, gmin, vs)
    solid = vox == 1
    lo = (0, 0, 0) if clip is None else tuple(int(v) for v in clip[0])
    hi = (dx, dy, dz) if clip is None else tuple(int(v) for v in clip[1])
    hi = (min(hi[0], dx - 1), min(hi[1], dy - 1), min(hi[2], dz - 1))
    summary = dict(faces=0, triangles=0, dropped=0, degenerate=0, vertex_voxels=0)
    if any(hi[a] <= lo[a] for a in range(3)):
        return np.zeros((0, 12), F), np.zeros(0, np.int32), summary
    sl = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    c = solid[sl]
    face = np.stack([c != solid[lo[2]:hi[2], lo[1]:hi[1], lo[0] + 1:hi[0] + 1],
                     c != solid[lo[2]:hi[2], lo[1] + 1:hi[1] + 1, lo[0]:hi[0]],
                     c != solid[lo[2] + 1:hi[2] + 1, lo[1]:hi[1], lo[0]:hi[0]]], axis=-1)
    idx = np.argwhere(face)                                # z, y, x, axis: the reference's order
    z, y, x, axis = idx[:, 0] + lo[2], idx[:, 1] + lo[1], idx[:, 2] + lo[0], idx[:, 3]
    # V00, V01, V11, V10 as (dx, dy, dz) per axis
    corners = np.array([[(0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0)],
                        [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)],
                        [(0, 0, 0), (0, 1, 0), (0, 1, 1), (0, 0, 1)]])
    off = corners[axis]                                    # (faces, 4, 3)
    vx, vy, vz = x[:, None] + off[:, :, 0], y[:, None] + off[:, :, 1], z[:, None] + off[:, :, 2]
    q = verts[vz, vy, vx]                                  # (faces, 4, 3)
    inv = solid[z, y, x]
    read = np.zeros(solid.shape, bool)
    read[vz, vy, vx] = True
    recs, cells, keep = [], [], []
    with np.errstate(all="ignore"):
        for t in (0, 1):
            a, b, d = q[:, 0], q[:, 1 + t], q[:, 2 + t]
            e1, e2 = b - a, d - a
            cr = [e1[:, 1] * e2[:, 2] - e2[:, 1] * e1[:, 2], e1[:, 2] * e2[:, 0] - e2[:, 2] * e1[:, 0], e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1]]
            l2 = _dot(cr, cr)
            fine = (l2 > 0) & np.isfinite(l2)
            invs = F(1.0) / np.sqrt(l2)
            n = np.stack([np.where(fine, np.where(inv, -(cr[k] * invs), cr[k] * invs), F(0)) for k in range(3)], axis=-1).astype(F)
            area = (F(0.5) * np.sqrt(l2)).astype(np.float64)
            keep.append((area > 1e-6) if area_rule == AREA_REFERENCE else np.ones(len(l2), bool))
            recs.append(np.concatenate([a, b, d, n], axis=1).astype(F))
            cells.append(((z * dy + y) * dx + x).astype(np.int32))
    rec = np.stack(recs, axis=1).reshape(-1, 12)           # face-major, then the two triangles
    cell = np.stack(cells, axis=1).reshape(-1)
    kp = np.stack(keep, axis=1).reshape(-1)
    tris, tri_cell = rec[kp], cell[kp]
    summary["faces"] = int(len(idx))
    summary["triangles"] = int(len(tris))
    summary["dropped"] = int(2 * len(idx) - len(tris))
    summary["degenerate"] = int((~tris[:, 9:12].astype(bool).any(axis=1)).sum()) if len(tris) else 0
    summary["vertex_voxels"] = int((read & (points > 0)).sum())
    return np.ascontiguousarray(tris), np.ascontiguousarray(tri_cell), summary
