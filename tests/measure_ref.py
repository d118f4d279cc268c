"""The component-measure rule of include/rto_hip.h in numpy alone, stated twice.

A label volume (dimZ, dimY, dimX) int32 holds the component's number, -1 outside the set; "in the set" means label >= 0 and voxels
beyond the grid are not in the set.  Voxel (i, j, k) has linear index v = i + dimX (j + dimY k).  Per component, 20 int64: voxels,
faces[6] (-x, +x, -y, +y, -z, +z: voxels whose neighbour there is not in the set), cells[3], euler, sum[3] (i, j, k), sum2[6]
(ii, jj, kk, ij, ik, jk).  CONN_FULL: cells = the distinct lattice vertices, edges and faces incident to a voxel of the component,
euler = n0 - n1 + n2 - voxels.  CONN_FACE: cells = the fully set face-adjacent pairs, 2 x 2 squares and 2 x 2 x 2 blocks, euler =
voxels - P + Q - O.

measure():          the windowed counting form.  Every count is a per-voxel predicate on the 3 x 3 x 3 window (OR / AND of shifted
                    copies of the membership mask) summed per label.  A FULL cell is counted at the incident set voxel with the
                    smallest linear index, a FACE cell at its lowest corner.
measure_by_piece(): per component, the whole-set rule applied to that component alone in an empty grid: cells are counted on
                    their own lattices (a vertex array, three edge arrays, three face arrays), with no attribution to voxels.
The two agree exactly when no cell is shared between components, which is what the rule claims.
"""
from __future__ import annotations

import numpy as np

import component_ref as cr

CONN_FACE, CONN_FULL = cr.CONN_FACE, cr.CONN_FULL
MEASURE_DTYPE = np.dtype([("voxels", "<i8"), ("faces", "<i8", (6,)), ("cells", "<i8", (3,)), ("euler", "<i8"), ("sum", "<i8", (3,)),
                          ("sum2", "<i8", (6,))])
DIRS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def _euler(t, connectivity):
    c, v = t["cells"], t["voxels"]
    return c[..., 0] - c[..., 1] + c[..., 2] - v if connectivity == CONN_FULL else v - c[..., 0] + c[..., 1] - c[..., 2]


def total_of(table):
    """The total row: the sum of the records, field by field."""
    t = np.zeros((), MEASURE_DTYPE)
    for f in MEASURE_DTYPE.names:
        t[f] = table[f].sum(axis=0)
    return t


def measure(labels, count, connectivity):
    """(table MEASURE_DTYPE[count], total) by windowed counting."""
    assert connectivity in (CONN_FACE, CONN_FULL)
    lab = np.asarray(labels, np.int32)
    Z, Y, X = lab.shape
    m = lab >= 0
    P = np.zeros((Z + 2, Y + 2, X + 2), bool)
    P[1:-1, 1:-1, 1:-1] = m
    flat = lab[m].astype(np.int64)

    def nb(dx, dy, dz):
        return P[1 + dz:1 + dz + Z, 1 + dy:1 + dy + Y, 1 + dx:1 + dx + X]

    def per_label(mask):
        return np.bincount(lab[mask].astype(np.int64), minlength=count).astype(np.int64)

    t = np.zeros(count, MEASURE_DTYPE)
    t["voxels"] = np.bincount(flat, minlength=count)
    for d, (dx, dy, dz) in enumerate(DIRS):
        t["faces"][:, d] = per_label(m & ~nb(dx, dy, dz))
    if connectivity == CONN_FULL:
        # a cell of the voxel's cube is given per axis by 0 (the voxel's own extent: offsets {0}), 1 (its near end: {-1, 0}) or
        # 2 (its far end: {0, 1}); three ends make a vertex, two an edge, one a face
        for mz in range(3):
            for my in range(3):
                for mx in range(3):
                    ends = (mx != 0) + (my != 0) + (mz != 0)
                    if ends == 0:
                        continue
                    rng = lambda mode: range(-1 if mode == 1 else 0, (1 if mode == 2 else 0) + 1)
                    blocked = np.zeros_like(m)
                    for dz in rng(mz):
                        for dy in rng(my):
                            for dx in rng(mx):
                                if (dz, dy, dx) < (0, 0, 0):          # a smaller linear index
                                    blocked |= nb(dx, dy, dz)
                    t["cells"][:, 3 - ends] += per_label(m & ~blocked)
    else:
        for e in range(1, 8):
            ex, ey, ez = e & 1, (e >> 1) & 1, e >> 2
            full = m.copy()
            for dz in range(ez + 1):
                for dy in range(ey + 1):
                    for dx in range(ex + 1):
                        full &= nb(dx, dy, dz)
            t["cells"][:, ex + ey + ez - 1] += per_label(full)
    k, j, i = (a.astype(np.int64) for a in np.nonzero(m))
    coords = (i, j, k)
    for a in range(3):
        t["sum"][:, a] = _isum(flat, coords[a], count)
    for q, (a, b) in enumerate(PAIRS):
        t["sum2"][:, q] = _isum(flat, coords[a] * coords[b], count)
    t["euler"] = _euler(t, connectivity)
    return t, total_of(t)


def _isum(flat, values, count):
    """Exact int64 sums of `values` per label (bincount's weights are float64: not exact above 2^53)."""
    out = np.zeros(count, np.int64)
    np.add.at(out, flat, values)
    return out


def measure_set(mask, connectivity):
    """One record for the whole set `mask` (bool (Z, Y, X)), cells counted on their own lattices."""
    m = np.asarray(mask, bool)
    Z, Y, X = m.shape
    P = np.zeros((Z + 2, Y + 2, X + 2), bool)
    P[1:-1, 1:-1, 1:-1] = m
    r = np.zeros((), MEASURE_DTYPE)
    r["voxels"] = int(m.sum())
    for d, (dx, dy, dz) in enumerate(DIRS):
        r["faces"][d] = int((m & ~P[1 + dz:1 + dz + Z, 1 + dy:1 + dy + Y, 1 + dx:1 + dx + X]).sum())
    if connectivity == CONN_FULL:
        # P is padded by one, so padded index p is voxel p - 1: a lattice point a touches padded a and a + 1; a spanned voxel v is padded v + 1
        def count_cells(span):
            acc = None
            for oz in ((1,) if span[2] else (0, 1)):
                for oy in ((1,) if span[1] else (0, 1)):
                    for ox in ((1,) if span[0] else (0, 1)):
                        part = P[oz:oz + Z + (0 if span[2] else 1), oy:oy + Y + (0 if span[1] else 1), ox:ox + X + (0 if span[0] else 1)]
                        acc = part.copy() if acc is None else acc | part
            return int(acc.sum())
        r["cells"][0] = count_cells((0, 0, 0))
        r["cells"][1] = count_cells((1, 0, 0)) + count_cells((0, 1, 0)) + count_cells((0, 0, 1))
        r["cells"][2] = count_cells((1, 1, 0)) + count_cells((1, 0, 1)) + count_cells((0, 1, 1))
    else:
        def blocks(ex, ey, ez):
            acc = np.ones((max(Z - ez, 0), max(Y - ey, 0), max(X - ex, 0)), bool)
            for dz in range(ez + 1):
                for dy in range(ey + 1):
                    for dx in range(ex + 1):
                        acc = acc & m[dz:Z - ez + dz, dy:Y - ey + dy, dx:X - ex + dx]
            return int(acc.sum())
        r["cells"][0] = blocks(1, 0, 0) + blocks(0, 1, 0) + blocks(0, 0, 1)
        r["cells"][1] = blocks(1, 1, 0) + blocks(1, 0, 1) + blocks(0, 1, 1)
        r["cells"][2] = blocks(1, 1, 1)
    k, j, i = (a.astype(np.int64) for a in np.nonzero(m))
    c = (i, j, k)
    for a in range(3):
        r["sum"][a] = int(c[a].sum())
    for q, (a, b) in enumerate(PAIRS):
        r["sum2"][q] = int((c[a] * c[b]).sum())
    r["euler"] = _euler(r, connectivity)
    return r


def measure_by_piece(labels, count, connectivity):
    """(table, total): every component measured alone in an empty grid by measure_set (inside its bounding box, which is the same
    thing: beyond the box the grid is empty either way), its index sums moved back by the box's corner."""
    lab = np.asarray(labels, np.int32)
    t = np.zeros(count, MEASURE_DTYPE)
    if count:
        k, j, i = np.nonzero(lab >= 0)
        l = lab[k, j, i]
        lo = np.full((count, 3), np.iinfo(np.int64).max, np.int64)
        hi = np.full((count, 3), -1, np.int64)
        for a, c in enumerate((i, j, k)):
            np.minimum.at(lo[:, a], l, c)
            np.maximum.at(hi[:, a], l, c)
    for c in range(count):
        (x0, y0, z0), (x1, y1, z1) = lo[c], hi[c]
        r = measure_set(lab[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] == c, connectivity)
        n, s = int(r["voxels"]), r["sum"].copy()
        o = (int(x0), int(y0), int(z0))
        for q, (a, b) in enumerate(PAIRS):                          # (o_a + u)(o_b + w) summed over the voxels
            r["sum2"][q] += o[a] * int(s[b]) + o[b] * int(s[a]) + n * o[a] * o[b]
        for a in range(3):
            r["sum"][a] += n * o[a]
        t[c] = r
    return t, total_of(t)


def measure_grid(grid, set, connectivity):
    """(labels, component table, measure table, total) of a uint8 grid under the rule of sections 18 and 22."""
    labels, comps = cr.label(grid, set, connectivity)
    table, total = measure(labels, len(comps), connectivity)
    return labels, comps, table, total


def topology(grid, set=cr.SET_SOLID, connectivity=CONN_FACE):
    """(pieces, tunnels, cavities): cavities are the complement's components under the dual connectivity that touch no grid face,
    tunnels = pieces + cavities - the whole set's Euler number."""
    dual = CONN_FULL if connectivity == CONN_FACE else CONN_FACE
    _, outside = cr.label(grid, 1 - set, dual)
    cavities = int((outside["touches"] == 0).sum())
    _, comps, _, total = measure_grid(grid, set, connectivity)
    return len(comps), len(comps) + cavities - int(total["euler"]), cavities


def physical_direct(labels, c, grid_min, voxel_size):
    """(centroid, covariance) of component c's voxel centres in world units, taken directly in float64."""
    k, j, i = np.nonzero(np.asarray(labels) == c)
    p = np.asarray(grid_min, np.float64) + (np.stack([i, j, k], 1).astype(np.float64) + 0.5) * float(voxel_size)
    mean = p.mean(axis=0)
    d = p - mean
    return mean, d.T @ d / len(p)
