"""The local-thickness rule (rto_thickness_field) restated in numpy: the reference the GPU fields, histograms
and summaries are checked against.

Voxel (i, j, k) has linear index v = i + dimX (j + dimY k); grids are uint8 (dimZ, dimY, dimX).  SET_SOLID is the voxels equal to 1,
SET_EMPTY the voxels equal to 0; voxels outside the grid do not exist.
    mq    = floor(max_radius / voxelSize * 64 + 0.5) as distance_ref.quantize; c = floor(mq^2 / 4096); c = 0 is invalid, c > 64 (+inf
            included) unsupported.
    D[q]  = min(d2 from q to the nearest voxel of the other set, c) for q in the medium (NONE clips to c); 0 outside the medium.
    t2[p] = max{ D[q] : q in the grid, (p - q)^2 < D[q] } for p in the medium; 0 elsewhere.
    bins[t], t = 0 .. c: medium voxels with t2 = t.  Summary: the smallest value over the medium, the smallest index that holds it,
            the voxels below c, the medium voxels; -1, -1, 0, 0 with no medium voxel.
The rule is stated twice: gather (every voxel looks at every offset o with o^2 < c and keeps the largest D[p + o] > o^2) and scatter
(every ball is painted over the voxels it covers, one ball at a time).  D comes from distance_ref: its brute force by default; the
separable form (which tests/test_distance.py pins to the brute force) for grids too large for that.
"""
from __future__ import annotations

import numpy as np

import distance_ref as dr

SET_EMPTY, SET_SOLID = dr.SET_EMPTY, dr.SET_SOLID
MAX_C = 64
SUMMARY_DTYPE = np.dtype([("min_t2", "<i8"), ("argmin", "<i8"), ("thin", "<i8"), ("medium", "<i8")])


class Unsupported(ValueError):
    """Where the call answers RTO_E_UNSUPPORTED (ValueError: RTO_E_INVALID)."""


def cap(max_radius, voxel_size):
    """c of a radius; ValueError where the call answers RTO_E_INVALID, Unsupported where it answers RTO_E_UNSUPPORTED."""
    mq = dr.quantize(max_radius, voxel_size)
    if mq is None:
        raise Unsupported("no cap: more than 8 voxels")
    return cap_of_quanta(mq)


def cap_of_quanta(mq):
    c = mq * mq // 4096
    if c == 0:
        raise ValueError("a radius under one voxel")
    if c > MAX_C:
        raise Unsupported("more than 8 voxels")
    return int(c)


def isqrt_below(c):
    """The largest h with h^2 < c: how far along an axis an offset with o^2 < c reaches."""
    h = 0
    while (h + 1) * (h + 1) < c:
        h += 1
    return h


def clipped_radius(grid, medium, c, fld=dr.brute_force):
    """D as int64: min(d2 to the complement of the medium, c) on the medium, 0 elsewhere."""
    g = np.asarray(grid, np.uint8)
    d2 = fld(g, 1 - medium).astype(np.int64)
    D = np.minimum(d2, c)
    assert ((D == 0) == (g != medium)).all()
    return D


def offsets(c):
    """Every (dz, dy, dx, o^2) with o^2 < c, in ascending o^2."""
    h = isqrt_below(c)
    out = [(dz * dz + dy * dy + dx * dx, dz, dy, dx) for dz in range(-h, h + 1) for dy in range(-h, h + 1) for dx in range(-h, h + 1)
           if dz * dz + dy * dy + dx * dx < c]
    return [(dz, dy, dx, s) for s, dz, dy, dx in sorted(out)]


def gather(D, c, dtype=np.int64):
    """t2 as int32 from D: every voxel takes the largest D[p + o] > o^2 over the offsets with o^2 < min(c, max D).  Voxels outside
    the grid hold 0 (a padded copy).  dtype: the working type; values never exceed 64, so uint8 gives the same field faster."""
    lim = min(c, int(D.max(initial=0)))
    h = isqrt_below(lim) if lim > 0 else 0
    P = np.pad(D.astype(dtype), h)
    Z, Y, X = D.shape
    best = np.zeros(D.shape, dtype)
    for dz, dy, dx, s in offsets(lim) if lim > 0 else []:
        q = P[h + dz:h + dz + Z, h + dy:h + dy + Y, h + dx:h + dx + X]
        np.maximum(best, np.where(q > s, q, 0).astype(dtype), out=best)
    return np.where(D > 0, best, 0).astype(np.int32)


def scatter(D, c):
    """The same field, one ball at a time: every voxel q with D[q] > 0 paints D[q] over the voxels p of the grid with
    (p - q)^2 < D[q].  A ball never reaches a voxel of the grid outside the medium (asserted)."""
    Z, Y, X = D.shape
    t2 = np.zeros(D.shape, np.int64)
    for k, j, i in zip(*np.nonzero(D)):
        r2 = int(D[k, j, i])
        h = isqrt_below(r2)
        z0, z1, y0, y1, x0, x1 = max(0, k - h), min(Z, k + h + 1), max(0, j - h), min(Y, j + h + 1), max(0, i - h), min(X, i + h + 1)
        zz, yy, xx = np.ogrid[z0:z1, y0:y1, x0:x1]
        inside = (zz - k) ** 2 + (yy - j) ** 2 + (xx - i) ** 2 < r2
        box = t2[z0:z1, y0:y1, x0:x1]
        box[inside] = np.maximum(box[inside], r2)
    assert (t2[D == 0] == 0).all()
    return t2.astype(np.int32)


def field(grid, medium, c, fld=dr.brute_force, dtype=np.int64):
    return gather(clipped_radius(grid, medium, c, fld), c, dtype)


def histogram(t2, c):
    """int64 bins[0 .. c]; bins[0] is 0 by the rule (the voxels outside the medium are not counted)."""
    bins = np.bincount(t2.reshape(-1), minlength=c + 1).astype(np.int64)
    assert bins.size == c + 1
    bins[0] = 0
    return bins


def summary(t2, c):
    out = np.zeros((), SUMMARY_DTYPE)
    flat = t2.reshape(-1)
    med = flat > 0
    out["medium"] = int(med.sum())
    out["thin"] = int((med & (flat < c)).sum())
    if med.any():
        m = int(flat[med].min())
        out["min_t2"] = m
        out["argmin"] = int(np.flatnonzero(flat == m)[0])
    else:
        out["min_t2"] = -1
        out["argmin"] = -1
    return out
