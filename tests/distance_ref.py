"""The distance-field rule (rto_distance_field, rto_edit_morphology) restated in numpy int64: the reference the
GPU fields and edits are checked against.

Voxel (i, j, k) has linear index v = i + dimX (j + dimY k); grids are uint8 (dimZ, dimY, dimX).  SET_SOLID is the voxels equal to 1,
SET_EMPTY the voxels equal to 0; voxels outside the grid belong to no set.
    d2[v] = min over the voxels u of the set of (i_v - i_u)^2 + (j_v - j_u)^2 + (k_v - k_u)^2, NONE where the set is empty.
    mq    = floor(max_dist / voxelSize * 64 + 0.5) in float64 from the float32 inputs, one IEEE operation at a time; +inf: no cap;
            NaN, a negative value or mq > 2^28: invalid.  In reach: 4096 d2 <= mq^2.  Out of reach: NONE.
    DILATE: EMPTY voxels whose d2 to SOLID is in reach become FILLED.  ERODE: FILLED voxels whose d2 to EMPTY is in reach become
            EMPTY.  OPEN = ERODE then DILATE, CLOSE = DILATE then ERODE; changed counts against the grid before the call.
The rule is stated twice: brute_force (a min over all voxels of the set) and separable (three axis minima over all pairs of a line, O(n^2) per line
at worst, for grids too large for the first).
"""
from __future__ import annotations

import numpy as np

SET_EMPTY, SET_SOLID = 0, 1
DILATE, ERODE, OPEN, CLOSE = 0, 1, 2, 3
NONE = 0x7fffffff
LIMIT = 1 << 28
SUMMARY_DTYPE = np.dtype([("max_d2", "<i8"), ("argmax", "<i8"), ("finite", "<i8"), ("reserved", "<i8")])
_BIG = np.int64(1) << 40              # "no voxel of the set seen yet" inside the separable form


def quantize(dist, voxel_size):
    """mq as an int, None for +inf (no cap); ValueError where the call answers RTO_E_INVALID."""
    d = np.float64(np.float32(dist))
    vs = np.float64(np.float32(voxel_size))
    if np.isinf(d) and d > 0:
        return None
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        f = np.floor(d / vs * 64.0 + 0.5)
    if not (f <= LIMIT and d >= 0):
        raise ValueError(f"invalid distance {dist}")
    return int(f)


def threshold(d2, mq):
    """The capped field: the uncapped one with everything out of reach of mq replaced by NONE."""
    if mq is None:
        return d2
    out = d2.copy()
    out[(d2 == NONE) | (4096 * d2.astype(np.int64) > mq * mq)] = NONE
    return out


def brute_force(grid, s, mq=None):
    """int32 (dimZ, dimY, dimX): the min over every voxel of the set, one set voxel at a time."""
    g = np.asarray(grid, np.uint8)
    k, j, i = np.nonzero(g == s)
    Z, Y, X = np.mgrid[0:g.shape[0], 0:g.shape[1], 0:g.shape[2]].astype(np.int64)
    best = np.full(g.shape, NONE, np.int64)
    for a in range(len(i)):
        best = np.minimum(best, (X - i[a]) ** 2 + (Y - j[a]) ** 2 + (Z - k[a]) ** 2)
    return threshold(best.astype(np.int32), mq)


def _axis_min(f, axis, reach=None):
    """out[.., u, ..] = min over s of f[.., s, ..] + (u - s)^2 along `axis`: every pair (u, u - k) and (u, u + k), k ascending.  The
    loop may stop at the first k whose k^2 is no smaller than every value on the lines that hold a finite value at all: a pair that
    far apart gives f[s] + k^2 >= k^2, which improves nothing.  Until every such entry has been reached the maximum is _BIG.  With
    a cap (reach = floor(mq^2 / 4096)) it may also stop once k^2 > reach: such a pair only makes values the threshold removes."""
    f = np.moveaxis(f, axis, 0)
    n = f.shape[0]
    out = f.copy()
    live = (f < _BIG).any(axis=0)
    for k in range(1, n):
        if not live.any() or k * k >= out[:, live].max() or (reach is not None and k * k > reach):
            break
        np.minimum(out[k:], f[:-k] + k * k, out=out[k:])
        np.minimum(out[:-k], f[k:] + k * k, out=out[:-k])
    return np.moveaxis(out, 0, axis)


def separable(grid, s, mq=None):
    """The same field as three axis minima in int64."""
    g = np.asarray(grid, np.uint8)
    f = np.where(g == s, np.int64(0), _BIG)
    for axis in (2, 1, 0):
        f = _axis_min(f, axis, None if mq is None else mq * mq // 4096)
    out = np.where(f >= _BIG, np.int64(NONE), f)
    assert out.max(initial=0) <= NONE
    return threshold(out.astype(np.int32), mq)


def field(grid, s, mq=None):
    return separable(grid, s, mq)


def summary(d2):
    """The rto_dist_summary of a field as a SUMMARY_DTYPE scalar: max_d2 = argmax = -1 when nothing is finite."""
    out = np.zeros((), SUMMARY_DTYPE)
    flat = d2.reshape(-1)
    fin = flat != NONE
    out["finite"] = int(fin.sum())
    if fin.any():
        m = int(flat[fin].max())
        out["max_d2"] = m
        out["argmax"] = int(np.flatnonzero(flat == m)[0])
    else:
        out["max_d2"] = -1
        out["argmax"] = -1
    return out


def _step(grid, s, rq, fld):
    d2 = fld(grid, s, rq)
    out = grid.copy()
    out[(d2 != NONE) & (grid == (1 - s))] = s
    return out


def morphology(grid, op, rq, fld=field):
    """(edited copy of the grid, changed) for rq quanta (an int; quantize() of the radius)."""
    g = np.array(grid, np.uint8, copy=True)
    if op not in (DILATE, ERODE, OPEN, CLOSE) or rq is None:
        raise ValueError("unknown op, or no radius")
    first = SET_SOLID if op in (DILATE, CLOSE) else SET_EMPTY
    out = _step(g, first, rq, fld)
    if op in (OPEN, CLOSE):
        out = _step(out, 1 - first, rq, fld)
    return out, int((out != g).sum())
