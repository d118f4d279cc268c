"""The dose rule (rto_dose_field) restated in numpy and plain Python: the reference the GPU fields, coverage
tables and summaries and the host layer's CPU form are checked against.

Index, layout, SOLID, EMPTY and the two evaluated sets are tests/exposure_ref.py's.  A source is s = (i, j, k, w), a voxel of the grid
and a weight; for an evaluated voxel p, d = s - p and the segment is centre(p) + t d, 0 < t < 1.
    crossed   a voxel q outside {p, s} is crossed when some t in (0, 1) puts the point strictly inside q's open cube.
    k(p, s)   the number of crossed voxels that are SOLID.
    c(p, s)   floor(((w T[k]) >> 16) / D) for a pair with max-norm |d| <= reach, else 0: T the Q16 table (k >= len(T) transmits 0),
              D = 1, or max(1, |d|^2) under the inverse-square falloff.
    e[v]      the sum of c(p, s) over the sources for an evaluated voxel, -1 for every other voxel.
    covered   per source, the evaluated voxels in reach with k = 0.
The crossing rule is stated twice.  (a) crossed_by_definition() is exposure_ref.crossed(p, d) & exposure_ref.crossed(s, -d): the
open-cube definition in exact integers from both ends.  (b) crossed_by_template() is periods 0 .. g - 1 of exposure_ref.template(d /
g), g the gcd of d's components, without the last entry, which is s.  walls() is (b) for many voxels against one source at once: the
same merge of the plane crossings t = (2 m + 1) / (2 |d_a|), the smallest found by integer cross-multiplication, equal times moving
together.  tests/test_dose.py pins (a) == (b) == walls().
"""
from __future__ import annotations

from math import gcd

import numpy as np

import exposure_ref as er

DOSE_ALL, DOSE_SKIN = 0, 1
FALLOFF_NONE, FALLOFF_INVERSE_SQUARE = 0, 1
MAX_SOURCES = 1024
MAX_REACH = 1023
MAX_TABLE = 64
NO_LIMIT = 0x7FFFFFFF
ONE = 65536
SUMMARY_DTYPE = np.dtype([("evaluated", "<i8"), ("total", "<i8"), ("dark", "<i8"), ("seen", "<i8"), ("peak", "<i8"), ("peak_voxel", "<i8")])


def crossed_by_definition(shape, p, s):
    """(a) The voxels of a (dimZ, dimY, dimX) grid crossed by the open segment from centre(p) to centre(s), as a bool array."""
    d = tuple(int(b) - int(a) for a, b in zip(p, s))
    if d == (0, 0, 0):
        return np.zeros(shape, bool)
    return er.crossed(shape, p, d) & er.crossed(shape, s, tuple(-c for c in d))


def crossed_by_template(p, s):
    """(b) The voxels crossed, in the order they are crossed, as a list of (i, j, k)."""
    d = tuple(int(b) - int(a) for a, b in zip(p, s))
    if d == (0, 0, 0):
        return []
    g = gcd(gcd(abs(d[0]), abs(d[1])), abs(d[2]))
    prim = tuple(c // g for c in d)
    out = []
    for period in range(g):
        for o in er.template(prim):
            out.append(tuple(int(p[a]) + period * prim[a] + int(o[a]) for a in range(3)))
    assert out[-1] == tuple(int(c) for c in s)
    return out[:-1]


def walls_by_definition(g, P, s):
    solid = np.asarray(g) == 1
    return np.asarray([int((crossed_by_definition(solid.shape, tuple(p), s) & solid).sum()) for p in P], np.int64)


def walls_by_template(g, P, s):
    solid = np.asarray(g) == 1
    return np.asarray([sum(int(solid[k, j, i]) for i, j, k in crossed_by_template(tuple(p), s)) for p in P], np.int64)


def walls(g, P, s):
    """(b) for the voxels P, an (N, 3) array of (i, j, k), against the source voxel s: k(p, s) as int64 (N)."""
    solid = np.asarray(g) == 1
    P = np.asarray(P, np.int64).reshape(-1, 3)
    d = np.asarray(s, np.int64)[None, :] - P
    L, sign = np.abs(d), np.where(d < 0, -1, 1)
    m, at, k = np.zeros_like(P), P.copy(), np.zeros(len(P), np.int64)
    idx = np.flatnonzero(L.max(axis=1) > 0)
    while idx.size:
        Ls, ms = L[idx], m[idx]
        valid, num = ms < Ls, 2 * ms + 1
        best_num, best_den = np.ones(idx.size, np.int64), np.zeros(idx.size, np.int64)        # 1 / 0: later than every crossing
        for a in range(3):
            sooner = valid[:, a] & (num[:, a] * best_den < best_num * Ls[:, a])
            best_num, best_den = np.where(sooner, num[:, a], best_num), np.where(sooner, Ls[:, a], best_den)
        move = valid & (num * best_den[:, None] == best_num[:, None] * Ls)
        assert move.any(axis=1).all()
        m[idx] = ms + move
        at[idx] += sign[idx] * move
        on = ~(m[idx] == Ls).all(axis=1)                                  # the others have arrived at s
        idx = idx[on]
        k[idx] += solid[at[idx, 2], at[idx, 1], at[idx, 0]]
    return k


def check_args(g, sources, transmit, falloff, mode, reach):
    if sources is None:
        raise ValueError("sources is NULL")
    src = [tuple(int(c) for c in s) for s in sources]
    if not 1 <= len(src) <= MAX_SOURCES:
        raise ValueError("n out of range")
    if any(len(s) != 4 for s in src) or min(s[3] for s in src) < 0 or sum(s[3] for s in src) > 2 ** 31 - 1:
        raise ValueError("bad weights")
    T = [ONE] if transmit is None else [int(t) for t in transmit]
    if not 1 <= len(T) <= MAX_TABLE or min(T) < 0 or max(T) > ONE:
        raise ValueError("a bad table")
    if falloff not in (FALLOFF_NONE, FALLOFF_INVERSE_SQUARE):
        raise ValueError("unknown falloff")
    if mode not in (DOSE_ALL, DOSE_SKIN):
        raise ValueError("unknown mode")
    if reach < 1:
        raise ValueError("reach below 1")
    dz, dy, dx = np.asarray(g).shape
    for n, s in enumerate(src):
        if not (0 <= s[0] < dx and 0 <= s[1] < dy and 0 <= s[2] < dz):
            raise ValueError(f"source {n} is outside the grid")
    return src, T


def dose(g, sources, transmit=None, falloff=FALLOFF_NONE, mode=DOSE_ALL, reach=NO_LIMIT, walls=walls, counts=None):
    """(e int32 (dimZ, dimY, dimX), covered int64 (n), the summary as a SUMMARY_DTYPE scalar).  `counts`, a dict, receives 'pairs',
    'clear' and 'two': the (evaluated voxel, source) pairs in reach, those with k = 0 and those with k >= 2."""
    src, T = check_args(g, sources, transmit, falloff, mode, reach)
    g = np.asarray(g)
    r = min(int(reach), MAX_REACH)
    table = np.asarray(T + [0], np.int64)                               # the last entry: k >= m
    ev = er.evaluated(g, mode)
    P = np.argwhere(ev)[:, ::-1].astype(np.int64)                       # (i, j, k), in the order of the linear index
    acc, sees, covered = np.zeros(len(P), np.int64), np.zeros(len(P), bool), []
    pairs = clear_pairs = two = 0
    known = {}
    for i, j, k, w in src:
        d = np.asarray((i, j, k), np.int64)[None, :] - P
        near = np.abs(d).max(axis=1) <= r if len(P) else np.zeros(0, bool)
        if (i, j, k) not in known:
            known[(i, j, k)] = walls(g, P[near], (i, j, k))
        kk = known[(i, j, k)]
        c = (w * table[np.minimum(kk, len(T))]) >> 16
        if falloff == FALLOFF_INVERSE_SQUARE:
            c = c // np.maximum(1, (d[near] ** 2).sum(axis=1))
        acc[near] += c
        sees[near] |= kk == 0
        covered.append(int((kk == 0).sum()))
        pairs, clear_pairs, two = pairs + int(near.sum()), clear_pairs + int((kk == 0).sum()), two + int((kk >= 2).sum())
    e = np.full(g.shape, -1, np.int32)
    e[ev] = acc
    s = np.zeros((), SUMMARY_DTYPE)
    s["evaluated"], s["total"], s["dark"], s["seen"] = len(P), int(acc.sum()), int((acc == 0).sum()), int(sees.sum())
    s["peak"], s["peak_voxel"] = -1, -1
    if len(P):
        top = int(np.argmax(acc))                                       # the first of equals: the smallest linear index
        s["peak"], s["peak_voxel"] = int(acc[top]), int(P[top, 0] + g.shape[2] * (P[top, 1] + g.shape[1] * P[top, 2]))
    if counts is not None:
        counts.update(pairs=pairs, clear=clear_pairs, two=two)
    return e, np.asarray(covered, np.int64), s
