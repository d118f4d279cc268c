"""The exposure rule (rto_exposure_field) restated in numpy and plain Python: the reference the GPU fields and
summaries and the host layer's CPU form are checked against.

Voxel p = (i, j, k) has linear index v = i + dimX (j + dimY k); grids are uint8 (dimZ, dimY, dimX).  SOLID is the voxels equal to 1,
EMPTY the voxels equal to 0; voxels outside the grid do not exist and block nothing.
    ray       the open half line centre(p) + t d, t > 0; in doubled coordinates the centre is P = 2 p + 1 and voxel q the open cube
              (2 q, 2 q + 2)^3.
    crossed   q != p is crossed when some t > 0 puts P + t d strictly inside q's cube on all three axes.
    blocked   (p, d) is blocked when a crossed voxel of the grid with max-norm |q - p| <= reach is SOLID.
    e[v]      for an evaluated voxel (ALL: every EMPTY voxel; SKIN: the EMPTY voxels with a SOLID face neighbour) the sum of the
              weights of the directions that are not blocked; -1 for every other voxel.
The rule is stated twice.  (a) crossed() is the open-cube definition itself: the t-interval of every axis as a pair of integer
fractions, compared by cross-multiplication, for one (p, d) against every q of the grid at once.  (b) template() makes one period of
the crossed offsets of a direction from the sorted plane crossings t = (2 m + 1) / (2 |a|) (fractions.Fraction), and
blocked_by_template() ORs the SOLID array shifted by every entry of every period.  tests/test_exposure.py pins (a) == (b).
"""
from __future__ import annotations

from fractions import Fraction
from math import gcd

import numpy as np

EXPO_ALL, EXPO_SKIN = 0, 1
MAX_COMP = 255
MAX_DIRS = 1024
NO_LIMIT = 0x7FFFFFFF
SUMMARY_DTYPE = np.dtype([("evaluated", "<i8"), ("total", "<i8"), ("dark", "<i8"), ("open", "<i8")])

UNIT = [(x, y, z) for z in (-1, 0, 1) for y in (-1, 0, 1) for x in (-1, 0, 1) if (x, y, z) != (0, 0, 0)]
# the issue's direction set D: the 26 unit directions, general ones, one that is not primitive, and the longest periods
D = UNIT + [(1, 2, 3), (3, -1, 2), (-2, 5, 0), (7, 1, -1), (5, 3, -4), (0, 0, -3), (9, 7, -8), (-6, 4, 2), (2, 2, 0),
            (255, 1, -1), (253, 255, 254), (-255, -255, -255)]


def primitive(d):
    a, b, c = (int(v) for v in d)
    g = gcd(gcd(abs(a), abs(b)), abs(c))
    if g == 0:
        raise ValueError("a zero direction")
    return (a // g, b // g, c // g)


def template(d):
    """One period of the offsets crossed along d, in the order they are crossed, as an (entries, 3) int64 array; the last is d / gcd."""
    p = primitive(d)
    moves = {}
    for a in range(3):
        for m in range(abs(p[a])):
            moves.setdefault(Fraction(2 * m + 1, 2 * abs(p[a])), []).append(a)
    at, out = [0, 0, 0], []
    for t in sorted(moves):
        for a in moves[t]:
            at[a] += 1 if p[a] > 0 else -1
        out.append(tuple(at))
    return np.asarray(out, np.int64).reshape(-1, 3)


def crossed(shape, p, d):
    """(a) The voxels q of a (dimZ, dimY, dimX) grid whose open cube the ray from centre(p) along d meets, as a bool array: on
    every axis with d_a != 0 the times inside q's slab are the open interval (lo_a, hi_a) of fractions over |d_a|; q is crossed when
    every hi_a > 0 and every lo_a < hi_b."""
    dz, dy, dx = shape
    q = np.ogrid[0:dz, 0:dy, 0:dx][::-1]                 # x, y, z, each broadcasting over the grid
    ok = np.ones(shape, bool)
    spans = []
    for a in range(3):
        P = 2 * int(p[a]) + 1
        if d[a] == 0:
            ok &= (q[a] == p[a])
            continue
        lo = (2 * q[a] - P) if d[a] > 0 else (P - 2 * q[a] - 2)
        spans.append((lo.astype(np.int64), lo.astype(np.int64) + 2, abs(int(d[a]))))
    for lo_a, hi_a, den_a in spans:
        ok = ok & (hi_a > 0)
        for lo_b, hi_b, den_b in spans:
            ok = ok & (lo_a * den_b < hi_b * den_a)
    ok[p[2], p[1], p[0]] = False
    return ok


def blocked_by_definition(g, d, reach=NO_LIMIT):
    """(a) for every voxel of the grid as the start: bool (dimZ, dimY, dimX).  Small grids only."""
    solid = np.asarray(g) == 1
    dz, dy, dx = solid.shape
    zz, yy, xx = np.ogrid[0:dz, 0:dy, 0:dx]
    out = np.zeros(solid.shape, bool)
    for k in range(dz):
        for j in range(dy):
            for i in range(dx):
                near = np.maximum(np.maximum(abs(xx - i), abs(yy - j)), abs(zz - k)) <= reach
                out[k, j, i] = bool((crossed(solid.shape, (i, j, k), d) & near & solid).any())
    return out


def blocked_by_template(g, d, reach=NO_LIMIT):
    """(b) blocked[p] = OR over the periods k and the template's entries o, while max-norm |k d + o| <= reach and some voxel still
    has p + k d + o inside the grid, of SOLID[p + k d + o]."""
    solid = np.asarray(g) == 1
    dz, dy, dx = solid.shape
    dims = (dx, dy, dz)
    offs, p = template(d), np.asarray(primitive(d), np.int64)
    out = np.zeros(solid.shape, bool)
    k = 0
    while True:
        for o in offs:
            r = k * p + o
            # |r| grows on every axis along the ray: the first entry beyond the reach or the grid's size ends it
            if np.abs(r).max() > reach or (np.abs(r) >= dims).any():
                return out
            rx, ry, rz = (int(v) for v in r)
            dst = tuple(slice(max(0, -s), n - max(0, s)) for s, n in ((rz, dz), (ry, dy), (rx, dx)))
            src = tuple(slice(max(0, s), n - max(0, -s)) for s, n in ((rz, dz), (ry, dy), (rx, dx)))
            out[dst] |= solid[src]
        k += 1


def evaluated(g, mode):
    g = np.asarray(g)
    empty = g == 0
    if mode == EXPO_ALL:
        return empty
    solid = np.pad(g == 1, 1)
    near = (solid[1:-1, 1:-1, :-2] | solid[1:-1, 1:-1, 2:] | solid[1:-1, :-2, 1:-1] | solid[1:-1, 2:, 1:-1] | solid[:-2, 1:-1, 1:-1] |
            solid[2:, 1:-1, 1:-1])
    return empty & near


def check_args(dirs, weights, mode, reach):
    if dirs is None:
        raise ValueError("dirs is NULL")
    dirs = [tuple(int(c) for c in d) for d in dirs]
    if not 1 <= len(dirs) <= MAX_DIRS:
        raise ValueError("n out of range")
    for d in dirs:
        if d == (0, 0, 0) or max(abs(c) for c in d) > MAX_COMP:
            raise ValueError("a bad direction")
    w = [1] * len(dirs) if weights is None else [int(v) for v in weights]
    if len(w) != len(dirs) or min(w) < 0 or sum(w) > 2 ** 31 - 1:
        raise ValueError("bad weights")
    if mode not in (EXPO_ALL, EXPO_SKIN):
        raise ValueError("unknown mode")
    if reach < 1:
        raise ValueError("reach below 1")
    return dirs, w


def exposure(g, dirs, weights=None, mode=EXPO_SKIN, reach=NO_LIMIT, blocked=blocked_by_template, counts=None):
    """(e int32 (dimZ, dimY, dimX), the summary as a SUMMARY_DTYPE scalar).  `counts`, a dict, receives 'pairs' and 'blocked': the
    (evaluated voxel, direction) pairs and how many of them are blocked."""
    dirs, w = check_args(dirs, weights, mode, reach)
    g = np.asarray(g)
    ev = evaluated(g, mode)
    total = np.zeros(g.shape, np.int64)
    seen = {}
    nblocked = 0
    for d, wd in zip(dirs, w):
        key = primitive(d)
        if key not in seen:
            seen[key] = blocked(g, key, reach)
        total += np.where(seen[key], 0, wd)
        nblocked += int((seen[key] & ev).sum())
    e = np.where(ev, total, -1).astype(np.int32)
    s = np.zeros((), SUMMARY_DTYPE)
    s["evaluated"] = int(ev.sum())
    s["total"] = int(total[ev].sum())
    s["dark"] = int((total[ev] == 0).sum())
    s["open"] = int((total[ev] == sum(w)).sum())
    if counts is not None:
        counts["pairs"] = int(ev.sum()) * len(dirs)
        counts["blocked"] = nblocked
    return e, s


def hemisphere(n=64):
    """n float directions of the upper hemisphere (z > 0), a Fibonacci spiral: for hip.quantize_directions."""
    i = np.arange(n) + 0.5
    z = i / n
    r = np.sqrt(1.0 - z * z)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)
