"""The part-segmentation rule (rto_segment_parts, rto_edit_parts) restated in numpy int64: the reference the
GPU labels, tables and edits and host/Parts.cpp are checked against.

Voxel (i, j, k) of a (dimZ, dimY, dimX) uint8 grid has linear index v = i + dimX (j + dimY k).  S is the voxels equal to `set`;
CONN_FACE joins voxels that differ by 1 on exactly one axis, CONN_FULL voxels that differ by at most 1 on every axis.
    height  h[v] = the uncapped d2 of distance_ref from v to the voxels NOT in S (>= 1 on S), 0 off S, NONE on S when S is the grid.
    order   key(v) = (h[v], -v): a strict total order.
    ascent  up(v) = the neighbour in S with the largest key if that exceeds key(v), else v (a peak).  A basin is what ends at one
            peak; basins are numbered in ascending order of their peak's index.
    passes  adjacent (a, b) of S in different basins: height min(h[a], h[b]), index min(a, b).  A basin edge (A < B): s the largest
            pass height, at the smallest pass index that attains it, pairs the number of such voxel pairs.
    merge   edges in the order (s descending, A, B); a union-find carries P = the largest peak height of a cluster; an edge joins
            two clusters exactly when 1,000,000 s >= ratio^2 min(P, P'); the joined cluster takes the larger P.
    parts   the clusters in ascending order of their smallest voxel; labels int32, -1 off S.
    necks   one per pair of adjacent parts, sorted by (part_lo, part_hi): h the largest s among the basin edges between the two, at
            of that edge (ties in s: the smaller at), pairs summed.
    cut     every voxel of S with a neighbour in S of a LARGER part number leaves S.
The rule is stated twice: `loops` (one voxel at a time, a sorted-edge union-find) and `segment` (array shifts and pointer
doubling).  Both return a Result.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import distance_ref as dr

SET_EMPTY, SET_SOLID = 0, 1
CONN_FACE, CONN_FULL = 6, 26
NONE = dr.NONE
RATIO_MAX = 1001

PART_DTYPE = np.dtype([("root", "<i8"), ("voxels", "<i8"), ("lo", "<i4", (3,)), ("hi", "<i4", (3,)), ("touches", "<i4"), ("basins", "<i4"),
                       ("peak", "<i8"), ("peak_h", "<i4"), ("reserved", "<i4")])
NECK_DTYPE = np.dtype([("part_lo", "<i4"), ("part_hi", "<i4"), ("h", "<i4"), ("reserved", "<i4"), ("at", "<i8"), ("pairs", "<i8")])
SUMMARY_DTYPE = np.dtype([("parts", "<i8"), ("basins", "<i8"), ("necks", "<i8"), ("pairs", "<i8")])
assert PART_DTYPE.itemsize == 64 and NECK_DTYPE.itemsize == 32 and SUMMARY_DTYPE.itemsize == 32

# labels: int32 (dimZ, dimY, dimX); basin_of: the basin number per voxel (-1 off S); edges: the basin edges as rows
# (A, B, s, at, pairs) in the merge's order; heights: h as int64.
Result = namedtuple("Result", "labels parts necks summary basin_of edges heights")


def offsets(connectivity):
    """Every (dx, dy, dz) of the neighbourhood."""
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                k = (dx != 0) + (dy != 0) + (dz != 0)
                if k == 1 or (k > 1 and connectivity == CONN_FULL):
                    out.append((dx, dy, dz))
    return out


def heights(grid, set):
    g = np.asarray(grid, np.uint8)
    h = dr.field(g, 1 - set).astype(np.int64)
    h[g != set] = 0
    return h


def _joins(s, pa, pb, ratio):
    return 1000000 * int(s) >= ratio * ratio * min(int(pa), int(pb))


def _tables(shape, h, basin_of, edges, cluster, ratio):
    """The label volume, the part and neck tables and the summary from the basin volume, the basin edges and the basin -> cluster
    map (any numbering)."""
    dz, dy, dx = shape
    flat_b = basin_of.reshape(-1)
    inside = np.flatnonzero(flat_b >= 0)
    cl = np.asarray(cluster, np.int64)
    nb = len(cl)
    cv = cl[flat_b[inside]]                                                # the cluster of every voxel of S, in index order
    first = np.full(nb, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(first, cv, inside)
    ids = np.flatnonzero(first < np.iinfo(np.int64).max)
    ids = ids[np.argsort(first[ids], kind="stable")]                       # clusters in ascending order of their smallest voxel
    number = np.full(nb, -1, np.int64)
    number[ids] = np.arange(len(ids))
    part_of_basin = number[cl] if nb else np.zeros(0, np.int64)
    labels = np.full(dz * dy * dx, -1, np.int32)
    pv = part_of_basin[flat_b[inside]]
    labels[inside] = pv
    n = len(ids)
    parts = np.zeros(n, PART_DTYPE)
    parts["root"] = first[ids]
    parts["voxels"] = np.bincount(pv, minlength=n)
    x, y, z = inside % dx, (inside // dx) % dy, inside // (dx * dy)
    lo = np.full((n, 3), np.iinfo(np.int32).max, np.int64)
    hi = np.full((n, 3), -1, np.int64)
    for k, c in enumerate((x, y, z)):
        np.minimum.at(lo[:, k], pv, c)
        np.maximum.at(hi[:, k], pv, c)
    parts["lo"], parts["hi"] = lo, hi
    t = np.zeros(n, np.int64)
    for k, d in enumerate((dx, dy, dz)):
        t |= (lo[:, k] == 0).astype(np.int64) << k
        t |= (hi[:, k] == d - 1).astype(np.int64) << (3 + k)
    parts["touches"] = t
    parts["basins"] = np.bincount(part_of_basin, minlength=n) if nb else 0
    hv = h.reshape(-1)[inside]
    order = np.lexsort((-inside, hv, pv))                                  # per part, ascending key: the last entry is the peak
    last = np.flatnonzero(np.r_[pv[order][1:] != pv[order][:-1], True]) if n else np.zeros(0, np.int64)
    parts["peak"] = inside[order][last]
    parts["peak_h"] = hv[order][last]
    necks = {}
    for A, B, s, at, pairs in edges:
        a, b = int(part_of_basin[A]), int(part_of_basin[B])
        if a == b:
            continue
        k = (min(a, b), max(a, b))
        old = necks.get(k)
        if old is None:
            necks[k] = [int(s), int(at), int(pairs)]
        else:
            if (int(s), -int(at)) > (old[0], -old[1]):
                old[0], old[1] = int(s), int(at)
            old[2] += int(pairs)
    table = np.zeros(len(necks), NECK_DTYPE)
    for i, k in enumerate(sorted(necks)):
        table[i] = (k[0], k[1], necks[k][0], 0, necks[k][1], necks[k][2])
    summary = np.zeros((), SUMMARY_DTYPE)
    summary["parts"], summary["basins"], summary["necks"], summary["pairs"] = n, nb, len(table), int(table["pairs"].sum())
    return labels.reshape(shape), parts, table, summary


# ---------------------------------------------------------------- the first statement: one voxel at a time
def loops_basins(grid, set=SET_SOLID, connectivity=CONN_FACE):
    """Rules 1 to 4 one voxel at a time: (h, basin_of as a flat int64 array, the basin edges in the merge's order, the peaks).  What
    `loops` needs before the ratio comes in; a caller that wants several ratios of one grid makes it once."""
    g = np.asarray(grid, np.uint8)
    dz, dy, dx = g.shape
    h = heights(g, set)
    hf = [int(a) for a in h.reshape(-1)]
    n = g.size
    offs = offsets(connectivity)

    def neighbours(v):
        x, y, z = v % dx, (v // dx) % dy, v // (dx * dy)
        for ox, oy, oz in offs:
            a, b, c = x + ox, y + oy, z + oz
            if 0 <= a < dx and 0 <= b < dy and 0 <= c < dz:
                u = a + dx * (b + dy * c)
                if hf[u] > 0:
                    yield u

    up = [-1] * n
    for v in range(n):
        if hf[v] == 0:
            continue
        best = v
        for u in neighbours(v):
            if (hf[u], -u) > (hf[best], -best):
                best = u
        up[v] = best
    peak = [-1] * n
    for v in range(n):
        if up[v] < 0:
            continue
        chain = []
        u = v
        while peak[u] < 0 and up[u] != u:
            chain.append(u)
            u = up[u]
        top = peak[u] if peak[u] >= 0 else u
        peak[u] = top
        for w in chain:
            peak[w] = top
    peaks = sorted({p for p in peak if p >= 0})
    number = {p: i for i, p in enumerate(peaks)}
    basin_of = np.full(n, -1, np.int64)
    for v in range(n):
        if peak[v] >= 0:
            basin_of[v] = number[peak[v]]
    found = {}
    for v in range(n):
        if hf[v] == 0:
            continue
        for u in neighbours(v):
            if u < v or basin_of[u] == basin_of[v]:
                continue
            key = (int(min(basin_of[u], basin_of[v])), int(max(basin_of[u], basin_of[v])))
            s, at = min(hf[u], hf[v]), v
            e = found.get(key)
            if e is None:
                found[key] = [s, at, 1]
            else:
                if (s, -at) > (e[0], -e[1]):
                    e[0], e[1] = s, at
                e[2] += 1
    edges = sorted(((A, B, e[0], e[1], e[2]) for (A, B), e in found.items()), key=lambda r: (-r[2], r[0], r[1]))
    return h, basin_of, edges, peaks


def loops(grid, set=SET_SOLID, connectivity=CONN_FACE, ratio=800, basins=None):
    assert 0 <= ratio <= RATIO_MAX
    g = np.asarray(grid, np.uint8)
    h, basin_of, edges, peaks = loops_basins(g, set, connectivity) if basins is None else basins
    hf = h.reshape(-1)
    parent = list(range(len(peaks)))
    P = [int(hf[p]) for p in peaks]

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for A, B, s, _, _ in edges:
        a, b = find(A), find(B)
        if a != b and _joins(s, P[a], P[b], ratio):
            parent[b] = a
            P[a] = max(P[a], P[b])
    cluster = [find(a) for a in range(len(peaks))]
    basin_of = basin_of.reshape(g.shape)
    labels, parts, necks, summary = _tables(g.shape, h, basin_of, edges, cluster, ratio)
    return Result(labels, parts, necks, summary, basin_of.astype(np.int32), np.array(edges, np.int64).reshape(-1, 5), h)


# ---------------------------------------------------------------- the second statement: whole arrays
def _shift(a, off, fill):
    """out[z, y, x] = a[z + dz, y + dy, x + dx], `fill` where that lies outside."""
    ox, oy, oz = off
    dz, dy, dx = a.shape
    out = np.full(a.shape, fill, a.dtype)
    zs, zd = (slice(oz, dz), slice(0, dz - oz)) if oz >= 0 else (slice(0, dz + oz), slice(-oz, dz))
    ys, yd = (slice(oy, dy), slice(0, dy - oy)) if oy >= 0 else (slice(0, dy + oy), slice(-oy, dy))
    xs, xd = (slice(ox, dx), slice(0, dx - ox)) if ox >= 0 else (slice(0, dx + ox), slice(-ox, dx))
    out[zd, yd, xd] = a[zs, ys, xs]
    return out


def ascent(h, connectivity):
    """up as int64 (dimZ, dimY, dimX): the linear index each voxel of S steps to (itself at a peak), -1 off S."""
    idx = np.arange(h.size, dtype=np.int64).reshape(h.shape)
    best_h, best_i = h.copy(), idx.copy()
    for off in offsets(connectivity):
        nh, ni = _shift(h, off, np.int64(0)), _shift(idx, off, np.int64(-1))
        better = (nh > best_h) | ((nh == best_h) & (ni < best_i) & (ni >= 0))
        best_h, best_i = np.where(better, nh, best_h), np.where(better, ni, best_i)
    return np.where(h > 0, best_i, -1)


def basin_edges(h, basin_of, connectivity):
    """The basin edges as int64 rows (A, B, s, at, pairs) in the merge's order."""
    idx = np.arange(h.size, dtype=np.int64).reshape(h.shape)
    rows = []
    for off in offsets(connectivity):
        if (off[2], off[1], off[0]) < (0, 0, 0):
            continue                                                       # the forward half: every unordered pair once
        nb, nh = _shift(basin_of, off, np.int64(-1)), _shift(h, off, np.int64(0))
        m = (basin_of >= 0) & (nb >= 0) & (nb != basin_of)
        a, b = basin_of[m], nb[m]
        rows.append(np.stack([np.minimum(a, b), np.maximum(a, b), np.minimum(h[m], nh[m]), idx[m]], 1))
    rows = np.concatenate(rows) if rows else np.zeros((0, 4), np.int64)
    if not len(rows):
        return np.zeros((0, 5), np.int64)
    rows = rows[np.lexsort((rows[:, 3], -rows[:, 2], rows[:, 1], rows[:, 0]))]          # per (A, B): s descending, then at ascending
    start = np.flatnonzero(np.r_[True, (rows[1:, 0] != rows[:-1, 0]) | (rows[1:, 1] != rows[:-1, 1])])
    pairs = np.diff(np.r_[start, len(rows)])
    e = np.column_stack([rows[start], pairs])
    return e[np.lexsort((e[:, 1], e[:, 0], -e[:, 2]))]


def merge(edges, peak_h, ratio):
    """The basin -> cluster map (the cluster's number is one of its basins): clusters as an explicit membership array."""
    cluster = np.arange(len(peak_h), dtype=np.int64)
    P = np.array(peak_h, np.int64)
    for A, B, s, _, _ in edges:
        a, b = cluster[A], cluster[B]
        if a != b and _joins(s, P[a], P[b], ratio):
            P[a] = max(P[a], P[b])
            cluster[cluster == b] = a
    return cluster


def segment(grid, set=SET_SOLID, connectivity=CONN_FACE, ratio=800):
    assert 0 <= ratio <= RATIO_MAX
    g = np.asarray(grid, np.uint8)
    h = heights(g, set)
    up = ascent(h, connectivity).reshape(-1)
    inside = up >= 0
    root = np.where(inside, up, 0)
    while True:                                                            # pointer doubling
        nxt = root[root]
        if (nxt == root).all():
            break
        root = nxt
    peaks = np.flatnonzero(inside & (up == np.arange(up.size)))           # ascending
    basin_of = np.where(inside, np.searchsorted(peaks, root), -1).reshape(g.shape).astype(np.int64)
    edges = basin_edges(h, basin_of, connectivity)
    cluster = merge(edges, h.reshape(-1)[peaks], ratio)
    labels, parts, necks, summary = _tables(g.shape, h, basin_of, edges, cluster, ratio)
    return Result(labels, parts, necks, summary, basin_of.astype(np.int32), edges, h)


def peak_count(grid, set, connectivity):
    """The number of voxels of S with no higher-keyed neighbour, counted directly."""
    h = heights(grid, set)
    idx = np.arange(h.size, dtype=np.int64).reshape(h.shape)
    top = h > 0
    for off in offsets(connectivity):
        nh, ni = _shift(h, off, np.int64(0)), _shift(idx, off, np.int64(-1))
        top &= ~((nh > h) | ((nh == h) & (ni >= 0) & (ni < idx)))
    return int(top.sum())


def cut(grid, set=SET_SOLID, connectivity=CONN_FACE, ratio=800, labels=None):
    """(edited copy of the grid, changed) of rto_edit_parts."""
    g = np.array(grid, np.uint8)
    lab = (segment(g, set, connectivity, ratio).labels if labels is None else labels).astype(np.int64)
    hit = np.zeros(g.shape, bool)
    for off in offsets(connectivity):
        hit |= (lab >= 0) & (_shift(lab, off, np.int64(-1)) > lab)
    g[hit] = 1 - set
    return g, int(hit.sum())


# ---------------------------------------------------------------- the grids of the tests
def two_balls(dx=40, dy=24, dz=24, r=8, gap=13):
    """Two balls of radius r whose centres are `gap` voxels apart along x, centred in the grid."""
    z, y, x = np.mgrid[0:dz, 0:dy, 0:dx]
    cx = (dx - gap) // 2
    g = np.zeros((dz, dy, dx), np.uint8)
    for c in (cx, cx + gap):
        g[(x - c) ** 2 + (y - dy // 2) ** 2 + (z - dz // 2) ** 2 <= r * r] = 1
    return g


def opened_noise(dx, dy, dz, seed, fill=0.62):
    """A seeded random grid opened once (erode by one face step, dilate by one): blobs with many basins in both sets."""
    rng = np.random.default_rng(seed)
    g = (rng.random((dz, dy, dx)) < fill).astype(np.uint8)
    er = g.copy()
    for off in offsets(CONN_FACE):
        er &= _shift(g, off, np.uint8(0))
    out = er.copy()
    for off in offsets(CONN_FACE):
        out |= _shift(er, off, np.uint8(0))
    return out
