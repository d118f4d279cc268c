"""The connected-component rule of include/rto_hip.h in numpy alone.

Voxel (i, j, k) of a (dimZ, dimY, dimX) uint8 grid has linear index v = i + dimX (j + dimY k).  The set is the voxels equal to 1
(SET_SOLID) or 0 (SET_EMPTY); CONN_FACE joins voxels that differ by 1 on exactly one axis, CONN_FULL voxels that differ by at most
1 on every axis.  A component's root is its smallest linear index, components are numbered in ascending order of root, the label
volume holds that number and -1 outside the set.

Method: maximal x-runs of the set are labelled first (their order is the order of their first voxels), runs of neighbouring
rows that overlap (FULL: after widening by one voxel) are joined by a union-find over run numbers that always hooks the larger
root under the smaller, so a component's final root is its first run.
"""
from __future__ import annotations

import numpy as np

SET_EMPTY, SET_SOLID = 0, 1
CONN_FACE, CONN_FULL = 6, 26
SELECT_SMALLER_THAN, SELECT_ALL_BUT_LARGEST, SELECT_ENCLOSED, SELECT_CONTAINING, SELECT_NOT_CONTAINING = 0, 1, 2, 3, 4

COMPONENT_DTYPE = np.dtype([("root", "<i8"), ("voxels", "<i8"), ("lo", "<i4", (3,)), ("hi", "<i4", (3,)), ("touches", "<i4"),
                            ("reserved", "<i4")])


def _union(n, a, b):
    """Roots of the union-find over 0 .. n-1 with the edges (a[i], b[i]): parent[i] = the smallest member of i's class."""
    parent = np.arange(n, dtype=np.int64)
    while len(a):
        pa, pb = parent[a], parent[b]
        diff = pa != pb
        if not diff.any():
            break
        a, b, pa, pb = a[diff], b[diff], pa[diff], pb[diff]
        np.minimum.at(parent, np.maximum(pa, pb), np.minimum(pa, pb))      # hook the larger root under the smaller
        while True:                                                        # full compression
            pp = parent[parent]
            if (pp == parent).all():
                break
            parent = pp
    return parent


def label(grid, set=SET_SOLID, connectivity=CONN_FACE):
    """(labels int32 (dimZ, dimY, dimX), table COMPONENT_DTYPE) of the rule."""
    assert set in (SET_EMPTY, SET_SOLID) and connectivity in (CONN_FACE, CONN_FULL)
    g = np.asarray(grid)
    dz, dy, dx = g.shape
    m = (g == set).reshape(dz * dy, dx)
    labels = np.full(m.shape, -1, np.int32)
    if not m.any():
        return labels.reshape(dz, dy, dx), np.zeros(0, COMPONENT_DTYPE)
    # runs, in (row, x) order == order of their first voxel's linear index
    pad = np.zeros((m.shape[0], 1), bool)
    e = np.concatenate([pad, m, pad], 1).astype(np.int8)
    d = np.diff(e, axis=1)
    rrow, x0 = np.nonzero(d == 1)                                          # row-major: sorted by (row, x)
    _, x1 = np.nonzero(d == -1)
    x1 = x1 - 1                                                            # inclusive
    R = len(rrow)
    ry, rz = rrow % dy, rrow // dy
    W = dx + 4
    skey = rrow.astype(np.int64) * W + x0                                   # ascending
    ekey = rrow.astype(np.int64) * W + x1
    dil = 1 if connectivity == CONN_FULL else 0
    dirs = [(1, 0), (0, 1)] if connectivity == CONN_FACE else [(1, 0), (-1, 1), (0, 1), (1, 1)]
    ea, eb = [], []
    for ddy, ddz in dirs:
        ny, nz = ry + ddy, rz + ddz
        ok = (ny >= 0) & (ny < dy) & (nz < dz)
        src = np.nonzero(ok)[0]
        nrow = (nz[src] * dy + ny[src]).astype(np.int64)
        first = np.searchsorted(ekey, nrow * W + np.maximum(x0[src] - dil, 0), "left")       # first run ending at or after a0 - dil
        last = np.searchsorted(skey, nrow * W + x1[src] + dil, "right") - 1                  # last run starting at or before a1 + dil
        cnt = np.maximum(last - first + 1, 0)
        if cnt.sum() == 0:
            continue
        a = np.repeat(src, cnt)
        offs = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        b = np.repeat(first, cnt) + offs
        ea.append(a)
        eb.append(b)
    parent = _union(R, np.concatenate(ea) if ea else np.zeros(0, np.int64), np.concatenate(eb) if eb else np.zeros(0, np.int64))
    roots = np.nonzero(parent == np.arange(R))[0]                          # ascending run number == ascending first voxel
    comp_of_run = np.searchsorted(roots, parent).astype(np.int32)
    n = len(roots)
    table = np.zeros(n, COMPONENT_DTYPE)
    table["root"] = skey[roots] // W * dx + skey[roots] % W
    length = (x1 - x0 + 1).astype(np.int64)
    table["voxels"] = np.bincount(comp_of_run, weights=length, minlength=n).astype(np.int64)
    lo = np.full((n, 3), np.iinfo(np.int32).max, np.int64)
    hi = np.full((n, 3), -1, np.int64)
    for k, (vlo, vhi) in enumerate(((x0, x1), (ry, ry), (rz, rz))):
        np.minimum.at(lo[:, k], comp_of_run, vlo)
        np.maximum.at(hi[:, k], comp_of_run, vhi)
    table["lo"], table["hi"] = lo, hi
    dims = (dx, dy, dz)
    t = np.zeros(n, np.int64)
    for k in range(3):
        t |= (lo[:, k] == 0).astype(np.int64) << k
        t |= (hi[:, k] == dims[k] - 1).astype(np.int64) << (3 + k)
    table["touches"] = t
    # label volume: the run number of every voxel of the set, through the run -> component table
    start = np.zeros(m.shape, np.int32)
    start[rrow, x0] = 1
    run_of_voxel = np.cumsum(start.reshape(-1), dtype=np.int64).reshape(m.shape) - 1
    labels[m] = comp_of_run[run_of_voxel[m]]
    return labels.reshape(dz, dy, dx), table


def select(labels, table, select, arg=0):
    """The bool mask over components that `select` picks (rto_edit_components' table)."""
    n = len(table)
    if select == SELECT_SMALLER_THAN:
        return table["voxels"] < arg
    if select == SELECT_ALL_BUT_LARGEST:
        s = np.ones(n, bool)
        if n:
            s[int(np.argmax(table["voxels"]))] = False                     # argmax: the first (smallest root) of equals
        return s
    if select == SELECT_ENCLOSED:
        return table["touches"] == 0
    at = int(labels.reshape(-1)[arg])
    if at < 0:
        return np.zeros(n, bool)
    s = np.arange(n) == at
    return s if select == SELECT_CONTAINING else ~s


def apply_selection(grid, set, connectivity, sel, arg=0):
    """(edited grid, changed) of rto_edit_components(set, connectivity, sel, arg) on a copy of `grid`."""
    g = np.array(grid, np.uint8)
    labels, table = label(g, set, connectivity)
    s = select(labels, table, sel, arg)
    hit = (labels >= 0) & np.concatenate([s, [False]])[labels]             # labels == -1 indexes the appended False
    g[hit] = 0 if set == SET_SOLID else 1
    return g, int(hit.sum())


def brute_force(grid, set=SET_SOLID, connectivity=CONN_FACE):
    """The statement itself, for tiny grids: flood fill in ascending index order.  (labels, table)."""
    g = np.asarray(grid)
    dz, dy, dx = g.shape
    labels = np.full(g.shape, -1, np.int32)
    rows = []
    for seed in range(g.size):
        z, y, x = seed // (dx * dy), (seed // dx) % dy, seed % dx
        if g[z, y, x] != set or labels[z, y, x] >= 0:
            continue
        cid = len(rows)
        labels[z, y, x] = cid
        stack, members = [(x, y, z)], []
        while stack:
            p = stack.pop()
            members.append(p)
            for ddz in (-1, 0, 1):
                for ddy in (-1, 0, 1):
                    for ddx in (-1, 0, 1):
                        k = (ddx != 0) + (ddy != 0) + (ddz != 0)
                        if k == 0 or (connectivity == CONN_FACE and k != 1):
                            continue
                        q = (p[0] + ddx, p[1] + ddy, p[2] + ddz)
                        if not (0 <= q[0] < dx and 0 <= q[1] < dy and 0 <= q[2] < dz):
                            continue
                        if g[q[2], q[1], q[0]] != set or labels[q[2], q[1], q[0]] >= 0:
                            continue
                        labels[q[2], q[1], q[0]] = cid
                        stack.append(q)
        mm = np.array(members)
        lo, hi = mm.min(0), mm.max(0)
        dims = (dx, dy, dz)
        t = sum((1 << a) for a in range(3) if lo[a] == 0) + sum((8 << a) for a in range(3) if hi[a] == dims[a] - 1)
        rows.append((seed, len(members), lo, hi, t, 0))
    table = np.zeros(len(rows), COMPONENT_DTYPE)
    for i, r in enumerate(rows):
        table[i] = r
    return labels, table
