"""The skeleton rule (rto_skeleton_field / rto_edit_skeleton) restated in numpy and plain Python: the
reference the GPU fields, summaries and edits and the host layer's CPU form are checked against.

Voxel (i, j, k) has linear index v = i + dimX (j + dimY k); grids are uint8 (dimZ, dimY, dimX).  SET_SOLID is the voxels equal to 1,
SET_EMPTY the voxels equal to 0; a voxel outside the grid is NOT in the set (section 22's convention, not section 19's).
    mask      the 27 bits of a voxel's 3 x 3 x 3 block, bit b = (dx + 1) + 3 (dy + 1) + 9 (dz + 1); bit 13 is the voxel itself.
    FULL      joins X by 26 and its complement by 6; FACE joins X by 6 and its complement by 26.
    simple    FULL: X n N26* is non-empty and 26-connected; with B = N18* \\ X, B n N6* is non-empty and lies in one 6-component
              of B.  FACE: the same of the complemented neighbourhood.
    pass p    M = the voxels of X with a neighbour (6 under FULL, 26 under FACE) not in X, fixed for the pass; then for
              s = 0 .. 7 every voxel of subfield s = (i & 1) + 2 (j & 1) + 4 (k & 1) that is in M, no anchor, not kept by the
              mode and simple leaves X, all of them at once.  The first pass that removes nothing ends the thinning.
    CURVE     keeps a voxel with exactly one neighbour in X among its 26 (FULL only).
    k[v]      -1 outside the set, 0 for the skeleton, p >= 1 for the pass that removed v.
The simple test is stated twice: simple() floods inside the mask with shifts, on whole arrays of masks at once; simple_slow() walks
the 27 cells with a stack.  tests/test_skeleton.py pins both to scipy.ndimage.label.
"""
from __future__ import annotations

import numpy as np

SET_EMPTY, SET_SOLID = 0, 1
CONN_FACE, CONN_FULL = 6, 26
SKEL_TOPOLOGY, SKEL_CURVE = 0, 1
NO_LIMIT = 0x7FFFFFFF
SUMMARY_DTYPE = np.dtype([("kept", "<i8"), ("removed", "<i8"), ("passes", "<i8"), ("reserved", "<i8")])

ALL27 = (1 << 27) - 1
N26 = ALL27 & ~(1 << 13)


def _bits(pred):
    m = 0
    for b in range(27):
        if pred(b % 3 - 1, (b // 3) % 3 - 1, b // 9 - 1):
            m |= 1 << b
    return m


N18 = _bits(lambda x, y, z: 1 <= abs(x) + abs(y) + abs(z) <= 2)
N6 = _bits(lambda x, y, z: abs(x) + abs(y) + abs(z) == 1)
_X0, _X2 = _bits(lambda x, y, z: x == -1), _bits(lambda x, y, z: x == 1)
_Y0, _Y2 = _bits(lambda x, y, z: y == -1), _bits(lambda x, y, z: y == 1)


def _u(v):
    return np.uint32(v)


def _sx(m):
    return m | ((m << _u(1)) & _u(ALL27 & ~_X0)) | ((m >> _u(1)) & _u(ALL27 & ~_X2))


def _sy(m):
    return m | ((m << _u(3)) & _u(ALL27 & ~_Y0)) | ((m >> _u(3)) & _u(ALL27 & ~_Y2))


def _sz(m):
    return m | ((m << _u(9)) & _u(ALL27)) | (m >> _u(9))


def _dilate26(m):
    return _sz(_sy(_sx(m)))


def _dilate6(m):
    return _sx(m) | _sy(m) | _sz(m)


def _flood(start, inside, dilate):
    f = start
    while True:
        g = dilate(f) & inside
        if np.array_equal(g, f):
            return f
        f = g


def simple_full(n):
    """n: uint32 array of neighbourhood masks (bit 13 ignored).  True where the centre is a simple point under FULL."""
    n = np.asarray(n, dtype=np.uint32) & _u(N26)
    low = n & (~n + _u(1))
    ok = (n != 0) & (_flood(low, n, _dilate26) == n)
    b = ~n & _u(N18)
    b6 = b & _u(N6)
    low = b6 & (~b6 + _u(1))
    reach = _flood(low, b, _dilate6)
    return ok & (b6 != 0) & ((reach & b6) == b6)


def simple(n, connectivity):
    n = np.asarray(n, dtype=np.uint32)
    return simple_full(n if connectivity == CONN_FULL else ~n & _u(N26))


def _components(cells, adjacent):
    """The components of a list of (x, y, z) cells under `adjacent`."""
    left, out = set(cells), []
    while left:
        stack, comp = [left.pop()], set()
        while stack:
            c = stack.pop()
            comp.add(c)
            for d in list(left):
                if adjacent(c, d):
                    left.discard(d)
                    stack.append(d)
        out.append(comp)
    return out


def simple_slow(mask, connectivity):
    """The definition, cell by cell, for one mask."""
    cells = [(b % 3 - 1, (b // 3) % 3 - 1, b // 9 - 1) for b in range(27) if b != 13]
    inx = {c for b, c in zip([b for b in range(27) if b != 13], cells) if (mask >> b) & 1}
    out = set(cells) - inx
    adj26 = lambda a, b: max(abs(a[0] - b[0]), abs(a[1] - b[1]), abs(a[2] - b[2])) == 1
    adj6 = lambda a, b: abs(a[0] - b[0]) + abs(a[1] - b[1]) + abs(a[2] - b[2]) == 1
    l1 = lambda c: abs(c[0]) + abs(c[1]) + abs(c[2])
    big, small = (inx, out) if connectivity == CONN_FULL else (out, inx)      # big joins by 26, small by 6
    if not big or len(_components(sorted(big), adj26)) != 1:
        return False
    s18 = [c for c in small if l1(c) <= 2]
    s6 = [c for c in small if l1(c) == 1]
    if not s6:
        return False
    return sum(1 for comp in _components(sorted(s18), adj6) if any(c in comp for c in s6)) == 1


def _shifted(p, dx, dy, dz):
    nz, ny, nx = p.shape[0] - 2, p.shape[1] - 2, p.shape[2] - 2
    return p[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]


def marked(x, connectivity):
    """M: the voxels of the boolean volume x with a neighbour not in x; beyond the grid is not in x."""
    p = np.pad(x, 1)
    allin = np.ones_like(x)
    for b in range(27):
        d = (b % 3 - 1, (b // 3) % 3 - 1, b // 9 - 1)
        if b == 13 or (connectivity == CONN_FULL and abs(d[0]) + abs(d[1]) + abs(d[2]) != 1):
            continue
        allin &= _shifted(p, *d)
    return x & ~allin


def masks_at(x, idx):
    """The 27-bit masks of the voxels idx = (z, y, x index arrays) of the boolean volume x."""
    p = np.pad(x, 1)
    m = np.zeros(len(idx[0]), dtype=np.uint32)
    for b in range(27):
        dx, dy, dz = b % 3 - 1, (b // 3) % 3 - 1, b // 9 - 1
        m |= p[idx[0] + 1 + dz, idx[1] + 1 + dy, idx[2] + 1 + dx].astype(np.uint32) << _u(b)
    return m


def check_args(grid, set, connectivity, mode, anchors, max_passes):
    if set not in (SET_SOLID, SET_EMPTY):
        raise ValueError("unknown set")
    if connectivity not in (CONN_FACE, CONN_FULL):
        raise ValueError("connectivity must be 6 or 26")
    if mode not in (SKEL_TOPOLOGY, SKEL_CURVE):
        raise ValueError("unknown mode")
    if mode == SKEL_CURVE and connectivity != CONN_FULL:
        raise ValueError("CURVE needs FULL")
    if max_passes < 1:
        raise ValueError("max_passes is below 1")
    a = np.asarray(anchors, dtype=np.int64).reshape(-1)
    if len(a) and (a.min() < 0 or a.max() >= grid.size):
        raise ValueError("an anchor is not a voxel of the grid")
    return a


def skeleton(grid, set=SET_SOLID, connectivity=CONN_FULL, mode=SKEL_TOPOLOGY, anchors=(), max_passes=NO_LIMIT):
    """k (int32, the grid's shape) and the summary record."""
    a = check_args(grid, set, connectivity, mode, anchors, max_passes)
    x = grid == (1 if set == SET_SOLID else 0)
    k = np.where(x, 0, -1).astype(np.int32)
    anchor = np.zeros(grid.shape, dtype=bool)
    anchor.reshape(-1)[a] = True
    zz, yy, xx = np.indices(grid.shape, sparse=True)
    sub = ((xx & 1) + 2 * (yy & 1) + 4 * (zz & 1)).astype(np.uint8) + np.zeros(grid.shape, dtype=np.uint8)
    p = 0
    while p < min(max_passes, NO_LIMIT):
        p += 1
        cand = marked(x, connectivity) & ~anchor
        gone = 0
        for s in range(8):
            idx = np.nonzero(cand & (sub == s))
            if not len(idx[0]):
                continue
            m = masks_at(x, idx)
            ok = simple(m, connectivity)
            if mode == SKEL_CURVE:
                n = m & _u(N26)
                ok &= ~((n != 0) & ((n & (n - _u(1))) == 0))
            sel = tuple(i[ok] for i in idx)
            x[sel] = False
            k[sel] = p
            gone += int(ok.sum())
        if gone == 0:
            p -= 1
            break
    summary = np.zeros((), dtype=SUMMARY_DTYPE)
    summary["kept"] = int((k == 0).sum())
    summary["removed"] = int((k > 0).sum())
    summary["passes"] = int(k.max()) if (k > 0).any() else 0
    return k, summary


def edit(grid, set=SET_SOLID, connectivity=CONN_FULL, mode=SKEL_TOPOLOGY, anchors=(), max_passes=NO_LIMIT):
    """The grid after rto_edit_skeleton and the number of voxels flipped."""
    k, _ = skeleton(grid, set, connectivity, mode, anchors, max_passes)
    out = grid.copy()
    out[k > 0] = 0 if set == SET_SOLID else 1
    return out, int((k > 0).sum())


# ---- the grids of the closed forms (ISSUE / DESIGN section 23)
def ball(n, r):
    c = (n - 1) / 2
    z, y, x = np.indices((n, n, n))
    return (((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) <= r * r).astype(np.uint8)


def torus(n, R, r):
    c = (n - 1) / 2
    z, y, x = np.indices((n, n, n))
    q = np.sqrt((x - c) ** 2 + (y - c) ** 2) - R
    return ((q * q + (z - c) ** 2) <= r * r).astype(np.uint8)


def shell(n, r0, r1):
    c = (n - 1) / 2
    z, y, x = np.indices((n, n, n))
    d2 = (x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2
    return ((d2 >= r0 * r0) & (d2 <= r1 * r1)).astype(np.uint8)


def bar():
    return np.ones((5, 5, 40), dtype=np.uint8)            # 40 along x


def block():
    return np.ones((24, 24, 96), dtype=np.uint8)          # 96 x 24 x 24
