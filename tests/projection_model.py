"""A scalar model of k_project_march's traversal (csrc/rto_project.inc) for the tests: the same float32 operations in the same
order, but none of the statement's sorting.  Entry by rank (the largest entering event against every leaving event, the other
axes' coordinates by a binary search over their monotone T), the step (the next event's T per axis, recomputed from the plane
index), and the brick jump (the smallest leaving plane of the brick; the other axes cross what is ordered before it).
tests/test_projection.py holds it against tests/projection_ref.py's walk."""
from __future__ import annotations

import numpy as np

F = np.float32
STILL = float("inf"), 1          # sorts above every (T, 0): a still axis has no next event


class Axis:
    def __init__(self, o, inv, g, vs, dim, lo, hi):
        self.o, self.inv, self.g, self.vs, self.dim, self.lo, self.hi = F(o), F(inv), F(g), F(vs), dim, lo, hi
        self.moving = bool(np.isfinite(inv))
        self.up = bool(inv > 0)
        self.step = (1 if self.up else -1) if self.moving else 0
        self.c = 0
        self.next = STILL

    def t(self, j):
        with np.errstate(all="ignore"):
            return F(F(F(self.g + F(F(j) * self.vs)) - self.o) * self.inv)

    def arm(self):
        self.next = (float(self.t(self.c + (1 if self.up else 0))), 0) if self.moving else STILL

    def advance(self):
        self.c += self.step
        self.arm()

    def rank(self, t, incl):
        a, b = 0, self.dim + 1
        while a < b:
            mid = (a + b) >> 1
            tm = self.t(mid if self.up else self.dim - mid)
            if (tm <= t) if incl else (tm < t):
                a = mid + 1
            else:
                b = mid
        return a

    def inside(self):
        return self.lo <= self.c < self.hi

    def brick_exit(self):
        b = self.c >> 3
        return min(b * 8 + 8, self.dim) if self.up else b * 8


def entry(grid_min, voxel, dim, o, d, lo, hi):
    """The three axes at the first visited state, or None for a miss."""
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    with np.errstate(all="ignore"):
        inv = (F(1) / d).astype(np.float32)
    if not np.isfinite(o).all():
        return None
    ax = [Axis(o[a], inv[a], grid_min[a], voxel, dim[a], lo[a], hi[a]) for a in range(3)]
    if not any(A.moving for A in ax):
        return None
    t_in, t_out, need = [F(0)] * 3, [F(0)] * 3, [False] * 3
    for a, A in enumerate(ax):
        if not A.moving:
            with np.errstate(all="ignore"):
                q = np.floor(F(F(A.o - A.g) / A.vs))
            if not (q >= F(A.lo) and q < F(A.hi)):
                return None
            A.c = int(q)
            continue
        t_in[a], t_out[a] = A.t(A.lo if A.up else A.hi), A.t(A.hi if A.up else A.lo)
        need[a] = bool(t_in[a] > 0)
        if not t_out[a] > 0:
            return None
    e_t, e_axis = F(0), 3
    for a in range(3):
        if need[a] and (e_axis == 3 or t_in[a] >= e_t):
            e_t, e_axis = t_in[a], a
    if e_axis != 3:
        for b, B in enumerate(ax):
            if B.moving and b != e_axis and not (e_t < t_out[b] or (e_t == t_out[b] and e_axis < b)):
                return None
    for b, B in enumerate(ax):
        if not B.moving:
            continue
        if b == e_axis:
            B.c = B.lo if B.up else B.hi - 1
        else:
            n = B.rank(e_t, b < e_axis)
            B.c = n - 1 if B.up else B.dim - n
    for A in ax:
        A.arm()
    return ax if all(A.inside() for A in ax) else None


def march(grid_min, voxel, dim, o, d, lo=None, hi=None, skip=lambda brick: False):
    """(cells sampled, bricks consulted as (brick, the cell it was entered at)) of one ray; skip(brick) stands for the table."""
    lo = (0, 0, 0) if lo is None else lo
    hi = tuple(dim) if hi is None else hi
    ax = entry(grid_min, voxel, dim, o, d, lo, hi)
    cells, bricks = [], []
    if ax is None:
        return cells, bricks
    X, Y, Z = ax
    last, skipping = None, False
    budget = sum(dim) + 4
    while True:
        brick = (X.c >> 3, Y.c >> 3, Z.c >> 3)
        if brick != last:
            last = brick
            bricks.append((brick, (X.c, Y.c, Z.c)))
            skipping = skip(brick)
        if skipping:
            js = [A.brick_exit() for A in ax]
            ts = [(float(A.t(j)), 0) if A.moving else STILL for A, j in zip(ax, js)]
            m = 0 if ts[0] <= ts[1] and ts[0] <= ts[2] else (1 if ts[1] <= ts[2] else 2)
            for b, B in enumerate(ax):
                if b == m:
                    continue
                i = 0
                while i < 8 and (B.next < ts[m] or (b < m and B.next == ts[m])):
                    B.advance()
                    i += 1
            ax[m].c = js[m] if ax[m].up else js[m] - 1
            ax[m].arm()
        else:
            cells.append((X.c, Y.c, Z.c))
            if X.next <= Y.next and X.next <= Z.next:
                X.advance()
            elif Y.next <= Z.next:
                Y.advance()
            else:
                Z.advance()
        budget -= 1
        if not (all(A.inside() for A in ax) and budget > 0):
            return cells, bricks
