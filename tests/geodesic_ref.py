"""The rule of the geodesic distance fields (include/rto_hip.h, rto_geodesic_field / rto_geodesic_paths / rto_edit_geodesic;
DESIGN.md section 20), stated as a heap Dijkstra in plain Python over numpy arrays, with the paths, the summary and the flood.

  index   voxel (i, j, k) has linear index v = i + dimX (j + dimY k); grids are uint8 arrays of shape (dimZ, dimY, dimX)
  medium  SET_EMPTY: the bytes equal to 0, SET_SOLID: the bytes equal to 1; a path stays inside it
  moves   CONN_FACE: the 6 face neighbours, weight 1; CONN_FULL: the 26 neighbours, weight 3 / 4 / 5 for 1 / 2 / 3 changed
          coordinates.  A move needs both ends in the medium and nothing else.
  field   g[v] = the smallest total weight of a path from any seed (linear indices; those outside the medium are ignored) to v, int32;
          NONE outside the medium, out of reach, or above the limit
  paths   from a target down to g == 0: the next voxel is the smallest linear index among the neighbours u with g[u] finite and
          g[u] + w == g[current]
This file is the tests' statement of the rule: it shares no code with the library."""
from __future__ import annotations

import heapq

import numpy as np

SET_SOLID, SET_EMPTY = 1, 0
CONN_FACE, CONN_FULL = 6, 26
NONE = 0x7fffffff
NO_LIMIT = 0x7fffffff
SUMMARY_DTYPE = np.dtype([("max_g", "<i8"), ("argmax", "<i8"), ("reached", "<i8"), ("reserved", "<i8")])


def moves(connectivity):
    """(dz, dy, dx, weight) of every move, in ascending order of the neighbour's linear index."""
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                changed = (dx != 0) + (dy != 0) + (dz != 0)
                if changed == 0 or (connectivity == CONN_FACE and changed != 1):
                    continue
                out.append((dz, dy, dx, 1 if connectivity == CONN_FACE else 2 + changed))
    return out


def check_seeds(grid, seeds):
    s = np.asarray(seeds, np.int64).reshape(-1)
    if s.size < 1 or (s < 0).any() or (s >= grid.size).any():
        raise ValueError("seeds: at least one, each a voxel of the grid")
    return s


def field(grid, seeds, medium=SET_EMPTY, connectivity=CONN_FACE, limit=None):
    """The field by Dijkstra's algorithm with a binary heap, on the grid padded by one voxel of "not the medium"."""
    grid = np.asarray(grid)
    if medium not in (SET_SOLID, SET_EMPTY) or connectivity not in (CONN_FACE, CONN_FULL):
        raise ValueError("unknown medium or connectivity")
    if limit is not None and limit < 0:
        raise ValueError("limit is negative")
    s = check_seeds(grid, seeds)
    reach = NONE - 1 if limit is None or limit >= NO_LIMIT else int(limit)
    dz, dy, dx = grid.shape
    py, px = dy + 2, dx + 2
    inside = np.zeros((dz + 2, py, px), bool)
    inside[1:-1, 1:-1, 1:-1] = grid == medium
    inside = inside.reshape(-1).tolist()
    steps = [((mz * py + my) * px + mx, w) for mz, my, mx, w in moves(connectivity)]
    dist = [NONE] * len(inside)
    heap = []
    for v in s.tolist():
        p = ((v // (dx * dy) + 1) * py + (v // dx) % dy + 1) * px + v % dx + 1
        if inside[p] and dist[p] != 0:
            dist[p] = 0
            heap.append((0, p))
    heapq.heapify(heap)
    while heap:
        d, p = heapq.heappop(heap)
        if d != dist[p]:
            continue
        for off, w in steps:
            q = p + off
            nd = d + w
            if inside[q] and nd < dist[q] and nd <= reach:
                dist[q] = nd
                heapq.heappush(heap, (nd, q))
    out = np.asarray(dist, np.int64).reshape(dz + 2, py, px)[1:-1, 1:-1, 1:-1]
    return np.ascontiguousarray(out, np.int32)


def threshold(g, limit):
    """A limited field from the unlimited one: values above the limit become NONE."""
    if limit is None or limit >= NO_LIMIT:
        return g.copy()
    out = g.copy()
    out[g > limit] = NONE
    return out


def summary(g):
    flat = np.asarray(g).reshape(-1)
    finite = flat != NONE
    out = np.zeros((), SUMMARY_DTYPE)
    out["reached"] = int(finite.sum())
    if finite.any():
        m = int(flat[finite].max())
        out["max_g"] = m
        out["argmax"] = int(np.flatnonzero(flat == m)[0])
    else:
        out["max_g"] = out["argmax"] = -1
    return out


def paths(g, connectivity, targets, max_len):
    """(rows (n, max_len) int64 with -1 behind each path, lengths (n,) int64 with -1 for a target the field does not reach)."""
    g = np.asarray(g)
    dz, dy, dx = g.shape
    flat = g.reshape(-1)
    t = np.asarray(targets, np.int64).reshape(-1)
    if t.size < 1 or (t < 0).any() or (t >= flat.size).any() or max_len < 0:
        raise ValueError("targets: at least one, each a voxel of the grid; max_len >= 0")
    rows = np.full((t.size, max_len), -1, np.int64)
    lengths = np.full(t.size, -1, np.int64)
    mv = moves(connectivity)
    for i, p in enumerate(t.tolist()):
        if flat[p] == NONE:
            continue
        n = 0
        while True:
            if n < max_len:
                rows[i, n] = p
            n += 1
            gp = int(flat[p])
            if gp == 0:
                break
            x, y, z = p % dx, (p // dx) % dy, p // (dx * dy)
            nxt = None
            for mz, my, mx, w in mv:                       # ascending linear index: the first match is the smallest
                a, b, c = x + mx, y + my, z + mz
                if 0 <= a < dx and 0 <= b < dy and 0 <= c < dz:
                    u = a + dx * (b + dy * c)
                    if flat[u] != NONE and int(flat[u]) + w == gp:
                        nxt = u
                        break
            assert nxt is not None, "a finite voxel above 0 always has a predecessor"
            p = nxt
        lengths[i] = n
    return rows, lengths


def flood(grid, seeds, medium=SET_EMPTY, connectivity=CONN_FACE, limit=None):
    """rto_edit_geodesic: (the grid with every reached voxel flipped, the number flipped)."""
    g = field(grid, seeds, medium, connectivity, limit)
    out = np.array(grid, np.uint8, copy=True)
    hit = g != NONE
    out[hit] = 1 - medium
    return out, int(hit.sum())


def scipy_field(grid, seeds, medium, connectivity):
    """The second witness: scipy's Dijkstra (min_only) on the explicit graph of moves; unlimited."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    grid = np.asarray(grid)
    dz, dy, dx = grid.shape
    inside = grid == medium
    idx = np.arange(grid.size).reshape(grid.shape)
    src, dst, wt = [], [], []
    for mz, my, mx, w in moves(connectivity):
        a = (slice(max(0, -mz), dz - max(0, mz)), slice(max(0, -my), dy - max(0, my)), slice(max(0, -mx), dx - max(0, mx)))
        b = (slice(max(0, mz), dz - max(0, -mz)), slice(max(0, my), dy - max(0, -my)), slice(max(0, mx), dx - max(0, -mx)))
        both = inside[a] & inside[b]
        src.append(idx[a][both]); dst.append(idx[b][both]); wt.append(np.full(int(both.sum()), w, np.float64))
    graph = coo_matrix((np.concatenate(wt), (np.concatenate(src), np.concatenate(dst))), shape=(grid.size, grid.size)).tocsr()
    s = check_seeds(grid, seeds)
    s = np.unique(s[inside.reshape(-1)[s]])
    out = np.full(grid.size, NONE, np.int32)
    if s.size:
        d = dijkstra(graph, directed=True, indices=s, min_only=True)
        ok = np.isfinite(d)
        out[ok] = d[ok].astype(np.int32)
    return out.reshape(grid.shape)


def maze(dx=37, dy=21, dz=5):
    """A serpentine maze of EMPTY corridors: a wall on every other row and every other slab, each with one gap, at alternating
    ends, so that the only way from voxel 0 to the far end runs the length of every open row of every open slab."""
    g = np.zeros((dz, dy, dx), np.uint8)
    for y in range(1, dy, 2):
        g[:, y, :] = 1
        g[:, y, dx - 1 if (y // 2) % 2 == 0 else 0] = 0
    rows = (dy + 1) // 2                                   # open rows per slab
    far = (dy - 1 if dy % 2 else dy - 2, 0 if rows % 2 == 0 else dx - 1)       # the far end of the last row the snake from (y 0, x 0) walks
    for z in range(1, dz, 2):
        g[z] = 1
        y, x = far if (z // 2) % 2 == 0 else (0, 0)
        g[z, y, x] = 0
    return g
