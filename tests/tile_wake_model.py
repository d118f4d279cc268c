"""Sequential models of the two work-list protocols (k_geo_seeds / k_geo_relax of csrc/rto_geodesic.inc, DESIGN.md section 20;
k_skel_mark / k_skel_step of csrc/rto_skeleton.inc, section 23), and the directed grids of tests/test_tile_wake.py.

A model runs one launch after another and, within a launch, one workgroup (one 32 x 8 x 8 tile) after another; every tile of a
launch reads the state of the launch's start.  What a tile does is the kernel's text in numpy: copy the tile with its one-voxel
halo, work on the copy, write back what changed, and tell the neighbour tiles by the face position of each changed voxel.  With
omit=None a model is the protocol as built and equals the rule (geodesic_ref.field, skeleton_ref.skeleton).  Each omission leaves
one notification out:
    geodesic  "face_marks"        a lowering tile marks its 6 face neighbours only, never an edge or corner tile
              "seed_own_tile"     k_geo_seeds marks the seed's own tile only
    skeleton  "face_stamps"       a removal raises the stamps of its own tile and its 6 face neighbours only
              "sleep_below_pass"  a tile sleeps in pass P when its stamp is below P (instead of P - 1); the stamps then start at 1,
                                  so that pass 1 still runs everywhere
No GPU is involved: the models show which grids can tell a kernel with such an omission from the rule.  `python
tests/tile_wake_model.py` prints, for the grids of test_geodesic.py and test_skeleton.py, which of them do."""
from __future__ import annotations

import numpy as np

import geodesic_ref as gr
import skeleton_ref as sr

TILE = (32, 8, 8)                                          # x, y, z
SIZES = ((96, 24, 24), (70, 22, 22))                       # dimX, dimY, dimZ: 3 x 3 x 3 tiles, whole ones and ragged last ones
T0 = (32, 8, 8)                                            # the origin of the centre tile T
DIRECTIONS = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
GEO_OMISSIONS = ("face_marks", "seed_own_tile")
SKEL_OMISSIONS = ("face_stamps", "sleep_below_pass")


# ================================================================ what both kernels share
def tile_counts(shape):
    """(tilesZ, tilesY, tilesX) of a grid of shape (dimZ, dimY, dimX)."""
    return tuple(-(-n // t) for n, t in zip(shape, TILE[::-1]))


def _box(tile, shape, halo):
    """The slices of tile (tz, ty, tx): in the grid padded by one voxel and with the tile's halo, or in the grid itself."""
    return tuple(slice(t * n, min(t * n + n, d) + 2 * halo) for t, n, d in zip(tile, TILE[::-1], shape))


def told(tile, counts, lz, ly, lx, diagonal, own):
    """The tiles that hear of a change of the voxels (lz, ly, lx), local to `tile`: "the neighbours at offset -1 / +1 along an axis
    lie in the tile before / after when the voxel is on that face".  diagonal=False keeps the 6 face neighbours only."""
    out = set()
    side = [np.where(l == 0, -1, np.where(l == n - 1, 1, 0)).tolist() for l, n in zip((lz, ly, lx), TILE[::-1])]
    for e in set(zip(*side)):
        for a in np.ndindex(2, 2, 2):
            m = tuple(ai * ei for ai, ei in zip(a, e))
            changed = sum(v != 0 for v in m)
            if (changed == 0 and not own) or (changed > 1 and not diagonal):
                continue
            t = tuple(ti + mi for ti, mi in zip(tile, m))
            if all(0 <= ti < n for ti, n in zip(t, counts)):
                out.add(t)
    return out


# ================================================================ geodesic: k_geo_seeds, then launches of k_geo_relax
def geodesic_model(grid, seeds, medium=gr.SET_EMPTY, connectivity=gr.CONN_FACE, limit=None, omit=None):
    """(the field, launches with the closing one that finds no tile marked, tiles run)."""
    assert omit in (None, *GEO_OMISSIONS)
    grid = np.asarray(grid)
    dz, dy, dx = grid.shape
    counts = tile_counts(grid.shape)
    reach = gr.NONE - 1 if limit is None or limit >= gr.NO_LIMIT else int(limit)
    inside = np.pad(grid == medium, 1)
    g = np.full(inside.shape, gr.NONE, np.int64)           # padded by one voxel: NONE beyond the grid
    cur = np.zeros(counts, bool)
    for v in gr.check_seeds(grid, seeds).tolist():         # k_geo_seeds
        x, y, z = v % dx, (v // dx) % dy, v // (dx * dy)
        for mz, my, mx in ([(0, 0, 0)] if omit == "seed_own_tile" else [(0, 0, 0), *[d[::-1] for d in DIRECTIONS]]):
            nx, ny, nz = x + mx, y + my, z + mz
            if 0 <= nx < dx and 0 <= ny < dy and 0 <= nz < dz:
                cur[nz // TILE[2], ny // TILE[1], nx // TILE[0]] = True
        if inside[z + 1, y + 1, x + 1]:
            g[z + 1, y + 1, x + 1] = 0
    mv = gr.moves(connectivity)
    weight = np.asarray([w for _, _, _, w in mv])
    diagonal = connectivity == gr.CONN_FULL and omit != "face_marks"
    launches = tiles_run = 0
    while True:
        launches += 1
        if not cur.any():
            return np.ascontiguousarray(g[1:-1, 1:-1, 1:-1], np.int32), launches, tiles_run
        start, nxt = g.copy(), np.zeros(counts, bool)
        for tile in map(tuple, np.argwhere(cur).tolist()):
            tiles_run += 1
            box = _box(tile, grid.shape, 1)
            G = start[box].copy()                          # the tile's values with a one-voxel halo
            own = np.zeros(G.shape, bool)
            own[1:-1, 1:-1, 1:-1] = inside[box][1:-1, 1:-1, 1:-1]
            at = np.flatnonzero(own)                       # the tile's voxels of the medium: the only ones that change
            off = np.asarray([(mz * G.shape[1] + my) * G.shape[2] + mx for mz, my, mx, _ in mv])
            flat = G.reshape(-1)
            while at.size:                                 # sweeps until one lowers nothing
                best = (flat[at[:, None] + off] + weight).min(axis=1)
                low = (best < flat[at]) & (best <= reach)
                if not low.any():
                    break
                flat[at[low]] = best[low]
            lowered = G < start[box]
            g[box][lowered] = G[lowered]
            lz, ly, lx = np.nonzero(lowered[1:-1, 1:-1, 1:-1])
            for t in told(tile, counts, lz, ly, lx, diagonal, own=False):
                nxt[t] = True
        cur = nxt


# ================================================================ skeleton: per pass k_skel_mark, then 8 launches of k_skel_step
def skeleton_model(grid, which=sr.SET_SOLID, connectivity=sr.CONN_FULL, mode=sr.SKEL_TOPOLOGY, anchors=(), max_passes=sr.NO_LIMIT, omit=None):
    """(k, the summary record, tiles run).  The 27-bit blocks are read from the launch's start by skeleton_ref.masks_at, which is the
    tile's halo copy taken voxel by voxel, and judged by skeleton_ref.simple: the model is of the stamps, not of the simple test."""
    assert omit in (None, *SKEL_OMISSIONS)
    a = sr.check_args(grid, which, connectivity, mode, anchors, max_passes)
    counts = tile_counts(grid.shape)
    x = grid == (1 if which == sr.SET_SOLID else 0)
    k = np.where(x, 0, -1).astype(np.int32)
    anchor = np.zeros(grid.shape, bool)
    anchor.reshape(-1)[a] = True
    zz, yy, xx = np.indices(grid.shape, sparse=True)
    sub = (xx & 1) + 2 * (yy & 1) + 4 * (zz & 1)
    late = omit == "sleep_below_pass"
    stamp = np.full(counts, 1 if late else 0)
    p = tiles_run = 0
    while p < max_passes:
        p += 1
        marked = sr.marked(x, connectivity) & ~anchor      # k_skel_mark: every word, from the X of the pass's start
        gone = False
        for s in range(8):
            start, seen = x.copy(), stamp.copy()
            for tile in map(tuple, np.argwhere(seen >= (p if late else p - 1)).tolist()):
                tiles_run += 1
                box = _box(tile, grid.shape, 0)
                lz, ly, lx = np.nonzero(marked[box] & (sub[box] == s))
                if not lz.size:
                    continue
                idx = (lz + box[0].start, ly + box[1].start, lx + box[2].start)
                m = sr.masks_at(start, idx)
                go = sr.simple(m, connectivity)
                if mode == sr.SKEL_CURVE:
                    n = m & np.uint32(sr.N26)
                    go &= ~((n != 0) & ((n & (n - np.uint32(1))) == 0))
                if not go.any():
                    continue
                sel = tuple(i[go] for i in idx)
                x[sel] = False
                k[sel] = p
                gone = True
                for t in told(tile, counts, lz[go], ly[go], lx[go], omit != "face_stamps", own=True):
                    stamp[t] = p
        if not gone:
            p -= 1
            break
    summary = np.zeros((), sr.SUMMARY_DTYPE)
    summary["kept"], summary["removed"] = int((k == 0).sum()), int((k > 0).sum())
    summary["passes"] = int(k.max()) if (k > 0).any() else 0
    return k, summary, tiles_run


# ================================================================ the directed grids
def lin(dims, p):
    return int(p[0] + dims[0] * (p[1] + dims[1] * p[2]))


def tile_of(p):
    """(tz, ty, tx) of voxel (x, y, z)."""
    return (p[2] // TILE[2], p[1] // TILE[1], p[0] // TILE[0])


def _grid(dims, cells):
    g = np.zeros(dims[::-1], np.uint8)
    for x, y, z in cells:
        assert 0 <= x < dims[0] and 0 <= y < dims[1] and 0 <= z < dims[2], (dims, (x, y, z))
        g[z, y, x] = 1
    return g


def add(p, d, n=1):
    return tuple(pi + n * di for pi, di in zip(p, d))


def exit_voxel(delta):
    """c: the voxel of T on the face, edge or corner towards `delta`, in the middle along the axes where delta is 0."""
    return tuple(o + (0 if d < 0 else t - 1 if d > 0 else t // 2) for o, t, d in zip(T0, TILE, delta))


def _beyond(delta):
    """d = c + delta, in the neighbour tile T'(delta) and no other, and one more voxel along the first non-zero axis of delta."""
    d = add(exit_voxel(delta), delta)
    axis = next(i for i in range(3) if delta[i])
    return d, add(d, tuple(delta[i] if i == axis else 0 for i in range(3)))


def route_case(dims, delta):
    """(grid, seeds, c, d): the seed in the middle of T, a staircase along x, then y, then z to c, all inside T; d and one more."""
    c = exit_voxel(delta)
    at = tuple(o + t // 2 for o, t in zip(T0, TILE))
    cells = [at]
    for axis in range(3):
        while at[axis] != c[axis]:
            at = tuple(v + (1 if c[i] > v else -1) * (i == axis) for i, v in enumerate(at))
            cells.append(at)
    assert at == c and all(tile_of(p) == (1, 1, 1) for p in cells)
    d, e = _beyond(delta)
    assert tile_of(d) == add((1, 1, 1), delta[::-1]) == tile_of(e)
    return _grid(dims, [*cells, d, e]), np.asarray([lin(dims, cells[0])], np.int64), c, d


def seed_case(dims, delta):
    """(grid, seeds, c, d): c, d and one more; the seed is c itself."""
    c = exit_voxel(delta)
    d, e = _beyond(delta)
    return _grid(dims, [c, d, e]), np.asarray([lin(dims, c)], np.int64), c, d


DETOURS = (("xy", (0, 1), (1, 1)), ("xy_mirrored", (0, 1), (-1, -1)), ("xz_mirrored", (0, 2), (1, -1)), ("yz_mirrored", (1, 2), (-1, 1)))


def detour_case(axes, signs):
    """(grid, seeds, target, the tile edge direction) on (96, 24, 24), in the plane through the middle of T that `axes` = (a, b)
    span.  A column in T with the seed on it; from its far end a row along T's last b-plane into the tile after T along a, and up
    that tile's first a-plane to the target: the long way, which arrives through T's +a face.  From the column's near end a row
    just outside T's first b-plane, in the tile before T along b, that ends diagonally next to the target: the short way, which
    arrives one launch later across the tile edge (+a, +b) of that tile.  signs = -1 mirrors an axis about the middle of T."""
    dims = SIZES[0]
    a, b = axes
    (a0, b0), (a1, b1) = (T0[a], T0[b]), (T0[a] + TILE[a] - 1, T0[b] + TILE[b] - 1)
    ac = a0 + TILE[a] // 4
    plane = [(ac, v) for v in range(b0, b1 + 1)] + [(u, b0 - 1) for u in range(ac + 1, a1 + 1)] + [(u, b1) for u in range(ac, a1 + 2)]
    plane += [(a1 + 1, v) for v in range(b0, b1 + 1)] + [(a1 + 2, b0), (a1 + 3, b0)]

    def place(u, v):
        p = [o + t // 2 for o, t in zip(T0, TILE)]
        p[a] = u if signs[0] > 0 else dims[a] - 1 - u
        p[b] = v if signs[1] > 0 else dims[b] - 1 - v
        return tuple(p)
    edge = [0, 0, 0]
    edge[a], edge[b] = signs
    seed, target = place(ac, b0 + TILE[b] // 2), place(a1 + 1, b0)
    return _grid(dims, [place(u, v) for u, v in plane]), np.asarray([lin(dims, seed)], np.int64), target, tuple(edge)


def line_case(dims, delta):
    """(grid, anchors, c): the line c + i delta, i = -7 .. 4: 8 voxels inside T, 4 in T'(delta); the anchor is its far end."""
    c = exit_voxel(delta)
    cells = [add(c, delta, i) for i in range(-7, 5)]
    assert all(tile_of(p) == (1, 1, 1) for p in cells[:8]) and all(tile_of(p) == add((1, 1, 1), delta[::-1]) for p in cells[8:])
    return _grid(dims, cells), [lin(dims, cells[-1])], c


# ================================================================ the survey of the suites' own grids
def survey(geodesic_grids=None, skeleton_grids=None):
    """Which grids of test_geodesic.GRIDS (both media, CONN_FULL) and of test_skeleton.GPU_GRIDS (SETS x MODES) tell a model with an
    omission from the rule: {omission: (the combinations that do, the number tried)}, printed as it is found."""
    import test_geodesic as tg
    import test_skeleton as ts
    geodesic_grids = tg.GRIDS if geodesic_grids is None else geodesic_grids
    skeleton_grids = ts.GPU_GRIDS if skeleton_grids is None else skeleton_grids
    out = {}
    for omit in GEO_OMISSIONS:
        caught = []
        for name in geodesic_grids:
            g, seeds = tg._named(name)
            for medium in tg.MEDIA:
                want = tg._ref(name, g, seeds, medium, gr.CONN_FULL)
                if not np.array_equal(geodesic_model(g, seeds, medium, gr.CONN_FULL, omit=omit)[0], want):
                    caught.append((name, medium))
        out[omit] = (caught, len(geodesic_grids) * len(tg.MEDIA))
        print(f"geodesic {omit}: caught on {len(caught)} of {out[omit][1]} (grid, medium) under CONN_FULL: {caught}", flush=True)
    for omit in SKEL_OMISSIONS:
        caught = []
        for name in skeleton_grids:
            g = ts._named(name)
            for which in ts.SETS:
                for conn, mode in ts.MODES:
                    if not np.array_equal(skeleton_model(g, which, conn, mode, omit=omit)[0], ts._ref(name, g, which, conn, mode)[0]):
                        caught.append((name, which, conn, mode))
        out[omit] = (caught, len(skeleton_grids) * len(ts.SETS) * len(ts.MODES))
        never = sorted({*skeleton_grids} - {c[0] for c in caught})
        print(f"skeleton {omit}: caught on {len(caught)} of {out[omit][1]} (grid, set, connectivity, mode); never on {never}", flush=True)
    return out


if __name__ == "__main__":
    survey()
