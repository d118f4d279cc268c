"""Deep octree scenes (depth 11 to 21) for the tests: a numpy statement of the pyramid builder, and scene factories.

The builder works from the solid voxels alone, so a scene may span a grid of 2^20 voxels per side without storing it:
a cell of the occupancy pyramid is EMPTY when it holds no solid voxel, FILLED when every one of its 2^(3l) voxels lies
inside the grid and is solid, and mixed otherwise (voxels outside the grid count as EMPTY).  A node is a leaf (isLeaf =
isUniform = 1, isSolid for FILLED) when its cell is not mixed or has size 1; the flat array lists the tree breadth first,
the 8 children of every internal node at consecutive indices in child order (bit 0 = +x, bit 1 = +y, bit 2 = +z).

Scenes:
  * "spine": a virtual grid of 2^d voxels per side holding a few small balls, two cell-aligned solid blocks and a ball at
    the far corner whose corner voxel is carved out, so the corner's cells are mixed down to size 2.  A ray that meets that
    cell descends through child 7 at every level and holds 7 d + 1 stack entries there: 134 at d = 19, 141 at d = 20.
  * "thin": a dense grid of 3 * 2^(d-2) x 3 x 2 voxels with small blobs along x: depth d, a few MB, for the builders.
  * "bar": a grid of X x c x c voxels, X = 3 * 2^(d-2), c = 16 up to depth 16 and 4 from depth 17 on (at most 12.6 M voxels),
    that holds four cell-aligned solid c-cubes over its whole cross-section, at x = 0, N/2 - c, N/2 + 2c and X - c (N = 2^d),
    and six single voxels one empty voxel away from their -x and +x faces, so that the cells next to the cubes are mixed down to
    size 1.
    The cubes are leaves of size c: the only deep scenes where a ray ends inside a solid leaf larger than 2 voxels, at x up
    to 2^20.  The tree is built from the solid coordinates; the dense array `data` is made when first asked for.  Two
    cameras, each orbiting one cube (the second, which has grid on both sides along x, and the last, whose +x face is the
    grid's) at 2.5 c voxels.
Grid kinds: "frac" (origin -0.5, voxel 2^-d: every node plane exact), "far" (voxel 1, origin of sceneCache.bin: exact,
planes up to 2^20 from the origin), "tenth" (voxel 0.1, origin 0.3: the general child test).
"""
from __future__ import annotations

import numpy as np

NODE_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("size", "<i4"), ("isLeaf", "<i4"), ("isSolid", "<i4"),
                       ("isUniform", "<i4"), ("child", "<i4", (8,))])
DEPTHS = (11, 12, 16, 17, 18, 19, 20)
KINDS = ("frac", "far", "tenth")
STACK_CAP = 7 * 20 + 1
_OFF = np.array([[k & 1, (k >> 1) & 1, k >> 2] for k in range(8)], np.int64)


def _key(c):
    return c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)


def build_octree(solid, dims, cubes=()):
    """solid: (N, 3) int voxel coordinates (x, y, z), unique, inside dims = (nx, ny, nz); cubes: further solid cubes
    (x, y, z, edge) that are cells of the pyramid (edge a power of 2 dividing x, y, z), apart from `solid`.  Returns the
    flat array."""
    solid = np.asarray(solid, np.int64).reshape(-1, 3)
    dims = np.asarray(dims, np.int64)
    depth = int(np.ceil(np.log2(dims.max()))) if dims.max() > 1 else 0
    out = []
    cells = np.zeros((1, 3), np.int64)
    base = 0                                            # index of the first node of the current tree level
    for L in range(depth + 1):
        lv = depth - L
        keys, counts = np.unique(_key(solid >> lv), return_counts=True)
        k = _key(cells)
        pos = np.minimum(np.searchsorted(keys, k), max(len(keys) - 1, 0))
        cnt = np.where((len(keys) > 0) & (keys[pos] == k), counts[pos], 0) if len(keys) else np.zeros(len(cells), np.int64)
        full = 1 << (3 * lv)
        lo, hi = cells << lv, (cells + 1) << lv
        for x, y, z, e in cubes:
            c0 = np.array([x, y, z]); c1 = c0 + e
            inside = ((lo >= c0) & (hi <= c1)).all(1)
            cnt = np.where(inside, full, cnt + np.where(((lo <= c0) & (c1 <= hi)).all(1), e ** 3, 0))
        mixed = (cnt > 0) & (cnt < full) & (lv > 0)
        nd = np.zeros(len(cells), NODE_DTYPE)
        nd["x"], nd["y"], nd["z"] = (cells << lv).T
        nd["size"] = 1 << lv
        nd["isLeaf"] = nd["isUniform"] = ~mixed
        nd["isSolid"] = ~mixed & (cnt == full)
        nd["child"] = -1
        m = np.nonzero(mixed)[0]
        first = base + len(cells) + 8 * np.arange(len(m))
        nd["child"][m] = first[:, None] + np.arange(8)
        out.append(nd)
        base += len(cells)
        if not len(m):
            break
        cells = (2 * cells[m][:, None, :] + _OFF).reshape(-1, 3)
    return np.concatenate(out)


def _ball(centre, r):
    c = np.asarray(centre, np.float64)
    lo = np.floor(c - r).astype(np.int64)
    g = np.stack(np.meshgrid(*[np.arange(lo[a], lo[a] + int(2 * r) + 2) for a in range(3)], indexing="ij"), -1).reshape(-1, 3)
    return g[(((g + 0.5) - c) ** 2).sum(1) <= r * r]


def _block(corner, size):
    g = np.stack(np.meshgrid(*[np.arange(size)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return np.asarray(corner, np.int64) + g


def bar_edge(d):
    """The edge c of a bar scene's cubes and cross-section."""
    return 16 if d <= 16 else 4


def bar_solid(d):
    """(solid voxels (n, 3), the four cubes' low corners, c) of the bar geometry at depth d."""
    N, c = 1 << d, bar_edge(d)
    X = 3 * N // 4
    xs = (0, N // 2 - c, N // 2 + 2 * c, X - c)
    singles = np.array([[c + 1, 1, 1], [N // 2 + 1, 1, 2], [N // 2 - c - 2, 2, 1], [N // 2 + 2 * c - 2, 2, 2], [N // 2 + 3 * c + 1, 0, 3],
                        [X - c - 2, 1, 1]], np.int64)
    return np.concatenate([_block((x, 0, 0), c) for x in xs] + [singles]), xs, c


_bar_data = {}


def grid_frame(kind, d):
    """(grid_min float32[3], voxel float32) of a grid kind at depth d."""
    if kind == "frac":
        return np.full(3, -0.5, np.float32), np.float32(2.0 ** -d)
    if kind == "far":
        return np.array([-2125.0, -1215.0, -150.0], np.float32), np.float32(1.0)
    if kind == "tenth":
        return np.full(3, 0.3, np.float32), np.float32(0.1)
    raise KeyError(kind)


class DeepScene:
    def __init__(self, kind, d, geometry="spine"):
        self.kind, self.depth, self.geometry = kind, d, geometry
        self.min, self.voxel = grid_frame(kind, d)
        self._data = None
        N = 1 << d
        if geometry == "spine":
            self.dims = (N, N, N)
            self.data = None
            corner = _ball((N - 2.0, N - 2.0, N - 2.0), 2.6)
            corner = corner[(corner < N).all(1) & ~(corner == N - 1).all(1)]       # the corner voxel stays empty
            balls = [_ball((f * N + 0.3, f * N + 0.7, (1 - f) * N + 0.2), 2.2) for f in (0.3, 0.61, 0.875)]
            blocks = _block((0, 0, 0), 16), _block((N - 32, 0, N // 2), 8)
            self.blobs = [corner] + balls
            solid = np.unique(np.concatenate([corner] + balls), axis=0)
            big = ((N // 4, 0, 0, N // 4), (N // 2, N // 2, 0, N // 8))    # cell-aligned solid cubes (x, y, z, edge)
            self.nodes = build_octree(np.unique(np.concatenate([solid] + list(blocks)), axis=0), self.dims, big)
        elif geometry == "bar":
            solid, xs, c = bar_solid(d)
            self.dims = (3 * N // 4, c, c)
            self.edge, self.blocks = c, xs
            self.blobs = [np.array([[x + (c - 1) / 2, (c - 1) / 2, (c - 1) / 2]]) for x in xs]       # + 0.5: the cubes' centres
            self.nodes = build_octree(solid, self.dims)
        elif geometry == "thin":
            self.dims = (3 * N // 4, 3, 2)
            data = np.zeros(self.dims[::-1], np.uint8)                                 # (z, y, x)
            xs = [3, N // 2 - 1, N // 2 + 5, 3 * N // 4 - 2]
            for x in xs:
                data[:, :, x - 2:x + 1] = 1
                data[1, 1, x] = 0
            data[0, 2, xs[1] + 7] = 1
            self.data = data
            z, y, x = np.nonzero(data)
            self.blobs = [np.array([[x0, 1, 1]]) for x0 in xs]
            self.nodes = build_octree(np.stack([x, y, z], 1), self.dims)
        else:
            raise KeyError(geometry)

    @property
    def data(self):
        """The dense (z, y, x) uint8 array; a bar scene's is made on first use and shared by the grid kinds of a depth."""
        if self._data is None and self.geometry == "bar":
            if self.depth not in _bar_data:
                data = np.zeros(self.dims[::-1], np.uint8)
                solid = bar_solid(self.depth)[0]
                data[solid[:, 2], solid[:, 1], solid[:, 0]] = 1
                _bar_data[self.depth] = data
            return _bar_data[self.depth]
        return self._data

    @data.setter
    def data(self, value):
        self._data = value

    def world(self, p):
        return self.min.astype(np.float64) + np.asarray(p, np.float64) * float(self.voxel)

    def cameras(self, orc):
        """(name, view, pos) triples: 9 voxels from the first blob (the corner one of a spine scene), 16 from the second (rays
        reach level d in both), and one far away that sees the whole root box.  A bar scene: "block1" and "block3", each 2.5 c
        voxels from the centre of one cube."""
        N = 1 << self.depth
        out = []
        if self.geometry == "bar":
            for i in (1, 3):
                cam = orc.Camera(0.7, 0.5, float(np.float32(2.5 * self.edge * float(self.voxel))))
                cam.set_target(*[float(v) for v in self.world(self.blobs[i][0] + 0.5).astype(np.float32)])
                out.append((f"block{i}", cam.get_view(), cam.get_pos()))
            return out
        for i, (th, ph, r) in enumerate(((0.7, 0.5, 9.0), (2.4, -0.35, 16.0))):
            centre = self.blobs[i].mean(0) + 0.5
            cam = orc.Camera(th, ph, float(np.float32(r * float(self.voxel))))
            cam.set_target(*[float(v) for v in self.world(centre).astype(np.float32)])
            out.append((f"near{i}", cam.get_view(), cam.get_pos()))
        ext = N * float(self.voxel)
        cam = orc.Camera(0.45, 0.35, float(np.float32(1.7 * ext)))
        cam.set_target(*[float(v) for v in self.world(np.array(self.dims) / 2).astype(np.float32)])
        out.append(("far", cam.get_view(), cam.get_pos()))
        return out


_cache = {}


def scene(kind, d, geometry="spine"):
    key = (kind, d, geometry)
    if key not in _cache:
        _cache[key] = DeepScene(kind, d, geometry)
    return _cache[key]


def stack_need(nodes):
    """Stack entries a LIFO walk may hold when every box passes: 1 at a leaf, else max over the pushed children c of
    (children pushed before c) + need(c).  (Children always follow their parent in a breadth-first array.)"""
    n = len(nodes)
    need = np.ones(n, np.int64)
    ch = nodes["child"]
    for i in range(n - 1, -1, -1):
        if nodes["isLeaf"][i] == 1 or nodes["isUniform"][i] == 1:
            continue
        c = ch[i][ch[i] >= 0]
        need[i] = max(1, int((np.arange(len(c)) + need[c]).max()) if len(c) else 1)
    return int(need[0])
