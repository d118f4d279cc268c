"""Seeded mesh families for rto_voxelize_mesh at the sizes and edges where its kernels branch.  Every
generator returns a Case: rows (float64 [n, 3]), faces (int32 [m, 3]), the voxel size asked for, and grid = None (AUTO) or the
FIXED (dims (x, y, z), grid_min float32[3], voxel_size float32).

- many_small: 600 k faces of a few voxels each, so k_scan_counts carries between three rounds of 1024 block sums, with long
  runs of faces that have no voxels (outside the grid, degenerate, a NaN row) at the start, the end and inside the list.
- boundaries: faces whose pair spans start and end exactly on multiples of 16 (one k_vox_fill thread's run) and 4096 (one
  block), single-voxel faces, faces of 4095 / 4096 / 4097 pairs and empty faces on those boundaries.
- below_low: faces whose box is clipped at the low side of a FIXED grid (t_max in (-2, 0), t_min in (-1, 0): the truncating
  cast gives them voxel 0 and voxel 1), faces far below, faces straddling the high side and faces above it.
- huge_face: one triangle across a FIXED grid of more than 2^31 voxels, so the pairs of one face and the flat voxel index both
  pass 2^31; huge_refused repeats it 4096 times, so the pairs pass 2^43 and the call is refused.
- auto_edges: AUTO meshes whose extent gives a dim of 1000, 1001, 1999, 2000 or 2001 before the MAX_DIM rescale.
- fixed_limit: FIXED (2^20 + extra, 1, 1) with a few faces along x.
- empty_*: FIXED with no face, FIXED with every face outside, every face degenerate (FIXED and AUTO)."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

f32 = np.float32


class Case(NamedTuple):
    xyz: np.ndarray
    tris: np.ndarray
    voxel: np.float32
    grid: Optional[tuple]


def _fixed(dims, gmin, vs):
    return tuple(int(d) for d in dims), np.asarray(gmin, np.float32), f32(vs)


def _pack(tri_xyz, extra_rows=None, voxel=1.0, grid=None):
    """Faces given as vertices [m, 3, 3] -> rows and faces (three rows per face), extra rows appended unused."""
    tri_xyz = np.asarray(tri_xyz, np.float64).reshape(-1, 3, 3)
    xyz = tri_xyz.reshape(-1, 3)
    if extra_rows is not None:
        xyz = np.concatenate([xyz, np.asarray(extra_rows, np.float64).reshape(-1, 3)])
    tris = np.arange(3 * len(tri_xyz), dtype=np.int32).reshape(-1, 3)
    return Case(xyz, tris, f32(voxel), grid)


def _box_face(rng, lo, hi):
    """A triangle whose bounding box is exactly [lo, hi] per axis (one vertex takes each bound, the third lies between)."""
    v = np.empty((3, 3))
    for a in range(3):
        k = rng.permutation(3)
        v[k[0], a], v[k[1], a] = lo[a], hi[a]
        v[k[2], a] = rng.uniform(lo[a], hi[a])
    return v


def _span(rng, n, s, dim, gmin, vs):
    """World interval on one axis whose voxel box (s = max(0, (int)t_min), e = min(dim - 1, (int)t_max + 1)) is [s, s + n - 1].
    n = 1 only at the high side (s = dim - 1, clipped)."""
    if n == 1:
        assert s == dim - 1
        t0, t1 = s + rng.uniform(0.1, 0.4), s + rng.uniform(0.6, 2.5)
    else:
        t0, t1 = s + rng.uniform(0.1, 0.9), s + n - 2 + rng.uniform(0.1, 0.9)
    t0, t1 = min(t0, t1), max(t0, t1)
    return gmin + t0 * vs, gmin + t1 * vs


def _no_voxel_faces(rng, count, dims, gmin, vs):
    """Faces with no voxels on a FIXED grid: outside it (above the high side), degenerate (collinear or repeated vertices), or
    with a NaN coordinate.  Vertices [count, 3, 3]."""
    hi = np.asarray(gmin, np.float64) + np.asarray(dims, np.float64) * vs
    out = np.empty((count, 3, 3))
    kind = rng.integers(0, 4, count)
    for i, k in enumerate(kind):
        if k == 0:                                          # entirely above the grid on one axis
            a = rng.integers(0, 3)
            lo = np.asarray(gmin, np.float64) + rng.uniform(0, 1, 3) * (hi - np.asarray(gmin)) * 0.9
            lo[a] = hi[a] + rng.uniform(0.5, 40.0) * vs
            out[i] = _box_face(rng, lo, lo + rng.uniform(0.2, 3.0, 3) * vs)
        elif k == 1:                                        # collinear, exactly (quarter-voxel coordinates): denom is 0
            p = np.asarray(gmin) + np.floor(rng.uniform(0, 1, 3) * np.asarray(dims) * 4) * (vs / 4)
            d = rng.integers(-6, 7, 3) * (vs / 4)
            out[i] = [p, p + d, p + 2 * d]
        elif k == 2:                                        # a repeated vertex
            p = np.asarray(gmin) + rng.uniform(0, 1, 3) * (hi - np.asarray(gmin))
            q = p + rng.normal(size=3) * vs
            out[i] = [p, q, p]
        else:                                               # a NaN coordinate
            out[i] = _box_face(rng, np.asarray(gmin) + 1.5 * vs, np.asarray(gmin) + 3.5 * vs)
            out[i, rng.integers(0, 3), rng.integers(0, 3)] = np.nan
    return out


# ---------------------------------------------------------------- many small faces
def many_small(n_faces=600_000, seed=1):
    rng = np.random.default_rng(seed)
    dims, gmin, vs = (200, 160, 48), np.array([-10.25, 30.5, 7.75]), 0.5
    extent = np.asarray(dims) * vs
    # runs of faces without voxels: at the start, at the end, and inside (some longer than a setup block of 256)
    kinds = np.ones(n_faces, bool)
    kinds[:5000] = False
    kinds[-5000:] = False
    for _ in range(60):
        at, ln = int(rng.integers(0, n_faces)), int(rng.integers(1, 4000))
        kinds[at:at + ln] = False
    empty = _no_voxel_faces(rng, int((~kinds).sum()), dims, gmin, vs)
    m = int(kinds.sum())
    c = gmin + rng.uniform(0.02, 0.98, (m, 3)) * extent
    small = c[:, None, :] + rng.normal(scale=0.6 * vs, size=(m, 3, 3))
    v = np.empty((n_faces, 3, 3))
    v[kinds], v[~kinds] = small, empty
    return _pack(v, voxel=vs, grid=_fixed(dims, gmin, vs))


# ---------------------------------------------------------------- faces placed on the fill's run and block boundaries
BOUNDARY_DIMS = (512, 512, 8)


def _factor(c, dims=BOUNDARY_DIMS):
    """(nx, ny, nz) with nx ny nz = c within dims, or None."""
    for nz in range(1, dims[2] + 1):
        if c % nz:
            continue
        r = c // nz
        for nx in range(min(r, dims[0]), 0, -1):
            if r % nx == 0 and r // nx <= dims[1]:
                return nx, r // nx, nz
    return None


def _counts(c):
    """c pairs as faces that each factor within the grid."""
    out = []
    while c > 0:
        k = c
        while _factor(k) is None:
            k -= 1
        out.append(k)
        c -= k
    return out


def boundary_counts(seed=2):
    """The pair count of every face (0: no voxels), in list order."""
    rng = np.random.default_rng(seed)
    seq = [0, 0, 0] + [1] * 16 + [0]                                    # empty faces at offset 0; 16 single voxels end a run
    total = lambda: sum(seq)                                            # noqa: E731

    def pad(m):
        seq.extend(_counts(-total() % m))

    for rep in range(6):
        pad(4096)
        seq += [4096, 0, 0, 4095, 1, 4097]                                # a whole block; 4095 + 1 ends one; 4097 crosses one
        pad(16)
        seq += [0] * int(rng.integers(1, 300)) + [16, 32, 48, 0, 16 * 255, 1, 15]   # runs of 16; an empty run of faces
        pad(4096)
        seq += [0, 4096 * 3 + 8, 0, 4089, 4096 - 7, 7]                    # a face over three blocks and more
        seq += [int(x) for x in rng.integers(1, 60, int(rng.integers(50, 400)))]   # ragged small faces
        seq += [0] * 257 + [1] * 33 + [4096] + [0] * 1024                  # whole setup blocks (256 faces) without a pair
        seq += [4095] * 3 + [4097] * 3
    pad(4096)
    seq += [0] * 7
    return [c if c == 0 or _factor(c) else None for c in seq]


def boundaries(seed=2):
    rng = np.random.default_rng(seed)
    dims, gmin, vs = BOUNDARY_DIMS, np.array([3.0, -2.0, 0.5]), 0.25
    counts = boundary_counts(seed)
    assert None not in counts
    v = np.empty((len(counts), 3, 3))
    empty = _no_voxel_faces(rng, counts.count(0), dims, gmin, vs)
    k = 0
    for i, c in enumerate(counts):
        if c == 0:
            v[i] = empty[k]
            k += 1
            continue
        n = _factor(c)
        lo, hi = np.empty(3), np.empty(3)
        for a in range(3):
            s = dims[a] - 1 if n[a] == 1 else int(rng.integers(0, dims[a] - n[a] + 1))
            lo[a], hi[a] = _span(rng, n[a], s, dims[a], gmin[a], vs)
        v[i] = _box_face(rng, lo, hi)
    return _pack(v, voxel=vs, grid=_fixed(dims, gmin, vs))


# ---------------------------------------------------------------- boxes clipped at the grid's sides
def _clip_span(rng, kind, dim):
    """(t_min, t_max) in voxel units for one axis: 0 inside, 1 t_min in (-1, 0), 2 t_min, t_max in (-2, 0), 3 t_max < -2
    (no voxel), 4 across the high side, 5 above the high side (no voxel)."""
    if kind == 0:
        t0 = rng.uniform(0.05, dim - 3.0)
        return t0, t0 + rng.uniform(0.3, 2.5)
    if kind == 1:
        return rng.uniform(-0.95, -0.05), rng.uniform(0.1, 3.0)
    if kind == 2:
        t1 = rng.uniform(-1.95, -0.05)
        return t1 - rng.uniform(0.0, 3.0), t1
    if kind == 3:
        t1 = rng.uniform(-6.0, -2.05)
        return t1 - rng.uniform(0.0, 2.0), t1
    if kind == 4:
        return dim - rng.uniform(0.2, 2.5), dim + rng.uniform(0.1, 3.0)
    t0 = dim + rng.uniform(0.05, 3.0)
    return t0, t0 + rng.uniform(0.2, 2.0)


def below_low(n_faces=4000, seed=3):
    """Every face has at least one axis clipped at the low side (kinds 1-3) or the high side (4, 5); the others lie inside."""
    rng = np.random.default_rng(seed)
    dims, gmin, vs = (40, 36, 32), np.array([-3.25, 1.5, 100.0]), 0.5
    v = np.empty((n_faces, 3, 3))
    for i in range(n_faces):
        kinds = [0, 0, 0]
        for a in rng.choice(3, int(rng.integers(1, 4)), replace=False):
            kinds[a] = int(rng.choice([1, 2, 2, 2, 3, 4, 5]))
        lo, hi = np.empty(3), np.empty(3)
        for a in range(3):
            t0, t1 = _clip_span(rng, kinds[a], dims[a])
            lo[a], hi[a] = gmin[a] + t0 * vs, gmin[a] + t1 * vs
        v[i] = _box_face(rng, lo, hi)
    return _pack(v, voxel=vs, grid=_fixed(dims, gmin, vs))


# ---------------------------------------------------------------- more than 2^31 voxels and pairs
HUGE_DIMS = (2048, 1024, 1025)          # 2^31 + 2^21 voxels; one face's box covers all of them


def _huge_tri():
    return np.array([[0.25, 0.5, 0.75], [2047.75, 1023.5, 700.25], [900.5, 1023.75, 1024.5]])


def huge_face():
    return _pack(_huge_tri()[None], voxel=1.0, grid=_fixed(HUGE_DIMS, (0.0, 0.0, 0.0), 1.0))


def huge_refused(copies=4096):
    """copies x (2^31 + 2^21) pairs: above the 2^31 blocks of 4096 pairs one fill launch takes."""
    return _pack(np.repeat(_huge_tri()[None], copies, 0), voxel=1.0, grid=_fixed(HUGE_DIMS, (0.0, 0.0, 0.0), 1.0))


# ---------------------------------------------------------------- AUTO grids at the MAX_DIM rescale's edges
AUTO_EDGE_DIMS = (1000, 1001, 1999, 2000, 2001)


def auto_edges(dim, seed=4, axis=0):
    """An AUTO mesh at voxel 1 whose extent on `axis` gives `dim` before the rescale (the padded extent is dim - 0.5 voxels), with
    random faces inside, degenerate faces, faces on NaN rows and unused NaN rows."""
    rng = np.random.default_rng(seed + dim)
    L = dim - 2.5                                                      # + 2 voxels of padding: ceil(dim - 0.5) = dim
    size = np.array([7.0, 5.0, 3.0])
    size[axis] = L
    base = np.array([701000.0, 5660500.0, 1040.0]) if dim % 2 else np.zeros(3)
    corners = base + np.array([[0, 0, 0], size])                       # two vertices set the bounds
    faces = [[corners[0], corners[0] + size * [1, 0.5, 0.25], corners[1]]]
    for _ in range(150):
        c = base + rng.uniform(0, 1, 3) * size
        faces.append(c + rng.normal(scale=[2.0, 1.0, 0.7], size=(3, 3)).clip(-c + base, base + size - c))
    for _ in range(10):                                                # degenerate
        p = base + rng.uniform(0, 1, 3) * (size - 1.0)
        faces.append([p, p, p + rng.uniform(0, 1, 3)])
    for _ in range(8):                                                 # a NaN vertex
        f = base + rng.uniform(0, 1, (3, 3)) * size
        f[rng.integers(0, 3), rng.integers(0, 3)] = np.nan
        faces.append(f)
    return _pack(np.asarray(faces), extra_rows=[[np.nan, 1.0, 2.0], [3.0, np.nan, np.nan]], voxel=1.0)


# ---------------------------------------------------------------- the FIXED per-axis limit
def fixed_limit(extra=0):
    """FIXED (2^20 + extra, 1, 1): faces across the row of voxels (they reach far out in y, so they are well conditioned), one of
    them the whole length."""
    nx = (1 << 20) + extra
    v = np.array([[[0.25, -1.0e6, 0.5], [nx - 0.25, 0.25, 0.45], [0.25, 1.0e6, 0.55]],
                  [[10.5, -40.0, 0.0], [300.5, 40.0, 0.0], [10.5, 0.0, 1.0]],
                  [[nx - 900.5, -2.0, 0.6], [nx - 1.5, 3.0, 0.1], [nx - 10.5, 0.8, 0.9]]])
    return _pack(v, voxel=1.0, grid=_fixed((nx, 1, 1), (0.0, 0.0, 0.0), 1.0))


# ---------------------------------------------------------------- nothing to fill
def empty_no_faces():
    return Case(np.zeros((3, 3)), np.zeros((0, 3), np.int32), f32(0.5), _fixed((24, 20, 16), (1.0, 2.0, 3.0), 0.5))


def empty_all_outside(seed=5):
    rng = np.random.default_rng(seed)
    dims, gmin, vs = (24, 20, 16), np.array([1.0, 2.0, 3.0]), 0.5
    v = np.empty((700, 3, 3))
    for i in range(len(v)):
        kinds = [0, 0, 0]
        kinds[int(rng.integers(0, 3))] = int(rng.choice([3, 5]))
        lo, hi = np.empty(3), np.empty(3)
        for a in range(3):
            t0, t1 = _clip_span(rng, kinds[a], dims[a])
            lo[a], hi[a] = gmin[a] + t0 * vs, gmin[a] + t1 * vs
        v[i] = _box_face(rng, lo, hi)
    return _pack(v, voxel=vs, grid=_fixed(dims, gmin, vs))


def empty_all_degenerate(seed=6, auto=False):
    rng = np.random.default_rng(seed)
    dims, gmin, vs = (24, 20, 16), np.array([1.0, 2.0, 3.0]), 0.5
    p = gmin + np.floor(rng.uniform(0, 1, (600, 3)) * np.asarray(dims) * 4) * (vs / 4)
    d = rng.integers(-6, 7, (600, 3)) * (vs / 4)
    v = np.stack([p, p + d, p + 3.0 * d], 1)                           # collinear on quarter-voxel coordinates: denom is 0
    v[::3, 2] = v[::3, 0]                                              # repeated vertex
    return _pack(v, voxel=vs, grid=None if auto else _fixed(dims, gmin, vs))


EMPTY = {"no_faces": empty_no_faces, "all_outside": empty_all_outside, "all_degenerate": empty_all_degenerate,
         "all_degenerate_auto": lambda: empty_all_degenerate(auto=True)}
