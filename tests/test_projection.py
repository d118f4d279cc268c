"""Field projections (rto_project_field_*, Context.project_field_*, RayTracerBVH::projectField): per pixel the maximum, minimum,
mean, count or first value of an int32 volume over the voxels the pixel ray crosses.  CPU: the ABI's layout; a scalar model of the
kernel's entry by rank and brick jump against the statement (tests/projection_ref.py) on seeded rays; box splits; an axis ray; the
statement against float64, both ways; the statement against the host form; the kernels' register figures.  GPU: every output
against the statement, bit for bit and with no pixel excluded; the brick table on against off; the orderings between the ops; the
device form; the lifecycle; every refusal; a full sphere without the statement; the drop-in class.

Grids: the lifecycle suite's 40 x 12 x 12, a 13 x 9 x 5 grid (no dim a multiple of 8, z below one brick), a 32^3 grid with a 16^3
block, and an 8^3 grid (one brick); and, for k_project_bricks' runs of 64 voxels along x, seven grids of 65 to 200 voxels a
row (LONG below) with cameras of their own."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import distance_ref as dr
import projection_model as pm
import projection_ref as pr
from conftest import SPHERE_CAM, make_camera

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOV = 45.0
GMIN, VOX = np.array([-0.5, -0.5, -0.5], np.float32), np.float32(1.0 / 64)
EXPO_DIRS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [-1, 2, 1]], np.int32)
SOURCES = ("distance", "geodesic", "thickness", "skeleton", "exposure", "parts", "labels")
BRICK_VGPRS, MARCH_VGPRS = 64, 40            # 8 waves per SIMD for the stream, 12 for the gather-bound march


def _hip():
    from ray_tracing_octrees_amd import hip
    return hip


def _lut():
    return _hip().ramp_lut([(0, 0, 96, 255), (0, 200, 255, 255), (255, 255, 0, 200), (255, 32, 0, 255)])


def _base():
    g = np.zeros((12, 12, 40), np.uint8)             # tests/test_field_lifecycle.py's grid
    g[2:10, 2:10, 4:20] = 1
    g[6, 6, 30] = 1
    return g


def _odd():
    g = np.zeros((5, 9, 13), np.uint8)
    g[1:4, 2:8, 2:11] = 1
    g[2, 4, 5:8] = 0
    return g


def _block32():
    g = np.zeros((32, 32, 32), np.uint8)
    g[8:24, 8:24, 8:24] = 1
    return g


def _one():
    g = np.zeros((8, 8, 8), np.uint8)
    g[1:7, 2:6, 1:8] = 1
    return g


GRIDS = {"base": _base, "odd": _odd, "block32": _block32, "one": _one}


def _dims(g):
    return (g.shape[2], g.shape[1], g.shape[0])


def _vpos(x, y, z):
    return (GMIN + np.array([x, y, z], np.float32) * VOX).astype(np.float32)


def _diag_view(pos):
    """A view that looks down the space diagonal (1, 1, 1): the centre ray of an odd frame has three equal components."""
    s = np.float32(1 / np.sqrt(3))
    f = np.array([s, s, s], np.float32)
    r = (np.array([1, -1, 0], np.float32) / np.float32(np.sqrt(2))).astype(np.float32)
    R = np.stack([r, np.cross(r, f).astype(np.float32), -f]).astype(np.float32)
    V = np.eye(4, dtype=np.float32)
    V[:3, :3] = R
    V[:3, 3] = -(R @ pos)
    return V.T.reshape(16).copy()


def _camera(orc, name, g):
    """(view, pos) by name for grid g, "name@R" for another orbit radius.  "outside": oblique, at the grid's centre.  "axis":
    theta = phi = 0, the view axes are the world axes and the position is a lattice point: zero components on the centre row
    and column of an odd frame, |dx| == |dy| on the diagonals of a square one.  "inside": in the grid.  "empty": inside a brick
    of the base grid that holds no solid voxel, looking at the block.  "plane": on the grid plane x = 20.  "diagonal": on the
    lattice point (-3, -3, -3), looking down the space diagonal.  "away": beside the grid, looking away from it."""
    name, _, radius = name.partition("@")
    dx, dy, dz = _dims(g)
    centre = _vpos(dx / 2, dy / 2, dz / 2)

    def orbit(th, ph, R, target):
        cam = orc.Camera(th, ph, float(radius) if radius else R)
        cam.set_target(*[float(v) for v in target])
        return cam.get_view(), cam.get_pos()
    if name == "outside":
        return orbit(0.6, 0.45, float(VOX) * max(dx, dy, dz) * 1.2, centre)
    if name == "axis":
        return orbit(0.0, 0.0, 0.5, _vpos(dx // 2, dy // 2, dz // 2))
    if name == "inside":
        return orbit(3.7, -0.45, 0.45, centre)[0], _vpos(dx * 0.3 + 0.5, dy * 0.3 + 0.3, dz * 0.3 + 0.4)
    if name == "empty":
        return orbit(0.1, 1.4, 0.45, _vpos(12, 6, 6))[0], _vpos(36.5, 4.5, 3.5)
    if name == "plane":
        return orbit(0.9, 0.3, 0.45, centre)[0], _vpos(20, 6.3, 5.2)
    if name == "diagonal":
        pos = _vpos(-3, -3, -3)
        return _diag_view(pos), pos
    if name == "away":
        return orbit(0.0, 0.0, 0.5, centre)[0], _vpos(dx / 2, dy / 2, -4)
    raise KeyError(name)


def _rays(orc, view, pos, W, H):
    return orc.generate_rays(view, pos, W / H, FOV, W, H).reshape(-1, 3)


def _frame(view, pos, W, H):
    return _hip().make_frame(view, pos, W / H, FOV, W, H)


def _proj(hip, code, op, **kw):
    return hip.make_field_projection(code, op, none_rgba=(0.5, 0.25, 0.125, 0.75), miss_rgba=(0.0, 0.125, 0.25, 1.0), **kw)


def _make_fields(ctx, g, which=SOURCES):
    """Builds grid g on the context and makes the named products; returns {source: (hip FIELD_* constant, the volume)}."""
    hip = _hip()
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g, GMIN, VOX)
    out = {}
    if "distance" in which:
        out["distance"] = (hip.FIELD_DISTANCE, ctx.distance_field(hip.SET_EMPTY)[0])
    if "geodesic" in which:
        out["geodesic"] = (hip.FIELD_GEODESIC, ctx.geodesic_field([0], hip.SET_EMPTY, hip.CONN_FACE)[0])
    if "thickness" in which:
        out["thickness"] = (hip.FIELD_THICKNESS, ctx.thickness_field(hip.SET_SOLID, 4 * float(VOX))[0])
    if "skeleton" in which:
        out["skeleton"] = (hip.FIELD_SKELETON, ctx.skeleton_field(hip.SET_SOLID, hip.CONN_FULL, hip.SKEL_TOPOLOGY)[0])
    if "exposure" in which:
        out["exposure"] = (hip.FIELD_EXPOSURE, ctx.exposure_field(EXPO_DIRS, None, hip.EXPO_SKIN, 8)[0])
    if "parts" in which:
        ctx.segment_parts(hip.SET_SOLID, hip.CONN_FACE, 1001)
        out["parts"] = (hip.FIELD_PARTS, ctx.part_labels())
    if "labels" in which:
        ctx.label_components(hip.SET_SOLID, hip.CONN_FACE)
        out["labels"] = (hip.FIELD_LABELS, ctx.component_labels())
    return out


NAMES = ("rgba", "values", "voxels", "sums", "counts", "summary", "bins")


def _same(got, want, what):
    """A frame's seven results against the statement's (or another frame's), bit for bit; an output only where both hold it."""
    for name, a, b in zip(NAMES, got, want):
        if a is None or b is None:
            continue
        if name == "summary":
            assert a.tolist() == b.tolist(), (what, a, b)
        elif name == "rgba":
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), \
                f"{what}: {int((a.view(np.uint32) != b.view(np.uint32)).any(-1).sum())} pixels differ"
        else:
            assert np.array_equal(a, b), f"{what}: {int((np.asarray(a) != np.asarray(b)).sum())} {name} differ"


# ================================================================ CPU
def test_projection_struct_matches_the_header():
    """ctypes rto_field_projection is the header's: size, field order and offsets; the constants; the symbols exported."""
    hip = _hip()
    V = hip.FieldProjection
    assert C.sizeof(V) == 112
    offs = {name: getattr(V, name).offset for name, _ in V._fields_}
    assert offs == {"source": 0, "op": 4, "scale": 8, "valid_lo": 12, "valid_hi": 16, "range_lo": 20, "range_hi": 24, "clip": 28,
                    "clip_lo": 32, "clip_hi": 44, "miss_rgba": 56, "none_rgba": 72, "reserved": 88}
    hdr = open(os.path.join(ROOT, "include", "rto_hip.h")).read()
    body = re.search(r"typedef struct rto_field_projection \{(.*?)\} rto_field_projection;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in re.findall(r"(?:float|int32_t|int64_t)\s+([^;]+);", body):
        names += [re.sub(r"\[\d+\]", "", n).strip() for n in decl.split(",")]
    assert names == [n for n, _ in V._fields_]
    for k, name in enumerate(("MAX", "MIN", "MEAN", "COUNT", "FIRST")):
        assert re.search(r"#define RTO_PROJECT_%s\s+%d\b" % (name, k), hdr) and getattr(hip, "PROJECT_" + name) == k == getattr(pr, name)
    lib = hip.load()
    for sym in ("rto_project_field_device", "rto_project_field_host", "rto_last_projection_ms", "rto_debug_set_projection_table"):
        assert sym in hip.SYMBOLS and hasattr(lib, sym) and re.search(r"\b%s\(" % sym, hdr), sym
    assert "static_assert(sizeof(rto_field_projection) == 112" in open(
        os.path.join(ROOT, "ray_tracing_octrees_amd", "csrc", "rto_project.inc")).read()
    v = hip.make_field_projection(hip.FIELD_THICKNESS)
    assert (v.op, v.valid_lo, v.valid_hi, v.range_lo, v.range_hi, v.clip, list(v.reserved)) == (0, 0, 0x7ffffffe, 0, 0, 0, [0] * 6)


def _seeded_rays(seed, n):
    """(grid_min, voxel, dim, o, d, lo, hi) of n rays in six families: exact-lattice rays (integer gridMin, voxel 1, integer
    origin and target: they pass through voxel edges and corners), the same normalised, still axes (0, -0.0 and components whose
    reciprocal overflows), origins inside the grid or on a plane, origins 10^2 .. 10^7 away (consecutive planes share a T), and
    plain rays at the grid; half of them with a random box."""
    rng = np.random.default_rng(seed)
    for i in range(n):
        kind = i % 6
        dim = tuple(int(v) for v in rng.integers(1, 22, 3))
        fdim = np.array(dim, np.float32)
        if kind in (0, 1):
            g, vs = rng.integers(-5, 5, 3).astype(np.float32), np.float32(1)
            o = (g + rng.integers(-6, 28, 3)).astype(np.float32)
            d = ((g + rng.integers(0, np.array(dim) + 1)).astype(np.float32) - o).astype(np.float32)
            if kind == 1:
                d = (d / np.float32(np.sqrt((d * d).sum()) or 1)).astype(np.float32)
        elif kind == 2:
            g, vs = rng.uniform(-1, 1, 3).astype(np.float32), np.float32(rng.uniform(0.01, 0.3))
            o = (g + rng.uniform(-0.2, 1.2, 3).astype(np.float32) * vs * fdim).astype(np.float32)
            d = ((g + rng.uniform(0, 1, 3).astype(np.float32) * vs * fdim) - o).astype(np.float32)
            for a in rng.choice(3, rng.integers(1, 3), replace=False):
                d[a] = np.float32([0.0, -0.0, 1e-42, -1e-45][rng.integers(0, 4)])
        elif kind == 3:
            g, vs = rng.uniform(-1, 1, 3).astype(np.float32), np.float32(1 / 64)
            o = (g + (rng.integers(0, np.array(dim) + 1).astype(np.float32) * vs).astype(np.float32)).astype(np.float32)
            if rng.integers(0, 2):
                o[rng.integers(0, 3)] += np.float32(rng.uniform(0, 1)) * vs
            d = rng.normal(size=3).astype(np.float32)
        elif kind == 4:
            g, vs = rng.uniform(-1, 1, 3).astype(np.float32), np.float32(1 / 64)
            d = rng.normal(size=3).astype(np.float32)
            d = (d / np.float32(np.sqrt((d * d).sum()))).astype(np.float32)
            o = ((g + np.float32(0.5) * vs * fdim) - d * np.float32(10.0 ** rng.uniform(2, 7))).astype(np.float32)
        else:
            g, vs = rng.uniform(-1, 1, 3).astype(np.float32), np.float32(rng.uniform(0.01, 0.3))
            o = (g + rng.uniform(-1, 2, 3).astype(np.float32) * vs * np.float32(max(dim))).astype(np.float32)
            d = ((g + rng.uniform(0, 1, 3).astype(np.float32) * vs * fdim) - o).astype(np.float32)
        lo = hi = None
        if rng.integers(0, 2):
            lo = tuple(int(rng.integers(0, dim[a])) for a in range(3))
            hi = tuple(int(rng.integers(lo[a] + 1, dim[a] + 1)) for a in range(3))
        yield kind, g, vs, dim, o, d.astype(np.float32), lo, hi


def _runs(cells):
    """The brick sequence of a walk: (brick, its first voxel) of every run of voxels in one brick."""
    out = []
    for c in cells:
        b = (c[0] >> 3, c[1] >> 3, c[2] >> 3)
        if not out or out[-1][0] != b:
            out.append((b, c))
    return out


def test_entry_by_rank_and_brick_jump_equal_the_plain_walk():
    """The kernel's traversal as a scalar model (tests/projection_model.py: entry by rank, one step per event from the integer
    plane index, a jump to the state after a brick's exit event) against the statement's sort-everything walk, on 3,000 seeded
    rays: the model's voxels are the statement's in order; with every brick skipped the bricks it consults and the voxel it
    enters each at are the walk's runs; with a third of the bricks skipped it samples exactly the voxels of the others.  The
    families must bite: ties between axes, still axes, starts inside and walks that begin in the grid's interior."""
    n = {k: 0 for k in range(6)}
    ties = still = started_inside = 0
    for kind, g, vs, dim, o, d, lo, hi in _seeded_rays(7, 3000):
        want = pr.walk(g, vs, dim, o, d, lo, hi)
        cells, _ = pm.march(g, vs, dim, o, d, lo, hi)
        assert cells == want, (kind, g, vs, dim, o, d, lo, hi)
        runs = _runs(want)
        _, bricks = pm.march(g, vs, dim, o, d, lo, hi, skip=lambda b: True)
        assert bricks == runs, (kind, g, vs, dim, o, d, lo, hi)
        drop = {b for b, _ in runs if (b[0] + 2 * b[1] + b[2]) % 3 == 0}
        some, _ = pm.march(g, vs, dim, o, d, lo, hi, skip=lambda b: b in drop)
        assert some == [c for c in want if (c[0] >> 3, c[1] >> 3, c[2] >> 3) not in drop], (kind, g, vs, dim, o, d, lo, hi)
        if want:
            n[kind] += 1
            with np.errstate(all="ignore"):
                inv = np.float32(1) / d
            moving = [a for a in range(3) if np.isfinite(inv[a])]
            still += len(moving) < 3
            ts = np.concatenate([pr.plane_t(g, vs, dim, o, inv, a) for a in moving])
            ts = ts[ts > 0]
            ties += len(np.unique(ts)) < len(ts)
            started_inside += all(0 <= (o[a] - g[a]) / vs < dim[a] for a in range(3))
    assert min(n.values()) >= 60, n
    assert ties >= 200 and still >= 60 and started_inside >= 60, (ties, still, started_inside)


def test_a_split_box_partitions_the_visited_voxels():
    """For every axis and every cut: the walk in [lo, cut) and the walk in [cut, hi) are disjoint, and together they are the walk
    in [lo, hi) -- as sets and, merged by walk position, as sequences.  The rule has no t window, so this holds by construction;
    a rule that walks inside a slab window lost or doubled voxels here."""
    checked = 0
    for kind, g, vs, dim, o, d, lo, hi in _seeded_rays(11, 600):
        lo = (0, 0, 0) if lo is None else lo
        hi = dim if hi is None else hi
        whole = pr.walk(g, vs, dim, o, d, lo, hi)
        for a in range(3):
            for cut in range(lo[a] + 1, hi[a]):
                left = pr.walk(g, vs, dim, o, d, lo, tuple(cut if b == a else hi[b] for b in range(3)))
                right = pr.walk(g, vs, dim, o, d, tuple(cut if b == a else lo[b] for b in range(3)), hi)
                assert not set(left) & set(right) and len(left) + len(right) == len(whole)
                assert [c for c in whole if c[a] < cut] == left and [c for c in whole if c[a] >= cut] == right
                checked += bool(left) and bool(right)
    assert checked >= 500


def test_an_axis_ray_through_voxel_centres_visits_its_column():
    """Along +x, -x, +y, -y, +z and -z through the centre of voxel (5, 3, 2) of a 13 x 9 x 5 grid, from outside and from inside:
    exactly that column (or what is left of it in front of the origin), in the direction of travel; -0.0 components included."""
    dim = (13, 9, 5)
    centre = [5, 3, 2]
    for a in range(3):
        for sign in (1, -1):
            for start in (-3.5, centre[a] + 0.5):
                d = np.array([-0.0, 0.0, -0.0], np.float32)
                d[a] = sign
                at = [c + 0.5 for c in centre]
                at[a] = start if sign > 0 else (dim[a] + 3.5 if start < 0 else start)
                o = _vpos(*at)
                col = list(range(dim[a])) if sign > 0 else list(range(dim[a] - 1, -1, -1))
                if start >= 0:
                    col = [c for c in col if (c >= centre[a] if sign > 0 else c <= centre[a])]
                want = [tuple(c if b == a else centre[b] for b in range(3)) for c in col]
                assert pr.walk(GMIN, VOX, dim, o, d) == want, (a, sign, start)
                assert pm.march(GMIN, VOX, dim, o, d)[0] == want


def test_the_statement_against_float64_both_ways():
    """The float32 statement against the ray in float64, on 600 seeded rays at a 20 x 17 x 11 grid of voxel 1/64 at (-0.5, -0.5,
    -0.5), origins within two grid sizes, one ray in five with a still axis.

    The bound.  The statement's T_a(j) = fl(fl(fl(g + fl(j v)) - o) fl(1 / d)): ref64's slab error terms, one rounding u = 2^-24
    per operation.  With M = 4 above every |j v|, |P| and |o|, so |P - o| <= 2 M: the numerator is off by at most u (M + M + 2 M),
    the reciprocal and the product add 2 u |T| in relative terms.  Multiplied by |d_a| -- the ray moves |d_a| along axis a per
    unit of t -- the plane the float event stands for lies within delta = u (4 M) + 2 u |P - o| <= 8 u M of the true plane,
    along its own axis, whatever |d_a| is.  A still axis' coordinate floor(fl(fl(o - g) / v)) is off by at most 2 u |o - g| <=
    4 u M <= delta in space.  A voxel is visited exactly when its latest entering event is ordered before its earliest leaving
    event.  So, with EPS = 2 delta = 16 u M (3.8e-6, 0.02 % of a voxel):
      (a) every visited voxel's box, grown by EPS on every side, is met by the float64 ray at some t >= 0 (delta would do);
      (b) every voxel whose box shrunk by EPS on every side is still met by the float64 ray is visited: its exact entering
          events, moved late by delta, still come strictly before its leaving events moved early by delta, so no tie rule can
          drop it.  In terms of the chord: a shrunk per-axis interval loses EPS / |d_a| of t at each end, so every voxel the
          float64 ray crosses with a chord longer than 2 EPS / min |d_a| over the moving axes (|d| = 1: t is length) is among
          them.  The test asserts the shrunk-box form, which asks for more voxels than the chord form does."""
    u, M = 2.0 ** -24, 4.0
    EPS = 16 * u * M
    dim = (20, 17, 11)
    rng = np.random.default_rng(3)
    g64, v64 = GMIN.astype(np.float64), float(VOX)
    checked_a = checked_b = 0
    ix, iy, iz = np.meshgrid(np.arange(dim[0]), np.arange(dim[1]), np.arange(dim[2]), indexing="ij")
    lo_all = g64 + np.stack([ix, iy, iz], -1).reshape(-1, 3) * v64
    for _ in range(600):
        o = (GMIN + rng.uniform(-1, 2, 3).astype(np.float32) * VOX * np.float32(20)).astype(np.float32)
        tgt = GMIN + rng.uniform(0, 1, 3).astype(np.float32) * VOX * np.array(dim, np.float32)
        d = (tgt - o).astype(np.float32)
        d = (d / np.float32(np.sqrt((d * d).sum()))).astype(np.float32)
        if rng.integers(0, 5) == 0:
            d[rng.integers(0, 3)] = 0
        cells = pr.walk(GMIN, VOX, dim, o, d)
        o64, d64 = o.astype(np.float64), d.astype(np.float64)

        def meets(lo, hi):
            """Does the float64 ray (t >= 0) meet the boxes [lo, hi] (n, 3)?"""
            with np.errstate(all="ignore"):
                t1, t2 = (lo - o64) / d64, (hi - o64) / d64
            tn, tf = np.minimum(t1, t2), np.maximum(t1, t2)
            for a in range(3):
                if d64[a] == 0:
                    inside = (lo[:, a] <= o64[a]) & (o64[a] <= hi[:, a])
                    tn[:, a], tf[:, a] = np.where(inside, -np.inf, np.inf), np.where(inside, np.inf, -np.inf)
            return np.maximum(tn.max(1), 0) <= tf.min(1)
        if cells:
            lo = g64 + np.array(cells, np.float64) * v64
            assert meets(lo - EPS, lo + v64 + EPS).all(), (o, d)
            checked_a += len(cells)
        sure = meets(lo_all + EPS, lo_all + v64 - EPS)
        must = {tuple(int(x) for x in c) for c in np.stack([ix, iy, iz], -1).reshape(-1, 3)[sure]}
        assert must <= set(cells), (o, d, sorted(must - set(cells))[:3])
        checked_b += len(must)
    assert checked_a > 10000 and checked_b > 9000, (checked_a, checked_b)


def test_the_statement_against_the_host_form():
    """host/Projection (the plain voxel-by-voxel walk in C++) through host_capi, on the seeded rays: the same voxels in the same
    order; and every op's value, voxel, sum and count on a volume of adversarial values."""
    from ray_tracing_octrees_amd import host
    L = host.load()
    adv = np.array([0, 1, 0x7ffffffe, -1, -7, -2 ** 31 + 2, 0x7fffffff, 2, 1000, -2 ** 30], np.int64)
    nonempty = 0
    for kind, g, vs, dim, o, d, lo, hi in _seeded_rays(5, 1200):
        want = pr.walk(g, vs, dim, o, d, lo, hi)
        cap = sum(dim) + 4
        out = np.zeros((cap, 3), np.int32)
        gm = np.ascontiguousarray(g, np.float32)
        blo = np.array(lo if lo is not None else (0, 0, 0), np.int32)
        bhi = np.array(hi if hi is not None else dim, np.int32)
        dims = np.array(dim, np.int32)
        oo, dd = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
        n = L.rtoh_projection_walk(gm.ctypes.data, C.c_float(float(vs)), dims.ctypes.data, oo.ctypes.data, dd.ctypes.data, blo.ctypes.data,
                                   bhi.ctypes.data, out.ctypes.data, cap)
        assert n == len(want) and [tuple(r) for r in out[:n].tolist()] == want, (kind, g, vs, dim, o, d, lo, hi)
        if not want:
            continue
        nonempty += 1
        idx = np.arange(dim[0] * dim[1] * dim[2]).reshape(dim[2], dim[1], dim[0])
        vol = np.ascontiguousarray(adv[(idx * 7 + idx // 5) % len(adv)].astype(np.int32))
        for op in pr.OPS:
            for window in ((-2 ** 31 + 2, 2 ** 31 - 1), (0, 0x7ffffffe), (-7, -1)):
                res = np.zeros(4, np.int64)
                L.rtoh_projection_reduce(vol.ctypes.data, dims.ctypes.data, out.ctypes.data, n, op, window[0], window[1], res.ctypes.data)
                assert tuple(res.tolist()) == pr.reduce(want, vol, op, *window), (op, window)
    assert nonempty > 300


def test_projection_kernels_keep_their_budgets():
    """The built metadata (the product's flags): k_project_bricks and the five k_project_march kernels without scratch or
    spills, within the VGPR counts DESIGN.md section 28 quotes and argues from occupancy: 64 for the streaming brick kernel (8
    waves per SIMD with eight 256-byte loads in flight each cover the memory latency at full bandwidth), 40 for the march (12
    waves per SIMD: its trips are dependent 4-byte gathers that only other waves can hide)."""
    import test_isa_contract as isa
    asm = isa.built_asm()
    if asm is None:
        pytest.skip("no hipcc in this environment")
    meta = isa.kernel_meta(asm)
    names = [k for k in meta if "k_project_" in k]
    assert len(names) == 6 and len([k for k in names if "k_project_march" in k]) == 5, names
    for k in names:
        m = meta[k]
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (k, m)
        assert m["vgpr"] <= (MARCH_VGPRS if "march" in k else BRICK_VGPRS), (k, m)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("## 28."):]
    assert re.search(r"k_project_bricks[^.]*\b%d VGPRs" % BRICK_VGPRS, sec) and re.search(r"k_project_march[^.]*\b%d VGPRs" % MARCH_VGPRS, sec)


# ---------------------------------------------------------------- long rows: more than one run of 8 bricks along x
TENTH = (np.full(3, 0.3, np.float32), np.float32(0.1))
# name: (dimX, dimY, dimZ, (gridMin, voxelSize)).  k_project_bricks gives one wave to a run of 8 bricks (64 voxels) along x:
# "long65" the second run holds one column, "long72" exactly one brick (nbx = 9), "long100" five bricks, the last of four
# columns (nbx = 13; 6 waves, so the last workgroup is half empty), "long128" two whole runs (nbx = 16), "long130" three runs,
# the last of two columns (nbx = 17), "long200" four runs over one row of bricks (nbx = 25); "long130-tenth" is long130 at
# voxel 0.1, origin 0.3.
LONG = {"long65": (65, 9, 5, (GMIN, VOX)), "long72": (72, 12, 9, (GMIN, VOX)), "long100": (100, 5, 17, (GMIN, VOX)),
        "long128": (128, 9, 5, (GMIN, VOX)), "long130": (130, 9, 9, (GMIN, VOX)), "long200": (200, 5, 3, (GMIN, VOX)),
        "long130-tenth": (130, 9, 9, TENTH)}
LONG_OPS = (pr.MAX, pr.MIN, pr.COUNT, pr.FIRST)     # the table's two keys; its "no valued voxel" skip
LW, LH = 24, 16
_LONG = {}


def _long_grid(name):
    """All solid but for the plane x = 0, a tunnel along x through the boundary of the first two runs and one voxel at the far
    end: the distance to EMPTY changes along the whole row, up to 29^2 in the 130-voxel grids."""
    dx, dy, dz, _ = LONG[name]
    g = np.ones((dz, dy, dx), np.uint8)
    g[:, :, 0] = 0
    g[dz // 2, dy // 2, 58:min(70, dx)] = 0
    g[0, 0, dx - 1] = 0
    return g


def _long_volume(name):
    """A caller's volume whose valued voxels all lie at x >= 64: a frame changes when a table entry of a later run is wrong."""
    dx, dy, dz, _ = LONG[name]
    idx = np.arange(dx * dy * dz, dtype=np.int64).reshape(dz, dy, dx)
    return np.where((idx % dx >= 64) & ((idx * 7 + idx // dx) % 5 != 0), (idx * 37) % 101, -1).astype(np.int32)


def _x_view(pos, sign):
    """A view that looks along +x or -x with y to the right and the world's -z or z up; _diag_view's construction."""
    f = np.array([sign, 0, 0], np.float32)
    r = np.array([0, 1, 0], np.float32)
    R = np.stack([r, np.cross(r, f).astype(np.float32), -f]).astype(np.float32)
    V = np.eye(4, dtype=np.float32)
    V[:3, :3] = R
    V[:3, 3] = -(R @ pos)
    return V.T.reshape(16).copy()


def _long_frames(orc, name):
    """[(camera, view, pos, rays, the statement's walks)] of a long grid, made once.  "end": 6 voxels beyond the +x face, looking
    along -x.  "inside": in the grid at (60.5, 0.3, 0.2), looking along +x: the central ray that leans towards +y and +z
    stays in a cross-section of 5 x 3 voxels for 100 voxels.  "plane": on the grid plane x = 64, looking along +x (every
    plane T of that axis up to 64 is <= 0).  "orbit": the suite's oblique camera 12 voxels from the point (max(64, dimX / 2), dimY /
    2, dimZ / 2); at the suite's usual radius it sees next to nothing of such a grid."""
    if name not in _LONG:
        dx, dy, dz, (gmin, vox) = LONG[name]
        at = lambda x, y, z: (gmin + (np.array([x, y, z], np.float32) * vox).astype(np.float32)).astype(np.float32)
        cams = []
        pos = at(dx + 6, dy / 2 + 0.3, dz / 2 + 0.2)
        cams.append(("end", _x_view(pos, -1), pos))
        pos = at(60.5, 0.3, 0.2)
        cams.append(("inside", _x_view(pos, 1), pos))
        pos = at(64, dy / 2 - 0.3, dz / 2 + 0.2)
        cams.append(("plane", _x_view(pos, 1), pos))
        cam = orc.Camera(0.6, 0.45, float(np.float32(12 * float(vox))))
        cam.set_target(*[float(v) for v in at(max(64, dx / 2), dy / 2, dz / 2)])
        cams.append(("orbit", cam.get_view(), cam.get_pos()))
        out = []
        for cname, view, pos in cams:
            rd = _rays(orc, view, pos, LW, LH)
            out.append((cname, view, pos, rd, pr.walks(gmin, vox, (dx, dy, dz), pos, rd)))
        _LONG[name] = out
    return _LONG[name]


def _long_runs(hip, cname, cells, vol, field):
    """[(projection, caller volume or None, the statement's frame)] of a long grid's frame: MAX, MIN, COUNT and FIRST of the x >=
    64 volume, MAX of the distance to EMPTY.  Each has at least 50 valued pixels and, but for FIRST (one value may lead every
    walk) and the distance from the "inside" camera (its own voxel holds the maximum of every walk), two LUT indices."""
    runs = [(_proj(hip, hip.FIELD_CALLER, op, scale=hip.SCALE_SQRT if op == pr.COUNT else hip.SCALE_LINEAR), vol) for op in LONG_OPS]
    runs.append((_proj(hip, hip.FIELD_DISTANCE, pr.MAX, scale=hip.SCALE_SQRT, valid=(1, 0x7ffffffe)), None))
    out = []
    for v, volume in runs:
        want = pr.frame_of(cells, LW, LH, field if volume is None else volume, v, _lut())
        assert want[5]["valued"] >= 50, (cname, v.source, v.op, want[5])
        if not (v.op == pr.FIRST or (volume is None and cname == "inside")):
            assert not pr.degenerate(want[1], v), (cname, v.source, v.op, want[5])
        out.append((v, volume, want))
    return out


def _crosses_63_64(c):
    return any({a[0], b[0]} == {63, 64} for a, b in zip(c, c[1:]))


@pytest.mark.parametrize("name", list(LONG))
def test_long_row_frames_bite_and_feel_the_later_runs(orc, name):
    """On the statement alone.  Every frame of a long grid: at least 100 pixels visit something and at least 50 walks hold a
    voxel with x >= 64 (what a later run's table entries cover).  Over the grid's four frames: at least 50 walks cross x = 63 |
    64 and one is at least dimX / 2 voxels long.  (No single camera can do all four on every grid: a walk from the plane x =
    64 never crosses it, and in a 9 x 5 cross-section a walk that starts before x = 32 meets column 64 on a pixel or two.)  The
    "plane" camera stands on the plane, the "inside" camera in the grid.
    Sensitivity: tests/projection_model.py's march with a table that calls every brick of the runs >= 1 empty (skip = bx >= 8)
    gives another frame than the statement under every op, on at least 50 pixels of every frame."""
    dx, dy, dz, (gmin, vox) = LONG[name]
    dim = (dx, dy, dz)
    vol = _long_volume(name)
    field = dr.field(_long_grid(name), dr.SET_EMPTY)
    hip = _hip()
    frames = _long_frames(orc, name)
    for cname, view, pos, rd, cells in frames:
        assert sum(bool(c) for c in cells) >= 100, (name, cname)
        later = [any(x >= 64 for x, _, _ in c) for c in cells]
        assert sum(later) >= 50, (name, cname, sum(later))
        q = (pos - gmin) / vox
        if cname in ("inside", "plane"):
            assert all(0 <= q[a] < dim[a] for a in range(3)), (name, cname)
        if cname == "plane":
            assert pos[0] == np.float32(gmin[0] + np.float32(np.float32(64) * vox))
            assert {c[0][0] for c in cells if c} == {64}
        skipped = [pm.march(gmin, vox, dim, pos, d, skip=lambda b: b[0] >= 8)[0] if far else c for d, c, far in zip(rd, cells, later)]
        assert all(s == [v for v in c if v[0] < 64] for s, c in zip(skipped, cells))
        for v, volume, want in _long_runs(hip, cname, cells, vol, field):
            if volume is None:                     # the distance's maximum may lie in the first run: no promise
                continue
            blind = pr.frame_of(skipped, LW, LH, volume, v, _lut())
            assert (want[1] != blind[1]).sum() >= 50 and want[0].tobytes() != blind[0].tobytes(), (name, cname, v.source, v.op)
    assert sum(_crosses_63_64(c) for _, _, _, _, cells in frames for c in cells) >= 50
    assert max(len(c) for _, _, _, _, cells in frames for c in cells) >= dx / 2
    assert ((dx + 7) // 8 + 7) // 8 >= 2                                      # the kernel's runsX


@pytest.mark.parametrize("name", list(LONG))
def test_long_row_frames_against_the_host_form(orc, name):
    """host/Projection through host_capi on every pixel ray of the long grids' frames: the statement's voxels in the statement's
    order, and its value, voxel, sum and count under every op on the x >= 64 volume."""
    from ray_tracing_octrees_amd import host
    L = host.load()
    dx, dy, dz, (gmin, vox) = LONG[name]
    vol = np.ascontiguousarray(_long_volume(name))
    dims = np.array([dx, dy, dz], np.int32)
    gm = np.ascontiguousarray(gmin, np.float32)
    blo, bhi = np.zeros(3, np.int32), dims.copy()
    cap = dx + dy + dz + 4
    out = np.zeros((cap, 3), np.int32)
    res = np.zeros(4, np.int64)
    valued = 0
    for cname, view, pos, rd, cells in _long_frames(orc, name):
        oo = np.ascontiguousarray(pos, np.float32)
        for d, want in zip(rd, cells):
            dd = np.ascontiguousarray(d, np.float32)
            n = L.rtoh_projection_walk(gm.ctypes.data, C.c_float(float(vox)), dims.ctypes.data, oo.ctypes.data, dd.ctypes.data, blo.ctypes.data,
                                       bhi.ctypes.data, out.ctypes.data, cap)
            assert n == len(want) and [tuple(r) for r in out[:n].tolist()] == want, (name, cname, d)
            for op in pr.OPS:
                L.rtoh_projection_reduce(vol.ctypes.data, dims.ctypes.data, out.ctypes.data, n, op, 0, 0x7ffffffe, res.ctypes.data)
                assert tuple(res.tolist()) == pr.reduce(want, vol, op, 0, 0x7ffffffe), (name, cname, op)
            valued += res[3] > 0
    assert valued >= 200


# ================================================================ GPU
_WALKS = {}


def _walks(orc, gname, cam, W, H, proj=None):
    """(view, pos, the statement's walks) of a frame, made once per grid, camera, frame and box."""
    box = (tuple(proj.clip_lo), tuple(proj.clip_hi)) if proj is not None and proj.clip else None
    key = (gname, cam, W, H, box)
    if key not in _WALKS:
        g = GRIDS[gname]()
        view, pos = _camera(orc, cam, g)
        _WALKS[key] = (view, pos, pr.walks(GMIN, VOX, _dims(g), pos, _rays(orc, view, pos, W, H), proj))
    return _WALKS[key]


# (grid, camera, W, H, source, op, make_field_projection's keywords, totals)
CASES = [
    ("base", "outside", 24, 16, "distance", "MAX", dict(scale=1), False),
    ("base", "outside", 24, 16, "geodesic", "MIN", dict(), False),
    ("base", "outside", 13, 9, "thickness", "MEAN", dict(scale=1), True),
    ("base", "outside", 24, 16, "skeleton", "MEAN", dict(), True),
    ("base", "axis@0.25", 13, 9, "geodesic", "COUNT", dict(), True),
    ("base", "axis@0.25", 8, 8, "distance", "MAX", dict(valid=(1, 0x7ffffffe)), False),
    ("base", "inside", 24, 16, "exposure", "FIRST", dict(), False),
    ("base", "inside", 24, 16, "parts", "COUNT", dict(scale=2, valid=(1, 0x7ffffffe)), True),
    ("base", "empty", 24, 16, "labels", "COUNT", dict(), False),
    ("base", "empty", 24, 16, "distance", "MAX", dict(valid=(1, 0x7ffffffe)), False),
    ("base", "plane", 72, 8, "distance", "MEAN", dict(valid=(1, 0x7ffffffe), range=(1, 12)), True),
    ("base", "diagonal", 13, 9, "distance", "MAX", dict(valid=(1, 0x7ffffffe)), False),
    ("base", "diagonal", 13, 9, "thickness", "COUNT", dict(valid=(1, 0x7ffffffe)), True),
    ("base", "outside", 1, 1, "distance", "MIN", dict(), True),
    ("base", "outside", 24, 16, "geodesic", "FIRST", dict(valid=(10, 0x7ffffffe), clip=((0, 0, 0), (19, 12, 12))), False),
    ("odd", "outside", 24, 16, "distance", "MAX", dict(valid=(1, 0x7ffffffe)), False),
    ("odd", "outside", 13, 9, "geodesic", "MIN", dict(), False),
    ("odd", "inside", 24, 16, "geodesic", "FIRST", dict(valid=(0, 0x7ffffffe), scale=2), False),
    ("odd", "axis@0.125", 8, 8, "distance", "MEAN", dict(valid=(1, 0x7ffffffe), scale=1), True),
    ("block32", "outside", 24, 16, "distance", "MAX", dict(scale=1, valid=(1, 0x7ffffffe)), False),
    ("block32", "outside@0.6", 13, 9, "thickness", "MIN", dict(valid=(1, 0x7ffffffe)), False),
    ("block32", "inside", 72, 8, "geodesic", "FIRST", dict(valid=(0, 0x7ffffffe)), False),
    ("one", "outside", 8, 8, "distance", "MAX", dict(valid=(1, 0x7ffffffe)), False),
    ("one", "inside", 24, 16, "distance", "COUNT", dict(valid=(1, 0x7ffffffe)), True),
]


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c[:6]) + "".join("-%s" % k for k in c[6]))
def test_gpu_frames_equal_the_statement(ctx, orc, case):
    """Every output of a frame, bit for bit against projection_ref on the same volume: every op, every source, the four grids,
    frames of partial tiles, one pixel, one tile and nine tiles; cameras outside, on the axes at a lattice point, inside the
    grid, inside a brick the table skips, on a grid plane and on a lattice point looking down the space diagonal.  The
    statement's own frame is first shown not to be degenerate: at least 20 valued pixels and two LUT indices (a frame of one
    pixel: that pixel is valued)."""
    hip = _hip()
    gname, cam, W, H, source, op, kw, totals = case
    g = GRIDS[gname]()
    code, vol = _make_fields(ctx, g, (source,))[source]
    v = _proj(hip, code, getattr(hip, "PROJECT_" + op), **kw)
    view, pos, cells = _walks(orc, gname, cam, W, H, v)
    want = pr.frame_of(cells, W, H, vol, v, _lut())
    if W * H == 1:
        assert want[5]["valued"] == 1
    else:
        assert not pr.degenerate(want[1], v), (case, want[5])
    rd = _rays(orc, view, pos, W, H)
    if cam.startswith("axis") and W % 2:
        assert (rd == 0).sum(1).max() == 2
    if cam.startswith("axis") and W == H:
        assert (np.abs(rd[:, 0]) == np.abs(rd[:, 1])).sum() == 2 * W
    if cam == "diagonal":
        centre = rd[(H // 2) * W + W // 2]
        assert centre[0] == centre[1] == centre[2] and len(cells[(H // 2) * W + W // 2]) >= 30
    if cam in ("inside", "empty", "plane"):
        assert all(0 <= (pos[a] - GMIN[a]) / VOX < _dims(g)[a] for a in range(3))
    if cam == "empty":
        x, y, z = [int((pos[a] - GMIN[a]) / VOX) >> 3 for a in range(3)]
        window = (vol >= v.valid_lo) & (vol <= v.valid_hi)
        assert not window[z * 8:z * 8 + 8, y * 8:y * 8 + 8, x * 8:x * 8 + 8].any()           # the camera's own brick is skipped
    _same(ctx.project_field_host(_frame(view, pos, W, H), v, _lut(), totals=totals), want, str(case))


@gpu
def test_gpu_looking_away_is_a_frame_of_misses(ctx, orc):
    """A camera beside the grid that looks away from it: every pixel is a miss, the frame is miss_rgba, the summary zero."""
    hip = _hip()
    g = _base()
    code, vol = _make_fields(ctx, g, ("distance",))["distance"]
    view, pos, cells = _walks(orc, "base", "away", 13, 9)
    assert not any(cells)
    for op in pr.OPS:
        v = _proj(hip, code, op)
        got = ctx.project_field_host(_frame(view, pos, 13, 9), v, _lut())
        _same(got, pr.frame_of(cells, 13, 9, vol, v, _lut()), f"away {op}")
        assert (got[1] == hip.FIELD_PIXEL_MISS).all() and (got[2] == -1).all() and got[5].tolist() == (0, 0, 0, 0, 0, 0)
        assert (got[0] == np.float32([0.0, 0.125, 0.25, 1.0])).all()


ADVERSARIAL = np.array([0, 1, 0x7ffffffe, -1, -7, -2 ** 31 + 2, 0x7fffffff, 2, 1000, -2 ** 30], np.int64)


def _caller_volumes(g):
    """{name: (volume, valid window)} for the base grid: one valued voxel in the far corner brick, all valued, none valued, the
    adversarial values under a window that takes them all, and a maximum that repeats along x."""
    n = g.size
    idx = np.arange(n).reshape(g.shape)
    wide = (-2 ** 31 + 2, 2 ** 31 - 1)
    lone = np.full(g.shape, -1, np.int32)
    lone[11, 11, 39] = 5
    ridge = ((idx // 40) % 7 + 1).astype(np.int32)                    # constant along x: every row repeats its maximum
    ridge[:, :, ::3] += 20
    return {"lone": (lone, (0, 0x7ffffffe)), "all": (((idx * 37) % 101).astype(np.int32), (0, 0x7ffffffe)),
            "none": (np.full(g.shape, -1, np.int32), (0, 0x7ffffffe)),
            "adversarial": (ADVERSARIAL[(idx * 7 + idx // 40) % len(ADVERSARIAL)].astype(np.int32), wide),
            "negative": ((np.where(idx % 3 == 0, -7, -2) - (idx // 40) % 5).astype(np.int32), wide), "ridge": (ridge, (0, 0x7ffffffe))}


@gpu
@pytest.mark.parametrize("name", ["lone", "all", "none", "adversarial", "negative", "ridge"])
def test_gpu_caller_volumes(ctx, orc, name):
    """A caller's volume under every op, with and without the totals, with the brick table and without it: all equal the
    statement, hence each other.  "lone": the frame is NONE but for the rays through the one voxel, and the table skips all
    other bricks.  "adversarial": INT32_MIN + 2 and INT32_MAX in one window; "negative": MEAN floors a negative sum towards
    minus infinity (the statement's values are checked to be of that kind).  "ridge": the maximum repeats along the ray, and
    d_voxels is its first holder."""
    hip = _hip()
    g = _base()
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g, GMIN, VOX)
    vol, window = _caller_volumes(g)[name]
    cam = "axis@0.3" if name == "ridge" else "outside"
    W, H = 24, 16
    view, pos, cells = _walks(orc, "base", cam, W, H)
    f = _frame(view, pos, W, H)
    try:
        for op in pr.OPS:
            v = _proj(hip, hip.FIELD_CALLER, op, valid=window, scale=hip.SCALE_SQRT if op == pr.COUNT else hip.SCALE_LINEAR)
            want = pr.frame_of(cells, W, H, vol, v, _lut())
            assert want[5]["hits"] >= 100
            if name == "lone":
                assert 1 <= want[5]["valued"] < 10 and (want[2][want[2] >= 0] == vol.size - 1).all()
            elif name == "none":
                assert want[5]["valued"] == 0 and (want[1][want[1] != pr.MISS] == pr.NONE).all()
            else:
                assert not pr.degenerate(want[1], v), (name, op, want[5])
            if name == "negative" and op == pr.MEAN:
                m = want[4] > 0
                assert ((want[3][m] % want[4][m] != 0) & (want[3][m] < 0)).sum() >= 20
                assert (want[1][m] == -((-want[3][m]) // want[4][m]) - ((-want[3][m]) % want[4][m] != 0)).all()
            if name == "adversarial" and op in (pr.MAX, pr.MIN):
                assert (want[1] == (2 ** 31 - 1 if op == pr.MAX else -2 ** 31 + 2)).sum() >= 20
            if name == "ridge" and op == pr.MAX:
                flat = vol.ravel()
                m = want[2] >= 0
                repeats = [(flat[[(z * 12 + y) * 40 + x for x, y, z in c]] == val).sum() for c, val in zip(cells, want[1].ravel()) if c]
                assert np.max(repeats) >= 3 and m.sum() >= 100
            for table in (True, False):
                ctx.debug_set_projection_table(table)
                for totals in (True, False):
                    _same(ctx.project_field_host(f, v, _lut(), vol, totals=totals), want, f"{name} op {op} table {table} totals {totals}")
    finally:
        ctx.debug_set_projection_table(True)


@gpu
@pytest.mark.parametrize("name", list(LONG))
def test_gpu_long_rows_equal_the_statement(ctx, orc, name):
    """Rows of more than 64 voxels, so that k_project_bricks runs a second, third and fourth wave along x, whole and partial, and
    the march reads their records: every output against the statement, with the brick table and without it, with the totals and
    without them.  A caller's volume valued only at x >= 64 (a missing or wrong record of a later run empties or dims the frame)
    under MAX, MIN, COUNT and FIRST, and the resident distance to EMPTY under MAX; the four cameras of _long_frames, whose
    statement frames test_long_row_frames_bite_and_feel_the_later_runs holds to their conditions."""
    hip = _hip()
    dx, dy, dz, (gmin, vox) = LONG[name]
    g = _long_grid(name)
    vol = _long_volume(name)
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g, gmin, vox)
    field = ctx.distance_field(hip.SET_EMPTY)[0]
    assert np.array_equal(field, dr.field(g, dr.SET_EMPTY))
    try:
        for cname, view, pos, rd, cells in _long_frames(orc, name):
            f = _frame(view, pos, LW, LH)
            assert sum(any(x >= 64 for x, _, _ in c) for c in cells) >= 50
            for v, volume, want in _long_runs(hip, cname, cells, vol, field):
                for table in (True, False):
                    ctx.debug_set_projection_table(table)
                    for totals in (True, False):
                        _same(ctx.project_field_host(f, v, _lut(), volume, totals=totals), want,
                              f"{name} {cname} source {v.source} op {v.op} table {table} totals {totals}")
    finally:
        ctx.debug_set_projection_table(True)


@gpu
def test_gpu_clip_boxes(ctx, orc):
    """The 32^3 grid's distance to EMPTY under boxes that cut a brick at offset 3, that are one voxel thick, that cover the whole
    grid (equal to no box, bit for bit) and that no ray meets (a frame of misses); MAX, COUNT and FIRST."""
    hip = _hip()
    g = _block32()
    code, vol = _make_fields(ctx, g, ("distance",))["distance"]
    W, H = 24, 16
    for op in (pr.MAX, pr.COUNT, pr.FIRST):
        kw = dict(valid=(1, 0x7ffffffe))
        for name, clip in (("offset 3 in a brick", ((11, 0, 3), (32, 27, 32))), ("one voxel thick", ((0, 0, 15), (32, 32, 16))),
                           ("one voxel wide", ((16, 0, 0), (17, 32, 32)))):
            v = _proj(hip, code, op, clip=clip, **kw)
            view, pos, cells = _walks(orc, "block32", "outside", W, H, v)
            want = pr.frame_of(cells, W, H, vol, v, _lut())
            assert want[5]["valued"] >= 20, (name, want[5])
            _same(ctx.project_field_host(_frame(view, pos, W, H), v, _lut(), totals=False), want, f"{name} op {op}")
        f = _frame(view, pos, W, H)
        plain = ctx.project_field_host(f, _proj(hip, code, op, **kw), _lut())
        whole = ctx.project_field_host(f, _proj(hip, code, op, clip=((0, 0, 0), (32, 32, 32)), **kw), _lut())
        assert plain[5]["valued"] >= 20
        _same(whole, plain, "a whole-grid box")
        high = [int(x) for x in ((pos - GMIN) / VOX > 16)]
        away = tuple(((0, 0, 0), (2, 2, 2)) if not high[0] else ((30, 30, 30), (32, 32, 32)))
        v = _proj(hip, code, op, clip=away, **kw)
        # the corner on the camera's side, seen from a camera that looks at the centre from close by: outside the frame
        cam = orc.Camera(0.6, 0.45, 0.3)
        cam.set_target(*[float(x) for x in _vpos(16, 16, 16)])
        nview, npos = cam.get_view(), cam.get_pos()
        ncells = pr.walks(GMIN, VOX, (32, 32, 32), npos, _rays(orc, nview, npos, W, H), v)
        if any(ncells):
            away = ((30, 30, 30), (32, 32, 32)) if not high[0] else ((0, 0, 0), (2, 2, 2))
            v = _proj(hip, code, op, clip=away, **kw)
            ncells = pr.walks(GMIN, VOX, (32, 32, 32), npos, _rays(orc, nview, npos, W, H), v)
        assert not any(ncells)
        got = ctx.project_field_host(_frame(nview, npos, W, H), v, _lut())
        _same(got, pr.frame_of(ncells, W, H, vol, v, _lut()), "a box no ray meets")
        assert (got[1] == hip.FIELD_PIXEL_MISS).all() and got[6].sum() == 0


@gpu
def test_gpu_orderings_between_the_ops(ctx, orc):
    """Without the statement, on the base grid's geodesic field: MAX >= MEAN >= MIN on every valued pixel, all three valued on the
    same pixels; COUNT under a window plus COUNT under its complement is COUNT of everything (NONE counting as 0); d_counts is
    COUNT's value; FIRST's voxel holds FIRST's value; the table off gives the same frames."""
    hip = _hip()
    g = _base()
    code, vol = _make_fields(ctx, g, ("geodesic",))["geodesic"]
    view, pos = _camera(orc, "outside", g)
    W, H = 72, 40
    f = _frame(view, pos, W, H)
    wide = (-2 ** 31 + 2, 2 ** 31 - 1)
    run = lambda op, valid, totals=True: ctx.project_field_host(f, _proj(hip, code, op, valid=valid), _lut(), totals=totals)
    mx, mn, mean, first = run(pr.MAX, (0, 0x7ffffffe)), run(pr.MIN, (0, 0x7ffffffe)), run(pr.MEAN, (0, 0x7ffffffe)), run(pr.FIRST, (0, 0x7ffffffe))
    valued = mx[1] > hip.FIELD_PIXEL_NONE
    assert valued.sum() >= 500 and ((mn[1] > hip.FIELD_PIXEL_NONE) == valued).all() and ((mean[1] > hip.FIELD_PIXEL_NONE) == valued).all()
    assert (mx[1][valued] >= mean[1][valued]).all() and (mean[1][valued] >= mn[1][valued]).all() and (mx[1][valued] > mn[1][valued]).any()
    assert (vol.ravel()[mx[2][valued]] == mx[1][valued]).all() and (vol.ravel()[first[2][valued]] == first[1][valued]).all()
    assert (mx[4][valued] * mn[1][valued].astype(np.int64) <= mx[3][valued]).all() and (mx[3][valued] <= mx[4][valued] * mx[1][valued].astype(np.int64)).all()
    cut = int(np.median(vol[(vol >= 0) & (vol < 0x7fffffff)]))
    count = lambda valid: np.where(run(pr.COUNT, valid)[1] > hip.FIELD_PIXEL_NONE, run(pr.COUNT, valid)[1], 0).astype(np.int64)
    below, above, everything = count((wide[0], cut)), count((cut + 1, wide[1])), count(wide)
    assert (below + above == everything).all() and (below > 0).sum() >= 100 and (above > 0).sum() >= 100
    c = run(pr.COUNT, wide)
    assert (np.where(c[1] > hip.FIELD_PIXEL_NONE, c[1], 0) == c[4]).all()
    try:
        ctx.debug_set_projection_table(False)
        for op, with_table in ((pr.MAX, mx), (pr.MIN, mn), (pr.MEAN, mean), (pr.FIRST, first)):
            _same(run(op, (0, 0x7ffffffe)), with_table, f"table off, op {op}")
            _same(run(op, (0, 0x7ffffffe), totals=False), with_table, f"table off, no totals, op {op}")
        ctx.debug_set_projection_table(True)
        for op, with_totals in ((pr.MAX, mx), (pr.MIN, mn), (pr.FIRST, first)):
            _same(run(op, (0, 0x7ffffffe), totals=False), with_totals, f"table on, no totals, op {op}")
    finally:
        ctx.debug_set_projection_table(True)


@gpu
def test_gpu_auto_range_and_the_device_form(ctx, orc):
    """Auto range is the frame of the explicit range (vmin, vmax), bit for bit; the device form on a caller's stream (with every
    optional output, and with none) is the host form; a caller's volume on the device; the kernels' times are reported."""
    torch = pytest.importorskip("torch")
    hip = _hip()
    g = _base()
    code, vol = _make_fields(ctx, g, ("distance",))["distance"]
    view, pos = _camera(orc, "outside", g)
    W, H = 72, 40
    f = _frame(view, pos, W, H)
    v = _proj(hip, code, pr.MAX, scale=hip.SCALE_SQRT, valid=(1, 0x7ffffffe))
    auto = ctx.project_field_host(f, v, _lut())
    s = auto[5]
    assert s["valued"] >= 20 and s["vmin"] < s["vmax"] and (s["lo"], s["hi"]) == (s["vmin"], s["vmax"])
    explicit = ctx.project_field_host(f, _proj(hip, code, pr.MAX, scale=hip.SCALE_SQRT, valid=(1, 0x7ffffffe), range=(int(s["vmin"]), int(s["vmax"]))), _lut())
    _same(explicit, auto, "explicit (vmin, vmax)")
    assert auto[6].sum() == s["valued"] and (auto[6] > 0).sum() >= 2
    ms = ctx.last_projection_ms()
    assert len(ms) == 3 and all(m > 0 for m in ms)
    other = torch.cuda.Stream()
    n = W * H
    d_lut = torch.from_numpy(_lut().view(np.int32)).cuda()
    d_rgba = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
    d_values, d_voxels, d_counts = (torch.full((n,), 7, dtype=torch.int32, device="cuda") for _ in range(3))
    d_sums = torch.full((n,), 7, dtype=torch.int64, device="cuda")
    d_summary = torch.zeros(4, dtype=torch.int64, device="cuda")
    d_bins = torch.full((256,), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.project_field_device(f, v, d_lut.data_ptr(), d_rgba.data_ptr(), 0, d_values.data_ptr(), d_voxels.data_ptr(), d_sums.data_ptr(),
                             d_counts.data_ptr(), d_summary.data_ptr(), d_bins.data_ptr(), other.cuda_stream)
    other.synchronize()
    got = (d_rgba.cpu().numpy().reshape(H, W, 4), d_values.cpu().numpy().reshape(H, W), d_voxels.cpu().numpy().reshape(H, W),
           d_sums.cpu().numpy().reshape(H, W), d_counts.cpu().numpy().reshape(H, W),
           d_summary.cpu().numpy().view(hip.FIELD_VIEW_SUMMARY_DTYPE)[0], d_bins.cpu().numpy())
    _same(got, auto, "the device form")
    d_rgba.zero_()
    torch.cuda.synchronize()
    ctx.project_field_device(f, v, d_lut.data_ptr(), d_rgba.data_ptr(), stream=other.cuda_stream)      # the context's own value buffer
    other.synchronize()
    assert d_rgba.cpu().numpy().tobytes() == auto[0].tobytes()
    d_vol = torch.from_numpy(vol).cuda()
    d_rgba.zero_()
    torch.cuda.synchronize()
    ctx.project_field_device(f, _proj(hip, hip.FIELD_CALLER, pr.MAX, scale=hip.SCALE_SQRT, valid=(1, 0x7ffffffe)), d_lut.data_ptr(),
                             d_rgba.data_ptr(), d_vol.data_ptr(), stream=other.cuda_stream)
    other.synchronize()
    assert d_rgba.cpu().numpy().tobytes() == auto[0].tobytes()


@gpu
def test_gpu_an_edit_drops_the_named_sources_and_keeps_the_caller(ctx, orc):
    """After an rto_edit_voxels with changed > 0 every named source is refused in its readers' words and nothing else on the
    context moved (a CALLER projection is the statement; the voxels are the edited grid); making a field again projects again."""
    hip = _hip()
    g = _base()
    fields = _make_fields(ctx, g)
    W, H = 24, 16
    view, pos, cells = _walks(orc, "base", "outside", W, H)
    f = _frame(view, pos, W, H)
    for name, (code, vol) in fields.items():
        v = _proj(hip, code, pr.MAX)
        _same(ctx.project_field_host(f, v, _lut()), pr.frame_of(cells, W, H, vol, v, _lut()), name)
    brush = hip.make_brushes([GMIN + np.float32(0.5) * VOX], 0.5 * float(VOX), hip.BRUSH_SPHERE, hip.EDIT_FILL)
    assert ctx.edit_voxels(brush) > 0
    edited = g.copy()
    edited[0, 0, 0] = 1
    for name, (code, _) in fields.items():
        with pytest.raises(hip.RtoError) as e:
            ctx.project_field_host(f, _proj(hip, code, pr.MAX), _lut())
        assert e.value.code == hip.RTO_E_INVALID and "the grid has changed since" in str(e.value), (name, str(e.value))
    assert np.array_equal(ctx.download_voxels(), edited)
    vol = np.arange(g.size, dtype=np.int32).reshape(g.shape)
    v = _proj(hip, hip.FIELD_CALLER, pr.MEAN)
    _same(ctx.project_field_host(f, v, _lut(), vol), pr.frame_of(cells, W, H, vol, v, _lut()), "CALLER after the edit")
    field = ctx.distance_field(hip.SET_EMPTY)[0]
    v = _proj(hip, hip.FIELD_DISTANCE, pr.MAX)
    after = ctx.project_field_host(f, v, _lut())
    assert after[5]["valued"] >= 20
    _same(after, pr.frame_of(cells, W, H, field, v, _lut()), "made again")


@gpu
def test_gpu_error_codes_in_the_header_s_order(ctx, orc, scenes):
    """Every refusal of the header.  Each call below is wrong in the way named and also in every way checked later, so the code
    and text it answers show the order: NULLs, alignment, source, op, scale, reserved, valid, range, frame size, frame limits,
    the volume's presence, (fresh context) no octree, no grid, the clip box, the source's residency.  A non-canonical array is
    no refusal of its own.  A refused call leaves the next frame unchanged."""
    torch = pytest.importorskip("torch")
    hip = _hip()
    g = _base()
    code, vol = _make_fields(ctx, g, ("thickness",))["thickness"]
    view, pos = _camera(orc, "outside", g)
    W, H = 24, 16
    f = _frame(view, pos, W, H)
    lut = _lut()
    ref = ctx.project_field_host(f, _proj(hip, code, pr.MAX), lut)
    Lib = ctx._L
    out = np.zeros((H, W, 4), np.float32)

    def call(proj, frame=f, lut_=lut, buf=out, volume=None, c=ctx):
        rc = Lib.rto_project_field_host(c._h, C.byref(frame) if frame is not None else None, C.byref(proj) if proj is not None else None,
                                        lut_.ctypes.data if lut_ is not None else None, volume.ctypes.data if volume is not None else None,
                                        buf.ctypes.data if buf is not None else None, None, None, None, None, None, None)
        return rc, Lib.rto_last_error(c._h).decode()

    def worst():
        """A projection wrong in every way one can be, on a source that is not resident."""
        v = hip.make_field_projection(hip.FIELD_GEODESIC, op=7, scale=9, valid=(3, 2), range=(5, 1), clip=((0, 0, 0), (41, 12, 12)))
        v.reserved[4] = 1
        return v

    big = hip.make_frame(view, pos, 1.0, FOV, 65536, 65536)
    flat = hip.make_frame(view, pos, 1.0, FOV, 0, 16)
    assert call(_proj(hip, code, pr.MAX))[0] == hip.RTO_OK
    for kw in (dict(frame=None), dict(lut_=None), dict(buf=None)):
        rc, msg = call(worst(), volume=vol, **kw)
        assert rc == hip.RTO_E_INVALID and "NULL" in msg, kw
    assert call(None)[0] == hip.RTO_E_INVALID
    v = worst()
    steps = [("source", lambda: setattr(v, "source", 8), "unknown source"), ("source", lambda: setattr(v, "source", -1), "unknown source"),
             ("op", lambda: setattr(v, "source", hip.FIELD_GEODESIC), "unknown op"), ("op", lambda: setattr(v, "op", -1), "unknown op"),
             ("scale", lambda: setattr(v, "op", 4), "unknown scale"),
             ("reserved", lambda: setattr(v, "scale", 2), "reserved"), ("valid", lambda: v.reserved.__setitem__(4, 0), "valid_lo"),
             ("valid", lambda: (setattr(v, "valid_lo", -2 ** 31 + 1), setattr(v, "valid_hi", 5)), "valid_lo"),
             ("range", lambda: setattr(v, "valid_lo", -2 ** 31 + 2), "range_lo > range_hi")]
    for what, fix, text in steps:
        fix()
        rc, msg = call(v, frame=big, volume=vol)
        assert rc == hip.RTO_E_INVALID and text in msg, (what, msg)
    v.range_lo = 1
    rc, msg = call(v, frame=flat, volume=vol)
    assert rc == hip.RTO_E_INVALID and "width/height" in msg
    rc, msg = call(v, frame=big, volume=vol)
    assert rc == hip.RTO_E_INVALID and "too large" in msg
    rc, msg = call(v, volume=vol)
    assert rc == hip.RTO_E_INVALID and "RTO_FIELD_CALLER only" in msg
    v.source = hip.FIELD_CALLER
    rc, msg = call(v)
    assert rc == hip.RTO_E_INVALID and "needs a volume" in msg
    fresh = hip.Context(0)
    try:
        v.source = hip.FIELD_GEODESIC
        assert call(v, c=fresh)[0] == hip.RTO_E_NO_OCTREE
        s = scenes("sphere16")
        fresh.upload_octree(s.nodes, GMIN, VOX)
        rc, msg = call(v, c=fresh)
        assert rc == hip.RTO_E_UNSUPPORTED and "no voxel grid is resident" in msg
    finally:
        fresh.close()
    rc, msg = call(v)
    assert rc == hip.RTO_E_INVALID and "clip box" in msg                      # clip_hi[0] = 41 > 40, on a source that is not resident
    for lo_, hi_ in (((-1, 0, 0), (40, 12, 12)), ((5, 0, 0), (5, 12, 12)), ((0, 0, 7), (40, 12, 6)), ((0, 0, 0), (40, 13, 12))):
        for a in range(3):
            v.clip_lo[a], v.clip_hi[a] = lo_[a], hi_[a]
        rc, msg = call(v)
        assert rc == hip.RTO_E_INVALID and "clip box" in msg, (lo_, hi_)
    for a, d in enumerate((40, 12, 12)):
        v.clip_lo[a], v.clip_hi[a] = 0, d
    rc, msg = call(v)
    assert rc == hip.RTO_E_INVALID and "no geodesic field is resident" in msg and "the grid has changed since" in msg
    v.source = hip.FIELD_LABELS
    rc, msg = call(v)
    assert rc == hip.RTO_E_INVALID and "no labels are resident" in msg and "the grid has changed since" in msg
    v.source = code
    assert call(v)[0] == hip.RTO_OK
    # the device form's alignment, behind the NULLs and in front of everything else
    dev = Lib.rto_project_field_device
    d = torch.zeros(W * H * 4 + 64, dtype=torch.float32, device="cuda")
    d_lut = torch.from_numpy(lut.view(np.int32)).cuda()
    p0 = d.data_ptr()
    P = lambda x: C.c_void_p(x) if x else None

    def devcall(proj, lut_=d_lut.data_ptr(), volume=0, rgba=p0, values=0, voxels=0, sums=0, counts=0, summary=0, bins=0):
        return dev(ctx._h, C.byref(f), C.byref(proj), P(lut_), P(volume), P(rgba), P(values), P(voxels), P(sums), P(counts), P(summary),
                   P(bins), None), Lib.rto_last_error(ctx._h).decode()

    bad = worst()
    for kw in (dict(rgba=p0 + 4), dict(lut_=p0 + 2), dict(volume=p0 + 2), dict(values=p0 + 2), dict(voxels=p0 + 2), dict(sums=p0 + 4),
               dict(counts=p0 + 2), dict(summary=p0 + 4), dict(bins=p0 + 4)):
        rc, msg = devcall(bad, **kw)
        assert rc == hip.RTO_E_INVALID and "aligned" in msg, kw
    rc, msg = devcall(bad, rgba=0)
    assert rc == hip.RTO_E_INVALID and "NULL" in msg
    rc, msg = devcall(bad)
    assert rc == hip.RTO_E_INVALID and "unknown op" in msg
    torch.cuda.synchronize()
    _same(ctx.project_field_host(f, _proj(hip, code, pr.MAX), lut), ref, "after the refusals")


@gpu
def test_gpu_sphere_maximum_without_the_statement(ctx, orc, scenes):
    """sphere64 at 256 x 144, MAX of the distance to EMPTY: every valued pixel's d_voxels holds the pixel's value in the
    downloaded field; no pixel exceeds rto_distance_field's reported maximum and some pixel reaches it; sums and counts bound
    the value; without the table, and without the totals, the same frame."""
    hip = _hip()
    s = scenes("sphere64")
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(s.grid.data, s.min, s.voxel)
    field, summary = ctx.distance_field(hip.SET_EMPTY)
    view, pos = make_camera(orc, *SPHERE_CAM)
    W, H = 256, 144
    f = hip.make_frame(view, pos, W / H, FOV, W, H)
    v = hip.make_field_projection(hip.FIELD_DISTANCE, hip.PROJECT_MAX, scale=hip.SCALE_SQRT, valid=(1, 0x7ffffffe))
    got = ctx.project_field_host(f, v, _lut())
    rgba, values, voxels, sums, counts, fs, bins = got
    valued = values > hip.FIELD_PIXEL_NONE
    assert valued.sum() > 3000 and fs["valued"] == valued.sum() == bins.sum() and (voxels[~valued] == -1).all()
    assert (field.ravel()[voxels[valued]] == values[valued]).all()
    assert values[valued].max() <= int(summary["max_d2"]) and fs["vmax"] == values[valued].max()
    assert (counts[valued] >= 1).all() and (sums[valued] <= counts[valued].astype(np.int64) * values[valued]).all()
    assert (values != hip.FIELD_PIXEL_MISS).sum() == fs["hits"] > valued.sum()
    _same(ctx.project_field_host(f, v, _lut(), totals=False), got, "without the totals")
    try:
        ctx.debug_set_projection_table(False)
        _same(ctx.project_field_host(f, v, _lut()), got, "without the table")
    finally:
        ctx.debug_set_projection_table(True)


@gpu
def test_gpu_drop_in_project_field(orc):
    """RayTracerBVH::projectField through host.py: framebuffer(), projectionValues() and fieldSummary() are the C ABI's frame."""
    import ray_tracing_octrees_amd as rto
    hip = _hip()
    grid = rto.VoxelGrid.test_sphere(32)
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    rt.setOctreeFromGrid(grid)
    cam = rto.Camera(*SPHERE_CAM)
    W, H = 96, 72
    v = hip.make_field_projection(hip.FIELD_DISTANCE, hip.PROJECT_MAX, scale=hip.SCALE_SQRT, valid=(1, 0x7ffffffe))
    assert rt.projectField(cam, W, H, W / H, FOV, v, _lut()) == hip.RTO_E_INVALID and "the grid has changed since" in rt.lastError
    assert rt.distanceField(hip.SET_EMPTY)[0] == hip.RTO_OK
    assert rt.projectField(cam, W, H, W / H, FOV, v, _lut()) == hip.RTO_OK
    img, (values, voxels, sums, counts), summary = rt.framebuffer(), rt.projectionValues(), rt.fieldSummary()
    og = orc.test_sphere_grid(32)
    ctx = rto.Context(0)
    try:
        ctx.build_octree(og.data, og.min, og.voxel_size)
        ctx.distance_field(hip.SET_EMPTY)
        f = rto.make_frame(cam.getView(), cam.getPos(), W / H, FOV, W, H)
        want = ctx.project_field_host(f, v, _lut())
    finally:
        ctx.close()
    assert want[5]["valued"] > 500
    _same((img, values, voxels, sums, counts, summary, None), want[:6] + (None,), "the drop-in class")
