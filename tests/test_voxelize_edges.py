"""Mesh voxelization at the sizes and edges where its kernels branch (tests/voxelize_families.py): the scan's
carry between chunks of 1024 block sums, pair spans on k_vox_fill's run and block boundaries, long runs of faces without voxels,
boxes clipped by the truncating casts at the grid's low side, one face of more than 2^31 pairs on a grid of more than 2^31
voxels, the refusal above 2^43 pairs, the AUTO rescale's edges, the FIXED per-axis limit and empty results.
CPU: the oracle's C statement of the fill (orc_voxelize_fill) equals the numpy rule (tests/voxelize_ref.py) on every golden and
every family numpy can afford, and the families reach the edges they are named for.  GPU: rto_voxelize_mesh equals the C
statement bit for bit, the context equals rto_build_octree of the expected grid, recentring equals the rule, and the refusals
leave the context as it was.  RTO_VOX_SEEDS=n runs n seeds of the randomised families (default 1)."""
from __future__ import annotations

import os

import numpy as np
import pytest

import test_mesh_voxelize as tmv
import voxelize_families as vf
import voxelize_ref as vr

SEEDS = range(int(os.environ.get("RTO_VOX_SEEDS", "1")))


def _orc():
    from oracle import orc
    return orc


def _grid_of(case):
    """(dims, grid_min, voxel_size) the library voxelizes into."""
    if case.grid is None:
        return vr.auto_grid(case.xyz, len(case.tris), case.voxel)
    return case.grid


FAMILIES = {
    "many_small": vf.many_small,
    "below_low": vf.below_low,
    "fixed_limit": vf.fixed_limit,
    **{f"boundaries_{s}": (lambda s=s: vf.boundaries(seed=2 + 100 * s)) for s in SEEDS},
    **{f"below_low_{s}": (lambda s=s: vf.below_low(seed=3 + 100 * s)) for s in SEEDS if s},
    **{f"auto_{d}": (lambda d=d: vf.auto_edges(d)) for d in vf.AUTO_EDGE_DIMS},
    **{f"empty_{k}": f for k, f in vf.EMPTY.items()},
}
_cache = {}


def family(name):
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
    return _cache[name]


# ================================================================ CPU
@pytest.mark.parametrize("name", tmv.NAMES)
def test_statement_equals_rule_on_every_golden(name):
    g = tmv.G[name]
    want, pairs = vr.fill(g["xyz"], g["tris"], g["min"], g["vs"], g["dims"])
    got, p, bad = _orc().voxelize_fill(g["xyz"], g["tris"], g["dims"], g["min"], g["vs"])
    assert not bad and p == pairs and np.array_equal(got, want), name
    assert np.array_equal(got, g["grid"]), name


def test_statement_flags_the_overflowing_box():
    """A FIXED grid 10^12 voxel sizes away: the rule refuses the mesh, the statement raises its flag and fills nothing."""
    g = tmv.G["utm_blocks_10"]
    gmin = (g["xyz"].min(0) - 1e12).astype(np.float32)
    with pytest.raises(ValueError):
        vr.fill(g["xyz"], g["tris"], gmin, 1.0, (64, 64, 64))
    got, _, bad = _orc().voxelize_fill(g["xyz"], g["tris"], (64, 64, 64), gmin, 1.0)
    assert bad and not got.any()


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_statement_equals_rule_on_every_family(name):
    c = family(name)
    dims, gmin, vs = _grid_of(c)
    want, pairs = vr.fill(c.xyz, c.tris, gmin, vs, dims)
    got, p, bad = _orc().voxelize_fill(c.xyz, c.tris, dims, gmin, vs)
    assert not bad and p == pairs, (name, p, pairs)
    assert np.array_equal(got, want), name


def _counts(c):
    dims, gmin, vs = _grid_of(c)
    return vr.face_terms(c.xyz, c.tris, gmin, vs, dims)["n"].prod(axis=1)


def test_many_small_carries_between_scan_chunks():
    c = family("many_small")
    cnt = _counts(c)
    blocks = -(-len(cnt) // 256)                                   # k_vox_setup blocks: one block sum each
    assert blocks > 2 * 1024                                       # three rounds of k_scan_counts: the carry runs twice
    assert not cnt[:5000].any() and not cnt[-5000:].any()          # runs without voxels at both ends
    assert (cnt == 0).sum() > 50_000
    chunk = 1024 * 256                                             # faces behind one chunk of block sums
    assert cnt[chunk:2 * chunk].sum() > 0 and cnt[2 * chunk:].sum() > 0


def test_boundaries_sit_on_runs_and_blocks():
    c = family("boundaries_0")
    cnt = _counts(c)
    assert np.array_equal(cnt, vf.boundary_counts())
    end = np.cumsum(cnt)
    start = end - cnt
    full = cnt > 0
    for m in (16, 4096):
        assert ((start[full] % m) == 0).sum() >= 20 and ((end[full] % m) == 0).sum() >= 20, m
        assert ((start[~full] % m) == 0).sum() >= 20, m            # empty faces exactly on a boundary
    assert cnt[0] == 0 and cnt[-1] == 0
    for k in (1, 4095, 4096, 4097):
        assert (cnt == k).sum() >= 3, k
    assert (cnt > 3 * 4096).any()


def test_below_low_fills_through_the_truncating_cast():
    """Faces whose box reaches voxel 0 or 1 only because (int) truncates toward zero fill voxels there: floor would not."""
    c = family("below_low")
    dims, gmin, vs = c.grid
    v = c.xyz[c.tris].astype(np.float32)
    te = (v.max(axis=1) - gmin) / vs
    for a in range(3):
        for lo, hi, layer in ((-1.0, 0.0, 1), (-2.0, -1.0, 0)):
            sel = (te[:, a] > lo) & (te[:, a] < hi)
            assert sel.sum() > 50, (a, lo)
            g, _ = vr.fill(c.xyz, c.tris[sel], gmin, vs, dims)
            assert np.take(g, layer, axis=2 - a).any(), (a, lo)
    hi_side = (te >= np.asarray(dims)).any(axis=1) & (_counts(c) > 0)
    assert hi_side.sum() > 50                                      # boxes clipped at the high side that still hold voxels


@pytest.mark.parametrize("dim", vf.AUTO_EDGE_DIMS)
def test_auto_edges_give_their_dim_before_the_rescale(dim):
    c = family(f"auto_{dim}")
    fin = np.isfinite(c.xyz).all(axis=1)
    vs = float(c.voxel)
    pre = int(np.ceil(((c.xyz[fin].max(0)[0] + vs) - (c.xyz[fin].min(0)[0] - vs)) / vs))
    assert pre == dim
    dims, _, v = _grid_of(c)
    scale = max(1, dim // 1000)                                    # integer division: 1001..1999 keep scale 1
    assert v == np.float32(scale) and dims[0] == int(np.ceil((dim - 0.5) / scale))
    assert (~fin).sum() >= 2 and (_counts(c) == 0).sum() >= 18      # NaN rows, degenerate faces and faces on NaN rows


def test_huge_face_passes_2_31_pairs_and_voxels():
    c = vf.huge_face()
    dims, gmin, vs = c.grid
    T = vr.face_terms(c.xyz, c.tris, gmin, vs, dims)
    assert int(T["n"].prod()) == dims[0] * dims[1] * dims[2] > 2 ** 31
    _, pairs, bad = _orc().voxelize_fill(c.xyz, c.tris, dims, gmin, vs, grid=False)
    assert pairs == dims[0] * dims[1] * dims[2] and not bad
    r = vf.huge_refused()
    _, pairs, bad = _orc().voxelize_fill(r.xyz, r.tris, dims, gmin, vs, grid=False)
    assert pairs == 4096 * dims[0] * dims[1] * dims[2] and -(-pairs // 4096) > 0x7fffffff and not bad


# ================================================================ GPU
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx2():
    from ray_tracing_octrees_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def _check(r, dims, gmin, vs, want, pairs):
    assert tuple(r.dims) == tuple(dims)
    assert tmv._bits(list(r.grid_min)) == tmv._bits(gmin) and tmv._bits(r.voxel_size) == tmv._bits(vs)
    assert r.filled == int(np.count_nonzero(want)) and r.pairs == pairs


@gpu
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_gpu_family_equals_statement(ctx, ctx2, name):
    from ray_tracing_octrees_amd import hip
    c = family(name)
    dims, gmin, vs = _grid_of(c)
    want, pairs, bad = _orc().voxelize_fill(c.xyz, c.tris, dims, gmin, vs)
    assert not bad
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx2.set_kernel(hip.KERNEL_AUTO)
    r = ctx.voxelize_mesh(c.xyz, c.tris, c.voxel, grid=c.grid)
    _check(r, dims, gmin, vs, want, pairs)
    assert np.array_equal(ctx.download_voxels(), want), name
    tmv._same_context(ctx, ctx2, want, gmin, vs, name)
    if name == "fixed_limit":
        assert ctx.info().depth == 20
    for passes in (1, 2):
        r = ctx.voxelize_mesh(c.xyz, c.tris, c.voxel, grid=c.grid, recenter=passes)
        m = vr.recenter(want, gmin, vs, passes)
        if not want.any():
            assert tmv._bits(m) == tmv._bits(gmin)
        _check(r, dims, m, vs, want, pairs)
        tmv._same_context(ctx, ctx2, want, m, vs, f"{name} recentred {passes}x")


def _snapshot(ctx):
    from ray_tracing_octrees_amd import hip
    f = hip.make_frame(np.eye(4, dtype=np.float32), [0, 0, 0], tmv.W / tmv.H, tmv.FOV, tmv.W, tmv.H)
    return ctx.download_nodes().tobytes(), ctx.download_voxels().tobytes(), bytes(ctx.info()), ctx.render_host(f).tobytes()


def _refused(ctx, c, code):
    from ray_tracing_octrees_amd import hip
    g = tmv.G["utm_blocks_10"]
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.voxelize_mesh(g["xyz"], g["tris"], g["voxel"])
    before = _snapshot(ctx)
    with pytest.raises(hip.RtoError) as e:
        ctx.voxelize_mesh(c.xyz, c.tris, c.voxel, grid=c.grid)
    assert e.value.code == code, e.value
    assert _snapshot(ctx) == before


@gpu
def test_gpu_fixed_limit_plus_one_is_refused(ctx):
    from ray_tracing_octrees_amd import hip
    _refused(ctx, vf.fixed_limit(extra=1), hip.RTO_E_INVALID)


@gpu
def test_gpu_pairs_above_2_43_are_refused(ctx):
    from ray_tracing_octrees_amd import hip
    _refused(ctx, vf.huge_refused(), hip.RTO_E_UNSUPPORTED)


@gpu
def test_gpu_huge_face_above_2_31(ctx, ctx2):
    """One face of 2^31 + 2^21 pairs on a grid of as many voxels: filled voxels past flat index 2^31, a second context of the
    same size, recentring from that box."""
    from ray_tracing_octrees_amd import hip
    c = vf.huge_face()
    dims, gmin, vs = c.grid
    want, pairs, bad = _orc().voxelize_fill(c.xyz, c.tris, dims, gmin, vs)
    assert not bad and want[dims[2] - 1].any()                     # voxels in the last layer: flat index above 2^31
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx2.set_kernel(hip.KERNEL_AUTO)
    r = ctx.voxelize_mesh(c.xyz, c.tris, c.voxel, grid=c.grid, recenter=2)
    m = vr.recenter(want, gmin, vs, 2)
    _check(r, dims, m, vs, want, pairs)
    got = ctx.download_voxels()
    assert np.array_equal(got, want)
    del got
    tmv._same_context(ctx, ctx2, want, m, vs, "huge face recentred 2x")
    r = ctx.voxelize_mesh(c.xyz, c.tris, c.voxel, grid=c.grid, recenter=1)
    _check(r, dims, vr.recenter(want, gmin, vs, 1), vs, want, pairs)
    ctx2.build_octree(np.zeros((1, 1, 1), np.uint8), (0, 0, 0), 1.0)   # give the second grid's memory back
