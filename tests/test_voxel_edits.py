"""Voxel edits (rto_edit_voxels, rto_download_voxels, rto_last_edit_ms, rto_brush_quantize, Context.edit_voxels,
RayTracerBVH::editVoxels / grid): brushes carve or fill the resident grid, then the octree is rebuilt on the GPU.  CPU: the numpy
rule (tests/edit_ref.py) on hand-made cases, the host quantisation against it, the ABI and the edit kernels' budget.  GPU: the
edited grid and changed count against the rule; the rebuilt octree, info and scene bounds against a fresh build of the edited
grid on both build paths; renders, triangles and pixel picks against the oracle and tests/query_ref.py."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import edit_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDIT_VGPR_BUDGET = 96       # 5 waves per SIMD or more; the kernels are memory- and brush-loop bound
SYMS = ("rto_edit_voxels", "rto_download_voxels", "rto_last_edit_ms", "rto_brush_quantize")


def _hip():
    from ray_tracing_octrees_amd import hip
    return hip


def _brush(centre, extent, shape=er.SPHERE, op=er.CARVE):
    return _hip().make_brushes([centre], [extent] if np.ndim(extent) == 1 else extent, shape, op)


def _world(gmin, voxel, ijk):
    """World position of a point given in voxel units (float32, as a caller would pass it)."""
    return (np.asarray(gmin, np.float64) + np.asarray(ijk, np.float64) * float(voxel)).astype(np.float32)


# ================================================================ CPU: the rule
GMIN, VOX = np.array([-0.5, -0.5, -0.5], np.float32), np.float32(1.0 / 64)


def _covered(dims, centre_vox, extent_vox, shape):
    g = np.zeros(dims[::-1], np.uint8)
    b = _brush(_world(GMIN, VOX, centre_vox), np.float32(np.asarray(extent_vox, np.float64) * float(VOX)), shape, er.FILL)
    out, changed = er.apply(g, b, GMIN, VOX)
    return set(map(tuple, np.argwhere(out == 1)[:, ::-1])), changed


def test_rule_half_voxel_sphere_on_a_centre_covers_that_voxel():
    got, changed = _covered((8, 8, 8), (3.5, 4.5, 2.5), 0.5, er.SPHERE)
    assert got == {(3, 4, 2)} and changed == 1


def test_rule_ties_on_the_boundary_are_inclusive():
    got, _ = _covered((8, 8, 8), (3.5, 3.5, 3.5), 1.0, er.SPHERE)      # the six face neighbours lie exactly on the sphere
    assert got == {(3, 3, 3), (2, 3, 3), (4, 3, 3), (3, 2, 3), (3, 4, 3), (3, 3, 2), (3, 3, 4)}
    got, _ = _covered((8, 8, 8), (3.5, 3.5, 3.5), 1.0, er.BOX)         # |D| == 2 eq on every axis: the 3x3x3 block
    assert got == {(x, y, z) for x in (2, 3, 4) for y in (2, 3, 4) for z in (2, 3, 4)}


def test_rule_centre_on_a_voxel_corner():
    # the 8 voxels around the corner are sqrt(3)/2 = 0.866 voxel away: 0.87 quantises to 56/64 (112^2 >= 3 * 64^2), 0.86 to 55/64
    got, _ = _covered((8, 8, 8), (4.0, 4.0, 4.0), 0.87, er.SPHERE)
    assert got == {(x, y, z) for x in (3, 4) for y in (3, 4) for z in (3, 4)}
    got, _ = _covered((8, 8, 8), (4.0, 4.0, 4.0), 0.86, er.SPHERE)
    assert got == set()
    got, _ = _covered((8, 8, 8), (4.0, 4.0, 4.0), (0.5, 0.5, 0.5), er.BOX)
    assert got == {(x, y, z) for x in (3, 4) for y in (3, 4) for z in (3, 4)}


def test_rule_quantisation_rounds_halves_up():
    h = 1.0 / 128                                                   # half a 1/64 step, in voxels
    for off, want in ((h, 1), (-h, 0), (3 * h, 2), (-3 * h, -1)):
        cq, eq = er.quantize(_world(GMIN, VOX, (off, 0, 0)), (max(off, 0) * float(VOX), 0, 0), er.SPHERE, er.CARVE, GMIN, VOX)
        assert cq[0] == want, (off, cq)
        if off > 0:
            assert eq[0] == want
    cq, eq = er.quantize(GMIN, (float(VOX) / 2, 0, 0), er.BOX, er.FILL, GMIN, VOX)
    assert list(cq) == [0, 0, 0] and list(eq) == [32, 0, 0]


def test_rule_boxes_partly_and_wholly_outside():
    dims = (10, 6, 4)
    got, changed = _covered(dims, (9.5, 2.5, 1.5), (2.0, 0.5, 0.5), er.BOX)        # centres 7.5 .. 11.5, inclusive: 7, 8, 9 (10, 11 do not exist)
    assert got == {(7, 2, 1), (8, 2, 1), (9, 2, 1)} and changed == 3
    got, changed = _covered(dims, (-3.5, 2.5, 1.5), (2.0, 40.0, 40.0), er.BOX)       # x -5.5 .. -1.5: nothing
    assert got == set() and changed == 0
    got, changed = _covered(dims, (5.0, 3.0, 2.0), (100.0, 100.0, 100.0), er.BOX)    # everything
    assert len(got) == changed == 10 * 6 * 4


def test_rule_order_later_brush_wins_and_changed_is_net():
    g = np.zeros((4, 4, 4), np.uint8)
    hip = _hip()
    c = _world(GMIN, VOX, (2.0, 2.0, 2.0))
    b = np.concatenate([_brush(c, np.float32(VOX), er.BOX, er.FILL), _brush(c, np.float32(VOX), er.BOX, er.CARVE)])
    out, changed = er.apply(g, b, GMIN, VOX)
    assert changed == 0 and not out.any()
    out, changed = er.apply(g, b[::-1].copy(), GMIN, VOX)
    assert changed == 8 and out.sum() == 8
    assert b.dtype == hip.BRUSH_DTYPE


def test_rule_range_limits():
    L = 1 << 27                                                     # inputs are float32: one voxel past the limit is 64 steps
    ok = er.quantize((L / 64.0, 0, 0), (L / 64.0, 0, 0), er.SPHERE, er.CARVE, (0, 0, 0), 1.0)
    assert ok is not None and ok[0][0] == L and ok[1][0] == L
    assert er.quantize(((L + 64) / 64.0, 0, 0), (0, 0, 0), er.SPHERE, er.CARVE, (0, 0, 0), 1.0) is None
    assert er.quantize((-(L + 64) / 64.0, 0, 0), (0, 0, 0), er.SPHERE, er.CARVE, (0, 0, 0), 1.0) is None
    assert er.quantize((0, 0, 0), (0, (L + 64) / 64.0, 0), er.BOX, er.CARVE, (0, 0, 0), 1.0) is None
    for bad in ((np.nan, 0, 0), (np.inf, 0, 0)):
        assert er.quantize(bad, (1, 1, 1), er.SPHERE, er.CARVE, (0, 0, 0), 1.0) is None
        assert er.quantize((0, 0, 0), bad, er.SPHERE, er.CARVE, (0, 0, 0), 1.0) is None
    assert er.quantize((0, 0, 0), (1, -1, 1), er.BOX, er.CARVE, (0, 0, 0), 1.0) is None
    assert er.quantize((0, 0, 0), (1, 1, 1), 2, er.CARVE, (0, 0, 0), 1.0) is None
    assert er.quantize((0, 0, 0), (1, 1, 1), er.BOX, 2, (0, 0, 0), 1.0) is None


def _seeded_brushes(rng, n, gmin, voxel, dims, spread=1.2, max_r=None):
    dims = np.asarray(dims, np.float64)
    lo, hi = -0.5 * (spread - 1) * dims, dims * (1 + 0.5 * (spread - 1))
    centres = _world(gmin, voxel, rng.uniform(lo, hi, (n, 3)))
    max_r = max_r if max_r is not None else max(2.0, dims.max() / 6)
    ext = (rng.uniform(0.3, max_r, (n, 3)) * float(voxel)).astype(np.float32)
    return _hip().make_brushes(centres, ext, rng.integers(0, 2, n), rng.integers(0, 2, n))


def test_host_quantisation_equals_the_rule():
    """rto_brush_quantize (C++, no device) == the numpy quantisation, including exact halves of a 1/64 step and refusals."""
    hip = _hip()
    rng = np.random.default_rng(11)
    grids = [((-0.5, -0.5, -0.5), 1.0 / 64), ((-2125.0, -1215.0, -150.0), 10.0), ((0.1, -3.3, 7.7), 0.37), ((0.0, 0.0, 0.0), 1.0)]
    n = 0
    for gmin, vox in grids:
        gmin = np.asarray(gmin, np.float32)
        vox = np.float32(vox)
        b = _seeded_brushes(rng, 300, gmin, vox, (300, 200, 100))
        halves = np.float32(gmin[0]) + (np.arange(-40, 40) + 0.5).astype(np.float32) * np.float32(vox) / np.float32(64)
        hb = hip.make_brushes(np.stack([halves, halves, halves], 1), np.abs(halves - gmin[0]), er.BOX, er.FILL)
        specials = hip.make_brushes([[0, 0, 0]] * 4, [[np.nan, 1, 1], [1, -1, 1], [1, 1, np.inf], [1e30, 1, 1]], er.BOX, er.CARVE)
        for rec in np.concatenate([b, hb, specials]):
            want = er.quantize(rec["centre"], rec["extent"], int(rec["shape"]), int(rec["op"]), gmin, vox)
            try:
                got = hip.brush_quantize(rec, gmin, vox)
            except hip.RtoError as e:
                assert e.code == hip.RTO_E_INVALID
                got = None
            if want is None:
                assert got is None, rec
            else:
                assert got is not None and tuple(want[0]) == got[0] and tuple(want[1]) == got[1], (rec, want, got)
                n += 1
    assert n > 1000


def test_brush_abi_layout_and_exports():
    """sizeof(rto_brush) == 32 with the fields where BRUSH_DTYPE and the ctypes mirror put them; the new symbols are exported."""
    hip = _hip()
    assert C.sizeof(hip.Brush) == 32 and hip.BRUSH_DTYPE.itemsize == 32
    assert [hip.BRUSH_DTYPE.fields[f][1] for f in ("centre", "extent", "shape", "op")] == [0, 12, 24, 28]
    assert [getattr(hip.Brush, f).offset for f in ("centre", "extent", "shape", "op")] == [0, 12, 24, 28]
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.fail("no C compiler: the header's layout cannot be checked")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "abi.c")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "rto_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d %d %d %d %d\\n", '
                    'sizeof(rto_brush), offsetof(rto_brush, centre), offsetof(rto_brush, extent), offsetof(rto_brush, shape), '
                    'offsetof(rto_brush, op), RTO_BRUSH_SPHERE, RTO_BRUSH_BOX, RTO_EDIT_CARVE, RTO_EDIT_FILL, RTO_EDIT_MAX_BRUSHES); return 0; }\n')
        exe = os.path.join(tmp, "abi")
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["32", "0", "12", "24", "28", str(hip.BRUSH_SPHERE), str(hip.BRUSH_BOX), str(hip.EDIT_CARVE), str(hip.EDIT_FILL),
                   str(hip.EDIT_MAX_BRUSHES)]
    L = hip.load()
    for s in SYMS:
        assert s in hip.SYMBOLS and hasattr(L, s), s
    header = open(os.path.join(ROOT, "include", "rto_hip.h")).read()
    for s in SYMS:
        assert s + "(" in header, s


def test_edit_kernels_keep_their_budgets():
    """The built assembly (the product's flags): both k_edit_brushes forms without scratch, spills or v_mfma, within the VGPR budget;
    the 16-byte form moves rows with dwordx4 loads and stores."""
    import test_isa_contract as isa
    asm = isa.built_asm()
    if asm is None:
        pytest.fail("no hipcc: the budget cannot be checked")
    meta = isa.kernel_meta(asm)
    names = [k for k in meta if "k_edit_brushes" in k]
    assert len(names) == 2, names
    for k in names:
        m = meta[k]
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (k, m)
        assert m["vgpr"] <= EDIT_VGPR_BUDGET, (k, m)
        ins = isa.body(asm, k[len("_ZN3rto"):])
        assert not any(t.startswith(("scratch_", "buffer_load", "buffer_store")) or "v_mfma" in t for t in ins), k
        if "ILb1E" in k:
            assert any(t.startswith("global_load_dwordx4") for t in ins) and any(t.startswith("global_store_dwordx4") for t in ins), k


# ================================================================ GPU
gpu = pytest.mark.gpu
W, H, FOV = 128, 96, 45.0


@pytest.fixture(scope="module")
def ctx2():
    """A second context: the fresh build of the edited grid that the edited context must equal."""
    from ray_tracing_octrees_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(params=["morton", "level_by_level"])
def path(request, ctx, ctx2):
    for c in (ctx, ctx2):
        c.debug_set_build_path(request.param == "level_by_level")
    yield request.param
    for c in (ctx, ctx2):
        c.debug_set_build_path(False)


def _odd_grid(orc, dims=(37, 53, 29), radii=(15.0, 22.0, 12.0)):
    rng = np.random.default_rng(5)
    z, y, x = np.mgrid[0:dims[2], 0:dims[1], 0:dims[0]]
    blob = ((x - dims[0] // 2) ** 2 / radii[0] ** 2 + (y - dims[1] // 2) ** 2 / radii[1] ** 2 + (z - dims[2] // 2) ** 2 / radii[2] ** 2) <= 1.0
    data = (blob & (rng.random(blob.shape) < 0.97)).astype(np.uint8)
    vox = np.float32(1.0 / 64)
    gmin = (-0.5 * np.asarray(dims, np.float32) * vox).astype(np.float32)
    return orc.Grid(dims, gmin, vox, data)


def _grid(orc, scenes, name):
    return _odd_grid(orc) if name == "odd37" else scenes(name).grid


def _view(orc, camera, name):
    from conftest import make_camera
    return camera("calgary_oblique") if name == "calgary" else make_camera(orc, 0.5, 0.7, 1.8)


def _same_struct(a, b):
    return bytes(a) == bytes(b)


def _check_rebuilt(ctx, ctx2, orc, g, edited, what):
    """ctx (edited) holds what a fresh rto_build_octree of `edited` leaves: voxels, nodes (== the oracle's), info, scene bounds."""
    assert np.array_equal(ctx.download_voxels(), edited), f"{what}: voxels"
    og = orc.Grid(g.dims, g.min, g.voxel_size, edited)
    want = orc.build_flat_octree(og)
    got = ctx.download_nodes()
    assert got.tobytes() == want.tobytes(), f"{what}: nodes ({len(got)} vs {len(want)})"
    ctx2.build_octree(edited, g.min, g.voxel_size)
    assert ctx2.download_nodes().tobytes() == want.tobytes(), what
    assert _same_struct(ctx.info(), ctx2.info()), f"{what}: info"
    assert _same_struct(ctx.scene_bounds(), ctx2.scene_bounds()), f"{what}: scene bounds"
    return og, want


def _check_renders(ctx, orc, og, nodes, view, pos, what):
    from conftest import assert_bit_exact
    from ray_tracing_octrees_amd import hip
    f = hip.make_frame(view, pos, W / H, FOV, W, H)
    nt = min(16, orc.max_threads())
    want, _ = orc.render(nodes, og.min, og.voxel_size, view, pos, W / H, FOV, W, H, nthreads=nt)
    assert_bit_exact(ctx.render_host(f), want, f"{what}: default render")
    np.testing.assert_array_equal(ctx.render_steps(f), orc.render_steps(nodes, og.min, og.voxel_size, view, pos, W / H, FOV, W, H),
                                  err_msg=f"{what}: step counts")
    cw, _ = orc.render_closest(nodes, og.min, og.voxel_size, view, pos, W / H, FOV, W, H, nthreads=nt)
    assert_bit_exact(ctx.render_closest_host(f), cw, f"{what}: closest-hit render")
    srgba, sdist = orc.render_skip(nodes, og.min, og.voxel_size, view, pos, W / H, FOV, W, H, nthreads=nt)
    grgba, gdist = ctx.render_skip_host(f)
    assert gdist.tobytes() == sdist.tobytes() and grgba.tobytes() == srgba.tobytes(), f"{what}: nearest-hit render"


@gpu
@pytest.mark.parametrize("name", ["sphere64", "sphere256", "odd37", "calgary"])
def test_gpu_edits_equal_the_rule_and_a_fresh_build(ctx, ctx2, orc, scenes, camera, name, path):
    """Seeded mixed brushes, partly and wholly outside ones, carve everything, fill everything: each edit's grid and changed
    count are the rule's; the context then equals a fresh build of the edited grid (nodes == oracle, info, scene bounds) and
    renders what the oracle renders on it."""
    from ray_tracing_octrees_amd import hip
    g = _grid(orc, scenes, name)
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    rng = np.random.default_rng({"sphere64": 17, "sphere256": 18, "odd37": 19, "calgary": 20}[name])
    dims = g.dims
    big = np.float32(max(dims) * float(g.voxel_size))
    centre_all = _world(g.min, g.voxel_size, np.asarray(dims, np.float64) / 2)
    lists = [
        ("seeded", _seeded_brushes(rng, 24, g.min, g.voxel_size, dims)),
        ("outside", np.concatenate([
            hip.make_brushes([_world(g.min, g.voxel_size, (-3.0, dims[1] / 2, dims[2] / 2))], [[5 * float(g.voxel_size)] * 3], er.BOX, er.FILL),
            hip.make_brushes([_world(g.min, g.voxel_size, (dims[0] + 0.3, dims[1] - 1.0, 0.5))], 6 * float(g.voxel_size), er.SPHERE, er.CARVE),
            hip.make_brushes([_world(g.min, g.voxel_size, (-50.0, -50.0, -50.0))], 10 * float(g.voxel_size), er.SPHERE, er.FILL)])),
        ("carve all", hip.make_brushes([centre_all], big, er.BOX, er.CARVE)),
        ("fill all", hip.make_brushes([centre_all], big, er.BOX, er.FILL)),
    ]
    cur = np.ascontiguousarray(g.data, np.uint8)
    view, pos = _view(orc, camera, name)
    for label, b in lists:
        want, want_changed = er.apply(cur, b, g.min, g.voxel_size)
        got_changed = ctx.edit_voxels(b)
        what = f"{name} {path} {label}"
        assert got_changed == want_changed, f"{what}: changed {got_changed} vs {want_changed}"
        og, nodes = _check_rebuilt(ctx, ctx2, orc, g, want, what)
        if label == "seeded":
            assert want_changed > 0, what
            _check_renders(ctx, orc, og, nodes, view, pos, what)
        cur = want
    assert cur.all()


@gpu
@pytest.mark.parametrize("name,source", [("sphere64", "gpu"), ("odd37", "gpu"), ("sphere64", "upload")])
def test_gpu_edits_rebuild_resident_triangles(ctx, orc, scenes, camera, name, source, path):
    """Triangles resident before an edit (built on the GPU, or uploaded) are rebuilt from the edited grid: the oracle's buffer,
    and the oracle's shadowed triangle frame."""
    from conftest import assert_bit_exact
    from ray_tracing_octrees_amd import hip
    g = _grid(orc, scenes, name)
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    if source == "gpu":
        ctx.build_leaf_triangles(None)
    else:
        tris, off = orc.build_leaf_triangles(g, orc.build_flat_octree(g))
        ctx.upload_leaf_triangles(tris, off)
    b = _seeded_brushes(np.random.default_rng(23), 16, g.min, g.voxel_size, g.dims)
    edited, changed = er.apply(g.data, b, g.min, g.voxel_size)
    assert ctx.edit_voxels(b) == changed > 0
    og = orc.Grid(g.dims, g.min, g.voxel_size, edited)
    nodes = orc.build_flat_octree(og)
    assert ctx.download_nodes().tobytes() == nodes.tobytes()
    wt, wo = orc.build_leaf_triangles(og, nodes)
    gt, go = ctx.download_leaf_triangles()
    assert gt.tobytes() == np.asarray(wt, np.float32).tobytes() and go.tobytes() == np.asarray(wo, np.int32).tobytes(), "triangles"
    ms = ctx.last_edit_ms()
    assert ms[0] >= 0 and ms[1] >= 0 and ms[2] >= 0, ms
    view, pos = _view(orc, camera, name)
    f = hip.make_frame(view, pos, W / H, FOV, W, H)
    want, _ = orc.render_triangles(nodes, wt, wo, og.min, og.voxel_size, view, pos, W / H, FOV, W, H, shadow=True,
                                   nthreads=min(16, orc.max_threads()))
    assert_bit_exact(ctx.render_triangles_host(f, shadow=True), want, f"{name} {source} {path}: triangles + shadow")


@gpu
def test_gpu_ten_edits_equal_one_fresh_build(ctx, ctx2, orc, scenes, camera):
    from ray_tracing_octrees_amd import hip
    g = scenes("sphere256").grid
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    ctx.build_leaf_triangles(None)
    rng = np.random.default_rng(31)
    cur = np.ascontiguousarray(g.data, np.uint8)
    for k in range(10):
        b = _seeded_brushes(rng, 1 + k, g.min, g.voxel_size, g.dims, spread=1.0, max_r=24)
        cur, changed = er.apply(cur, b, g.min, g.voxel_size)
        assert ctx.edit_voxels(b) == changed, k
    og, nodes = _check_rebuilt(ctx, ctx2, orc, g, cur, "ten edits")
    ctx2.build_leaf_triangles(None)
    t1, o1 = ctx.download_leaf_triangles()
    t2, o2 = ctx2.download_leaf_triangles()
    assert t1.tobytes() == t2.tobytes() and o1.tobytes() == o2.tobytes()
    view, pos = _view(orc, camera, "sphere256")
    _check_renders(ctx, orc, og, nodes, view, pos, "ten edits")


def _changing_selection(ctx, cr, g, cur):
    """(grid, edit_components arguments) that the CPU rule (tests/component_ref.py) says change at least one voxel: debris removal
    where there is debris; otherwise a slab is carved first, as test_gpu_carved_sphere_falls_in_two_... does, so that the smaller
    piece is there to drop."""
    from ray_tracing_octrees_amd import hip
    debris = (cr.SET_SOLID, cr.CONN_FACE, cr.SELECT_SMALLER_THAN, 50)
    if cr.apply_selection(cur, *debris)[1] > 0:
        return cur, debris
    dims = np.asarray(g.dims, np.float64)
    centre = _world(g.min, g.voxel_size, dims * (0.5, 0.5, 0.375))
    half = (np.array([dims[0], dims[1], 1.0]) * float(g.voxel_size)).astype(np.float32)
    assert ctx.edit_voxels(hip.make_brushes([centre], [half], er.BOX, er.CARVE)) > 0
    cur = ctx.download_voxels()
    pieces = (cr.SET_SOLID, cr.CONN_FACE, cr.SELECT_ALL_BUT_LARGEST, 0)
    assert cr.apply_selection(cur, *pieces)[1] > 0
    return cur, pieces


@gpu
@pytest.mark.parametrize("name", ["odd37x21", "odd37", "sphere32"])
def test_gpu_three_edits_share_one_rebuild_and_one_count(ctx, ctx2, orc, scenes, name, path):
    """rto_edit_voxels, rto_edit_components and rto_edit_morphology on one context, triangles resident: after each, `changed` is
    the number of bytes of the grid that differ, the nodes, triangles and info are bit for bit those of a fresh build of the
    downloaded grid with triangles, and the labels and the distance field made before the call are refused.  odd37x21 (37 x 21 x 29
    = 22,533 voxels) and odd37: dimX % 16 != 0 and n % 16 != 0, the narrow kernel forms, a last block and a last wave that are
    partly empty; sphere32: the wide forms."""
    import component_ref as cr
    from ray_tracing_octrees_amd import hip
    g = {"odd37x21": lambda: _odd_grid(orc, (37, 21, 29), (15.0, 8.5, 12.0)), "odd37": lambda: _odd_grid(orc),
         "sphere32": lambda: scenes("sphere32").grid}[name]()
    assert (g.dims[0] % 16 == 0) == (name == "sphere32") and (int(np.prod(g.dims)) % 16 == 0) == (name == "sphere32")
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    ctx.build_leaf_triangles(None)
    cur = np.ascontiguousarray(g.data, np.uint8)
    brushes = _seeded_brushes(np.random.default_rng(37), 6, g.min, g.voxel_size, g.dims)
    for step in ("edit_voxels", "edit_components", "edit_morphology"):
        what = f"{name} {path} {step}"
        if step == "edit_components":
            cur, selection = _changing_selection(ctx, cr, g, cur)
        ctx.label_components(cr.SET_SOLID, cr.CONN_FACE)
        ctx.distance_field(hip.SET_SOLID)
        ctx.component_labels(), ctx.distance()                              # both resident now
        if step == "edit_voxels":
            changed = ctx.edit_voxels(brushes)
        elif step == "edit_components":
            changed = ctx.edit_components(*selection)
        else:
            changed = ctx.edit_morphology(hip.MORPH_DILATE, 1.5 * float(g.voxel_size))
        after = ctx.download_voxels()
        print(f"{what}: changed {changed}, bytes that differ {int((after != cur).sum())}")
        assert changed == int((after != cur).sum()) > 0, what
        ctx2.build_octree(after, g.min, g.voxel_size)
        ctx2.build_leaf_triangles(None)
        assert ctx.download_nodes().tobytes() == ctx2.download_nodes().tobytes(), f"{what}: nodes"
        (t1, o1), (t2, o2) = ctx.download_leaf_triangles(), ctx2.download_leaf_triangles()
        assert t1.tobytes() == t2.tobytes() and o1.tobytes() == o2.tobytes(), f"{what}: triangles"
        assert _same_struct(ctx.info(), ctx2.info()), f"{what}: info"
        for read in (ctx.component_labels, ctx.distance):
            with pytest.raises(hip.RtoError) as e:
                read()
            assert e.value.code == hip.RTO_E_INVALID and "the grid has changed since" in str(e.value), what
        cur = after


@gpu
def test_gpu_unchanged_edit_touches_nothing(ctx, orc, scenes, camera):
    from ray_tracing_octrees_amd import hip
    g = scenes("sphere64").grid
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    ctx.build_leaf_triangles(None)
    view, _ = _view(orc, camera, "sphere64")
    ctx.update_frustum(view, FOV, W / H, True)
    nodes, tris = ctx.download_nodes(), ctx.download_leaf_triangles()
    info = bytes(ctx.info())
    assert ctx.info().culling_active == 1
    # wholly outside the grid (no launch at all), then inside but on voxels that are already EMPTY (a launch, no change)
    outside = hip.make_brushes([_world(g.min, g.voxel_size, (-40.0, 0.0, 0.0))], 8 * float(g.voxel_size), er.SPHERE, er.FILL)
    assert ctx.edit_voxels(outside) == 0
    assert ctx.last_edit_ms() == (-1.0, -1.0, -1.0)
    corner = hip.make_brushes([_world(g.min, g.voxel_size, (0.5, 0.5, 0.5))], 0.5 * float(g.voxel_size), er.SPHERE, er.CARVE)
    assert g.data[0, 0, 0] == 0
    assert ctx.edit_voxels(corner) == 0
    ms = ctx.last_edit_ms()
    assert ms[0] >= 0 and ms[1] == -1 and ms[2] == -1, ms
    assert ctx.edit_voxels(hip.make_brushes(np.zeros((0, 3)), 1.0)) == 0
    assert ctx.info().culling_active == 1 and bytes(ctx.info()) == info
    assert ctx.download_nodes().tobytes() == nodes.tobytes()
    t2 = ctx.download_leaf_triangles()
    assert t2[0].tobytes() == tris[0].tobytes() and t2[1].tobytes() == tris[1].tobytes()


@gpu
def test_gpu_edit_errors_leave_the_context_untouched(ctx, orc, scenes):
    from ray_tracing_octrees_amd import hip
    g = scenes("sphere64").grid
    fresh = hip.Context(0)
    try:
        good = hip.make_brushes([_world(g.min, g.voxel_size, (32, 32, 32))], 4 * float(g.voxel_size))
        for call in (lambda: fresh.edit_voxels(good), fresh.download_voxels):
            with pytest.raises(hip.RtoError) as e:
                call()
            assert e.value.code == hip.RTO_E_NO_OCTREE
        fresh.upload_octree(orc.build_flat_octree(g), g.min, g.voxel_size)
        for call in (lambda: fresh.edit_voxels(good), fresh.download_voxels):
            with pytest.raises(hip.RtoError) as e:
                call()
            assert e.value.code == hip.RTO_E_UNSUPPORTED
    finally:
        fresh.close()
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    nodes, vox, info = ctx.download_nodes(), ctx.download_voxels(), bytes(ctx.info())
    c = _world(g.min, g.voxel_size, (32, 32, 32))
    bad = [hip.make_brushes([c], [[np.nan, 1, 1]]), hip.make_brushes([c], [[0.1, -0.1, 0.1]], er.BOX),
           hip.make_brushes([[np.inf, 0, 0]], 0.1), hip.make_brushes([c], 0.1, 2), hip.make_brushes([c], 0.1, er.SPHERE, 7),
           hip.make_brushes([[1e7, 0, 0]], 0.1), hip.make_brushes([c], 1e7)]
    for b in bad:
        with pytest.raises(hip.RtoError) as e:
            ctx.edit_voxels(np.concatenate([good, b]))         # a good brush in front: nothing at all may happen
        assert e.value.code == hip.RTO_E_INVALID, b
    with pytest.raises(hip.RtoError) as e:
        ctx.edit_voxels(np.repeat(good, hip.EDIT_MAX_BRUSHES + 1))
    assert e.value.code == hip.RTO_E_INVALID
    L = hip.load()
    assert L.rto_edit_voxels(ctx._h, None, -1, None) == hip.RTO_E_INVALID
    assert L.rto_edit_voxels(ctx._h, None, 3, None) == hip.RTO_E_INVALID
    assert ctx.download_nodes().tobytes() == nodes.tobytes()
    assert np.array_equal(ctx.download_voxels(), vox) and bytes(ctx.info()) == info


@gpu
@pytest.mark.parametrize("name", ["sphere64", "calgary"])
def test_gpu_pick_carve_pick(ctx, orc, scenes, camera, name):
    """The reference's click flow: FIRST at a pixel, carve a sphere at the hit point, FIRST again: the statement's hit on the
    edited scene, further along the ray."""
    import query_ref as q
    from ray_tracing_octrees_amd import hip
    g = _grid(orc, scenes, name)
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    view, pos = _view(orc, camera, name)
    f = hip.make_frame(view, pos, W / H, FOV, W, H)
    first = ctx.query_pixels(f, np.stack(np.mgrid[0:W, 0:H], -1).reshape(-1, 2).astype(np.int32), hip.QUERY_FIRST)
    hitpix = np.nonzero(first["node"] >= 0)[0]
    assert len(hitpix), name
    i = int(hitpix[len(hitpix) // 2])
    px, py = i // H, i % H
    h0 = ctx.query_pixels(f, [[px, py]], hip.QUERY_FIRST)[0]
    d = orc.generate_rays(view, pos, W / H, FOV, W, H).reshape(H, W, 3)[py, px]
    point = (np.asarray(pos, np.float32) + d * np.float32(h0["t"])).astype(np.float32)
    b = hip.make_brushes([point], 4 * float(g.voxel_size), er.SPHERE, er.CARVE)
    edited, changed = er.apply(g.data, b, g.min, g.voxel_size)
    assert changed > 0 and ctx.edit_voxels(b) == changed
    h1 = ctx.query_pixels(f, [[px, py]], hip.QUERY_FIRST)[0]
    T = q.Tree32(orc.build_flat_octree(orc.Grid(g.dims, g.min, g.voxel_size, edited)), g.min, g.voxel_size)
    want = q.query32(T, pos, d[None, :])[q.FIRST][0]
    assert bytes(np.asarray(h1).tobytes()) == bytes(np.asarray(want).tobytes()), (h1, want)
    assert h1["t"] > h0["t"], (h0, h1)


@gpu
def test_gpu_host_class_edits(orc, scenes):
    """RayTracerBVH (through host.py): setOctree, then editVoxels -- the first edit builds from the class's grid -- renders what
    the oracle renders for the edited grid; grid() returns the edited voxels; a later edit works on the resident grid."""
    from conftest import assert_bit_exact
    import ray_tracing_octrees_amd as rto
    from ray_tracing_octrees_amd import hip
    grid = rto.VoxelGrid.test_sphere(64)
    root = rto.createOctreeFromVoxelGrid(grid)
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    rt.setOctree(root, grid)
    data, gmin, vox = grid.data, grid.min, grid.voxelSize
    cur = data
    cam = rto.Camera(0.5, 0.7, 1.8)
    for seed in (41, 42):
        b = _seeded_brushes(np.random.default_rng(seed), 12, gmin, vox, grid.dims)
        cur, changed = er.apply(cur, b, gmin, vox)
        assert rt.editVoxels(b) == changed, (seed, rt.lastError)
        assert np.array_equal(rt.grid(), cur), seed
        og = orc.Grid(grid.dims, gmin, vox, cur)
        nodes = orc.build_flat_octree(og)
        assert rt.numNodes == len(nodes)
        rt.renderSceneCompute(cam, W, H, W / H, FOV)
        want, _ = orc.render(nodes, gmin, vox, cam.getView(), cam.getPos(), W / H, FOV, W, H)
        assert_bit_exact(rt.framebuffer(), want, f"drop-in class after edit {seed}")
    tris, off = orc.build_leaf_triangles(og, nodes)
    want, _ = orc.render_triangles(nodes, tris, off, gmin, vox, cam.getView(), cam.getPos(), W / H, FOV, W, H, shadow=True)
    for build in (rt.buildLeafTriangles, rt.buildLeafTrianglesOnHost):     # from the resident grid / from grid() on the host
        build()
        rt.renderSceneTriangles(cam, W, H, W / H, FOV, True)
        assert_bit_exact(rt.framebuffer(), want, f"drop-in class: triangles after the edits ({build.__name__})")
    rto.freeOctree(root)
    assert hip.BRUSH_DTYPE.itemsize == 32
