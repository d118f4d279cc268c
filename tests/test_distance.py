"""Distance fields and morphology (rto_distance_field, rto_download_distance, rto_distance_device, rto_edit_morphology,
Context.distance_field / edit_morphology, RayTracerBVH::distanceField / dilate / erode / open / close / thickestPoint).  CPU: the
numpy rule (tests/distance_ref.py) stated twice and against scipy, caps, the algebra of the four operations, DILATE against the
sphere brush of the voxel edits, the host layer's transform, the ABI, the kernels' budgets, the sanitizer script.  GPU: fields and
summaries bit for bit against the rule on grids chosen around k_dt_x's mask words and the envelope's stacks; edits against the rule, a fresh build and the oracle's frame; state and errors."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import distance_ref as dr
import edit_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("rto_distance_field", "rto_download_distance", "rto_distance_device", "rto_last_distance_ms", "rto_edit_morphology",
        "rto_last_morphology_ms")
SETS = (dr.SET_SOLID, dr.SET_EMPTY)
OPS = (dr.DILATE, dr.ERODE, dr.OPEN, dr.CLOSE)
CAPS_VOX = (None, 1.0, 2.5, 3.0)             # caps in voxels; None: no cap
# VGPRs the build gives; a kernel that grows past its line here has changed
DT_VGPR = {"k_dt_x": 50, "k_dt_axis": 26, "k_dt_summary": 12, "k_morph_flip": 28}


def _hip():
    from ray_tracing_octrees_amd import hip
    return hip


def _tc():
    import test_components as tc          # its grids and its checks of a rebuilt context
    return tc


# ================================================================ grids
def _random(shape_xyz, fill, seed):
    x, y, z = shape_xyz
    return (np.random.default_rng(seed).random((z, y, x)) < fill).astype(np.uint8)


def _corner65():
    g = np.zeros((17, 33, 65), np.uint8)
    g[0, 0, 0] = 1
    return g


def _tie():
    g = np.zeros((3, 3, 9), np.uint8)
    g[1, 1, 0] = g[1, 1, 8] = 1                   # (4, 1, 1) is 16 from both
    return g


XEDGE = {f"x{n}": ((n, 5, 3), 0.1, 200 + n) for n in (15, 16, 17, 63, 64, 65, 129)}
LONG = {"long_x": ((200, 3, 3), 0.02, 301), "long_y": ((3, 200, 3), 0.02, 302), "long_z": ((3, 3, 200), 0.02, 303)}
RULE_GRIDS = ["3x2x5", "r17_2", "r17_20", "r17_50", "corner65", "full", "empty", "one_filled", "one_empty"]


def _named_grid(name, scenes=None):
    if name in XEDGE:
        return _random(*XEDGE[name])
    if name in LONG:
        return _random(*LONG[name])
    if name == "3x2x5":
        return _random((3, 2, 5), 0.5, 7)
    if name.startswith("r17_"):
        return _random((17, 9, 5), int(name[4:]) / 100.0, 17 + int(name[4:]))
    if name == "r33":
        return _random((33, 33, 33), 0.31, 41)
    if name == "corner65":
        return _corner65()
    if name == "tie":
        return _tie()
    if name == "checkerboard33":
        return _tc()._checkerboard(33)
    if name == "full":
        return np.ones((12, 20, 40), np.uint8)
    if name == "empty":
        return np.zeros((12, 20, 40), np.uint8)
    if name == "one_filled":
        return np.ones((1, 1, 1), np.uint8)
    if name == "one_empty":
        return np.zeros((1, 1, 1), np.uint8)
    if name == "odd37":
        return _tc()._odd37()
    return np.ascontiguousarray(scenes(name).grid.data, np.uint8)


_REF = {}


def _ref(name, grid, s):
    """The rule's uncapped field, computed once per (grid, set) and shared; the capped ones are thresholds of it."""
    key = (name, s)
    if key not in _REF:
        d = dr.field(grid, s)
        d.setflags(write=False)
        _REF[key] = d
    return _REF[key]


def _mq(vox_units):
    return None if vox_units is None else int(np.floor(vox_units * 64.0 + 0.5))


# ================================================================ CPU: the rule
@pytest.mark.parametrize("name", RULE_GRIDS)
def test_rule_two_statements_agree(name):
    g = _named_grid(name)
    for s in SETS:
        a = dr.separable(g, s)
        assert np.array_equal(dr.brute_force(g, s), a), (name, s)
        assert a.dtype == np.int32 and ((a == 0) == (g == s)).all()
        if not (g == s).any():
            assert (a == dr.NONE).all()


def test_rule_equals_scipy_squared_and_rounded():
    ndi = pytest.importorskip("scipy.ndimage")
    for name in RULE_GRIDS + ["r33"]:
        g = _named_grid(name)
        for s in SETS:
            if (g == s).any():
                e = ndi.distance_transform_edt(g != s)
                assert np.array_equal(np.rint(e * e).astype(np.int64), _ref(name, g, s).astype(np.int64)), (name, s)


def test_rule_longest_parabola_and_tie():
    d = dr.field(_corner65(), dr.SET_SOLID)
    assert d[16, 32, 64] == 64 * 64 + 32 * 32 + 16 * 16 and d[0, 0, 0] == 0
    s = dr.summary(d)
    assert s["max_d2"] == 5376 and s["argmax"] == 65 * 33 * 17 - 1 and s["finite"] == 65 * 33 * 17 and s["reserved"] == 0
    t = dr.field(_tie(), dr.SET_SOLID)
    assert t[1, 1, 4] == 16 and t[1, 1, 3] == 9 and t[1, 1, 5] == 9
    st = dr.summary(t)                                                   # the largest value is held four times: the smallest index wins
    assert st["max_d2"] == 18 and st["argmax"] == int(np.flatnonzero(t.reshape(-1) == 18)[0]) == 4
    none = dr.summary(dr.field(np.zeros((2, 2, 2), np.uint8), dr.SET_SOLID))
    assert none["finite"] == 0 and none["max_d2"] == -1 and none["argmax"] == -1


def test_rule_caps():
    vs = np.float32(1.0 / 64)
    assert dr.quantize(np.float32(3.0) * vs, vs) == 192 and dr.quantize(np.inf, vs) is None and dr.quantize(0.0, vs) == 0
    for bad in (np.nan, -1.0, -np.inf, 1e9):
        with pytest.raises(ValueError):
            dr.quantize(bad, vs)
    assert dr.quantize(np.float32(2.0 ** 22), np.float32(1.0)) == 1 << 28
    with pytest.raises(ValueError):
        dr.quantize(np.float32(2.0 ** 22 + 1), np.float32(1.0))
    g = np.zeros((1, 1, 8), np.uint8)
    g[0, 0, 0] = 1
    full = dr.field(g, dr.SET_SOLID)
    assert list(full[0, 0]) == [0, 1, 4, 9, 16, 25, 36, 49]
    assert list(dr.field(g, dr.SET_SOLID, 192)[0, 0][:5]) == [0, 1, 4, 9, dr.NONE]           # d2 = 9 is in reach at 3 voxels
    assert list(dr.field(g, dr.SET_SOLID, 191)[0, 0][:5]) == [0, 1, 4, dr.NONE, dr.NONE]     # and out at the next smaller rq
    assert list(dr.field(g, dr.SET_SOLID, 0)[0, 0]) == [0] + [dr.NONE] * 7                   # a cap of 0 leaves only the zeros
    for name in ("r17_20", "r17_2", "3x2x5"):
        gg = _named_grid(name)
        for s in SETS:
            for mq in (0, 63, 64, 91, 160, 192, 300):
                want = dr.threshold(_ref(name, gg, s), mq)
                assert np.array_equal(dr.separable(gg, s, mq), want) and np.array_equal(dr.brute_force(gg, s, mq), want)


def _sub(a, b):
    return bool(((a == 1) <= (b == 1)).all())


@pytest.mark.parametrize("name", ["r17_20", "r17_50", "3x2x5", "r33"])
def test_rule_morphology_algebra(name):
    """CLOSE only adds, OPEN only removes, both are idempotent; dilate(X) inside Y exactly when X inside erode(Y)."""
    g = _named_grid(name)
    rng = np.random.default_rng(11)
    for rq in (64, 96, 160):
        dil, ero = dr.morphology(g, dr.DILATE, rq)[0], dr.morphology(g, dr.ERODE, rq)[0]
        opn, cls = dr.morphology(g, dr.OPEN, rq)[0], dr.morphology(g, dr.CLOSE, rq)[0]
        assert _sub(g, dil) and _sub(ero, g) and _sub(g, cls) and _sub(opn, g)
        assert np.array_equal(dr.morphology(cls, dr.CLOSE, rq)[0], cls) and np.array_equal(dr.morphology(opn, dr.OPEN, rq)[0], opn)
        for y in (dil, cls, (rng.random(g.shape) < 0.7).astype(np.uint8), g):
            assert _sub(dil, y) == _sub(g, dr.morphology(y, dr.ERODE, rq)[0])
        assert dr.morphology(g, dr.OPEN, rq)[1] == int((opn != g).sum()) and dr.morphology(g, dr.CLOSE, rq)[1] == int((cls != g).sum())
    for op in OPS:
        out, changed = dr.morphology(g, op, 0)
        assert changed == 0 and np.array_equal(out, g)


def test_rule_pinhole_closes_and_full_grid_does_not_erode():
    g = np.zeros((11, 11, 11), np.uint8)
    g[2:9, 2:9, 2:9] = 1
    cube = g.copy()
    g[5, 5, 5] = 0                                                      # a one-voxel pinhole
    out, changed = dr.morphology(g, dr.CLOSE, 64)
    assert changed == 1 and np.array_equal(out, cube)
    mid = dr.morphology(g, dr.DILATE, 64)[0]
    assert int((mid != g).sum()) > 1                                    # the intermediate grid differs far more: changed counts against the original
    full = np.ones((4, 5, 6), np.uint8)
    for rq in (64, 640):
        out, changed = dr.morphology(full, dr.ERODE, rq)
        assert changed == 0 and np.array_equal(out, full)
    # OPEN removes a whisker that is attached to a block, which no component rule can see
    w = np.zeros((9, 9, 12), np.uint8)
    w[2:7, 2:7, 1:6] = 1
    w[4, 4, 6:11] = 1
    out, changed = dr.morphology(w, dr.OPEN, 64)
    assert changed > 0 and not out[4, 4, 7:11].any() and out[3:6, 3:6, 2:5].all()


@pytest.mark.parametrize("r_vox", [0.5, 1.0, 1.5, 2.5, 4.0])
def test_rule_dilate_of_one_voxel_is_the_sphere_brush(r_vox):
    """Section 11's sphere brush on a voxel centre: D[a] = 128 (i[a] - c[a]), so sum D^2 <= (2 eq)^2 is 4096 d2 <= eq^2."""
    dims = (13, 11, 12)
    gmin, vox = np.array([-2.0, 1.0, 0.5], np.float32), np.float32(0.25)          # quantise exactly
    for c in ((6, 5, 6), (0, 0, 0), (12, 10, 11), (1, 9, 3)):
        g = np.zeros(dims[::-1], np.uint8)
        g[c[2], c[1], c[0]] = 1
        centre = (gmin.astype(np.float64) + (np.asarray(c, np.float64) + 0.5) * float(vox)).astype(np.float32)
        radius = np.float32(r_vox) * vox
        cq, eq = er.quantize(centre, [radius] * 3, er.SPHERE, er.FILL, gmin, vox)
        assert list(cq) == [64 * (2 * i + 1) // 2 for i in c] and eq[0] == dr.quantize(radius, vox) == int(r_vox * 64)
        want = er.cover(dims, er.SPHERE, cq, eq).astype(np.uint8)
        got, changed = dr.morphology(g, dr.DILATE, dr.quantize(radius, vox))
        assert np.array_equal(got, want) and changed == int(want.sum()) - 1, (c, r_vox)


@pytest.mark.parametrize("name", ["r17_2", "r17_20", "r17_50", "r33", "3x2x5", "corner65", "one_filled", "one_empty", "full", "empty"])
def test_reference_equals_the_host_layers_transform(name):
    """tests/distance_ref.py against distanceFieldCPU / applyMorphologyCPU (host/Distance.cpp)."""
    import ray_tracing_octrees_amd as rto
    g = _named_grid(name)
    for s in SETS:
        for mq in (None, 0, 64, 160, 192, 191):
            d, sm = rto.VoxelGrid.from_array(g, (0.0, 0.0, 0.0), 1.0).distanceField(s, -1 if mq is None else mq)
            want = dr.threshold(_ref(name, g, s), mq)
            assert np.array_equal(d, want), (name, s, mq)
            assert sm.tobytes() == dr.summary(want).tobytes(), (name, s, mq)
    for op in OPS:
        for rq in (0, 64, 96, 160):
            vg = rto.VoxelGrid.from_array(g, (0.0, 0.0, 0.0), 1.0)
            want, want_changed = dr.morphology(g, op, rq)
            assert vg.applyMorphology(op, rq) == want_changed and np.array_equal(vg.data, want), (name, op, rq)
    vg = rto.VoxelGrid.from_array(g, (0.0, 0.0, 0.0), 1.0)
    for bad in ((4, 64), (-1, 64), (0, -1), (0, (1 << 28) + 1)):
        assert vg.applyMorphology(*bad) == -1 and np.array_equal(vg.data, g), bad
    with pytest.raises(ValueError):
        vg.distanceField(2, -1)


def test_host_layer_refuses_a_diagonal_the_field_cannot_hold():
    """(dimX-1)^2 + (dimY-1)^2 + (dimZ-1)^2 >= 2^31 - 1 is refused: 46342 x 1 x 1 is, 46341 x 1 x 1 is not."""
    import ray_tracing_octrees_amd as rto
    ok = np.zeros((1, 1, 46341), np.uint8)
    ok[0, 0, 0] = 1
    d, sm = rto.VoxelGrid.from_array(ok, (0.0, 0.0, 0.0), 1.0).distanceField(dr.SET_SOLID, -1)
    assert d[0, 0, -1] == 46340 ** 2 == sm["max_d2"] and sm["argmax"] == 46340 and sm["finite"] == 46341
    bad = np.zeros((1, 1, 46342), np.uint8)
    bad[0, 0, 0] = 1
    vg = rto.VoxelGrid.from_array(bad, (0.0, 0.0, 0.0), 1.0)
    with pytest.raises(ValueError):
        vg.distanceField(dr.SET_SOLID, -1)
    assert vg.applyMorphology(dr.DILATE, 64) == -1


def test_distance_abi_layout_and_exports():
    """sizeof(rto_dist_summary) == 32 with the fields where DIST_SUMMARY_DTYPE puts them; the constants; the new symbols are exported."""
    hip = _hip()
    assert hip.DIST_SUMMARY_DTYPE.itemsize == 32 and dr.SUMMARY_DTYPE == hip.DIST_SUMMARY_DTYPE
    fields = ("max_d2", "argmax", "finite", "reserved")
    assert [hip.DIST_SUMMARY_DTYPE.fields[f][1] for f in fields] == [0, 8, 16, 24]
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.fail("no C compiler: the header's layout cannot be checked")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "abi.c")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "rto_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d %d %d %d %d\\n", '
                    'sizeof(rto_dist_summary), offsetof(rto_dist_summary, max_d2), offsetof(rto_dist_summary, argmax), '
                    'offsetof(rto_dist_summary, finite), offsetof(rto_dist_summary, reserved), RTO_DIST_NONE, RTO_MORPH_DILATE, '
                    'RTO_MORPH_ERODE, RTO_MORPH_OPEN, RTO_MORPH_CLOSE); return 0; }\n')
        exe = os.path.join(tmp, "abi")
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert out == [str(v) for v in (32, 0, 8, 16, 24, hip.DIST_NONE, hip.MORPH_DILATE, hip.MORPH_ERODE, hip.MORPH_OPEN, hip.MORPH_CLOSE)]
    assert (dr.NONE, dr.DILATE, dr.ERODE, dr.OPEN, dr.CLOSE) == (hip.DIST_NONE, hip.MORPH_DILATE, hip.MORPH_ERODE, hip.MORPH_OPEN,
                                                                 hip.MORPH_CLOSE)
    L = hip.load()
    header = open(os.path.join(ROOT, "include", "rto_hip.h")).read()
    for s in SYMS:
        assert s in hip.SYMBOLS and hasattr(L, s), s
        assert s + "(" in header, s


def test_distance_kernels_keep_their_budgets():
    """The built assembly (the product's flags): every k_dt_* and k_morph_* kernel without scratch, spills or v_mfma, at the VGPR
    counts DESIGN.md section 19 states; the 16-byte forms of k_dt_x and k_morph_flip move rows with dwordx4 accesses."""
    import test_isa_contract as isa
    asm = isa.built_asm()
    if asm is None:
        pytest.fail("no hipcc: the budget cannot be checked")
    meta = isa.kernel_meta(asm)
    names = [k for k in meta if "k_dt_" in k or "k_morph_" in k]
    assert len(names) == 7, names               # x x2, axis x2, summary, flip x2
    seen = set()
    for k in names:
        m = meta[k]
        base = next(b for b in DT_VGPR if b in k)
        seen.add(base)
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (k, m)
        assert m["vgpr"] <= DT_VGPR[base], (k, m)
        ins = isa.body(asm, k[len("_ZN3rto"):])
        assert not any(t.startswith(("scratch_", "buffer_load", "buffer_store")) or "v_mfma" in t for t in ins), k
        if ("k_dt_x" in k or "k_morph_flip" in k) and "ILb1E" in k:
            assert any(t.startswith("global_load_dwordx4") for t in ins) and any(t.startswith("global_store_dwordx4") for t in ins), k
    assert seen == set(DT_VGPR)


def test_sanitizer_script_reports_nothing():
    """tools/sanitize_distance.sh: host/Distance.cpp as a stand-alone program under AddressSanitizer and UBSan."""
    if not shutil.which("g++"):
        pytest.fail("no g++: the sanitizer build cannot be made")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize_distance.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "distance selftest ok" in r.stdout and "UBSan reports: 0" in r.stdout and "ASan reports: 0" in r.stdout, r.stdout


# ================================================================ GPU
gpu = pytest.mark.gpu
W, H, FOV = 128, 96, 45.0
GMIN, VOX = np.array([-0.5, -0.5, -0.5], np.float32), np.float32(1.0 / 64)


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


def _build(ctx, grid, gmin=GMIN, vox=VOX):
    ctx.set_kernel(_hip().KERNEL_AUTO)
    ctx.build_octree(grid, gmin, vox)


def _check_fields(ctx, name, g, vox, caps=CAPS_VOX):
    for s in SETS:
        full = _ref(name, g, s)
        for cap in caps:
            want = dr.threshold(full, _mq(cap))
            ws = dr.summary(want)
            max_dist = np.inf if cap is None else np.float32(cap) * np.float32(vox)
            if cap is not None:
                assert dr.quantize(max_dist, vox) == _mq(cap), (cap, vox)
            what = f"{name} set {s} cap {cap}"
            got, gs = ctx.distance_field(s, max_dist)
            assert got.dtype == np.int32 and got.shape == g.shape, what
            assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} voxels differ"
            assert gs.tobytes() == ws.tobytes(), (what, gs, ws)
            assert all(m >= 0 for m in ctx.last_distance_ms()), what


FIELD_GRIDS = [*sorted(XEDGE), *sorted(LONG), "corner65", "tie", "checkerboard33", "full", "empty", "one_filled", "one_empty", "odd37",
               "r33", "sphere64"]


@gpu
@pytest.mark.parametrize("name", FIELD_GRIDS)
def test_gpu_field_and_summary_equal_the_rule(ctx, scenes, name):
    g = _named_grid(name, scenes)
    _build(ctx, g)
    _check_fields(ctx, name, g, VOX)


@gpu
def test_gpu_field_of_calgary_equals_the_rule(ctx, scenes):
    sc = scenes("calgary").grid
    g = np.ascontiguousarray(sc.data, np.uint8)
    ctx.set_kernel(_hip().KERNEL_AUTO)
    ctx.build_octree(g, sc.min, sc.voxel_size)
    _check_fields(ctx, "calgary", g, np.float32(sc.voxel_size))


def _line(axis, n, at):
    shape = [1, 1, 1]
    shape[2 - axis] = n                                                  # axis 0 is x: the last index
    g = np.zeros(shape, np.uint8)
    g.reshape(-1)[list(at)] = 1
    return g


@gpu
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_gpu_longest_line_the_field_allows(ctx, axis):
    """46341 voxels along one axis, the most the 32-bit field allows: k_dt_x's single-row form (1449 mask words, one row per
    workgroup) and positions above 32767 in its notes and in k_dt_axis' packed stack entries.  One FILLED voxel at the start: the
    far end holds 46340^2; three voxels (0, 40000, 46000): entries with positions of 16 significant bits are pushed, stored and
    read back.  The EMPTY sets are left out: the brute force over 46,340 set voxels is too slow, and they add nothing here."""
    hip = _hip()
    n = 46341
    gmin, vox = np.zeros(3, np.float32), np.float32(1.0)
    for at in ((0,), (0, 40000, 46000)):
        g = _line(axis, n, at)
        _build(ctx, g, gmin, vox)
        full = dr.brute_force(g, dr.SET_SOLID)
        for cap in (None, 3.0):
            want = dr.threshold(full, _mq(cap))
            got, gs = ctx.distance_field(dr.SET_SOLID, np.inf if cap is None else cap)
            assert np.array_equal(got, want), (axis, at, cap, int((got != want).sum()))
            assert gs.tobytes() == dr.summary(want).tobytes(), (axis, at, cap, gs)
        if at == (0,):
            gs = ctx.distance_field(dr.SET_SOLID)[1]
            assert gs["max_d2"] == 46340 ** 2 == 2147395600 and gs["argmax"] == 46340 and gs["finite"] == n
    want, changed = dr.morphology(g, dr.DILATE, 96)
    assert changed == 5 and ctx.edit_morphology(hip.MORPH_DILATE, 1.5) == changed
    assert np.array_equal(ctx.download_voxels(), want)


@gpu
def test_gpu_refuses_a_diagonal_the_field_cannot_hold(ctx):
    """(dimX-1)^2 + (dimY-1)^2 + (dimZ-1)^2 >= 2^31 - 1: 46342 x 1 x 1 is refused by both calls and the context stays as it was."""
    hip = _hip()
    g = _line(0, 46342, (0,))
    _build(ctx, g, np.zeros(3, np.float32), np.float32(1.0))
    nodes, info = ctx.download_nodes(), bytes(ctx.info())
    for call in (lambda: ctx.distance_field(dr.SET_SOLID), lambda: ctx.distance_field(dr.SET_EMPTY, 2.0),
                 lambda: ctx.edit_morphology(hip.MORPH_DILATE, 1.5), lambda: ctx.edit_morphology(hip.MORPH_CLOSE, 1.0)):
        with pytest.raises(hip.RtoError) as e:
            call()
        assert e.value.code == hip.RTO_E_UNSUPPORTED and "diagonal" in str(e.value)
        assert ctx.download_nodes().tobytes() == nodes.tobytes() and bytes(ctx.info()) == info
        assert np.array_equal(ctx.download_voxels(), g)
    with pytest.raises(hip.RtoError) as e:
        ctx.distance()
    assert e.value.code == hip.RTO_E_INVALID


@gpu
def test_gpu_distance_device_pointer_holds_the_download(ctx):
    g = _named_grid("r33")
    _build(ctx, g)
    got, _ = ctx.distance_field(dr.SET_SOLID)
    p = ctx.distance_device()
    assert p and _tc()._d2h(p, 4 * g.size).tobytes() == got.tobytes() == _ref("r33", g, dr.SET_SOLID).tobytes()
    assert ctx.distance().tobytes() == got.tobytes()


RADII = {dr.DILATE: 1.5, dr.ERODE: 1.0, dr.OPEN: 1.5, dr.CLOSE: 2.5}


@gpu
@pytest.mark.parametrize("name", ["odd37", "sphere64", "random", "calgary"])
def test_gpu_morphology_equals_the_rule_and_a_fresh_build(ctx, ctx2, orc, scenes, camera, name, path):
    """Each op on the scene as loaded: the grid and changed are the rule's, the context equals a fresh build of that grid
    (nodes == the oracle's, info, scene bounds), the leaf triangles that were resident are those of a fresh triangle build, and the
    frame is the oracle's."""
    tc = _tc()
    data, gmin, vox, view, pos = tc._scene(orc, scenes, camera, name)
    ctx.set_kernel(_hip().KERNEL_AUTO)
    any_change = False
    for op in OPS:
        ctx.build_octree(data, gmin, vox)
        ctx.build_leaf_triangles(None)
        radius = np.float32(RADII[op]) * np.float32(vox)
        rq = dr.quantize(radius, vox)
        assert rq == int(RADII[op] * 64)
        want, want_changed = dr.morphology(data, op, rq)
        got_changed = ctx.edit_morphology(op, radius)
        what = f"{name} {path} op {op}"
        assert got_changed == want_changed, f"{what}: changed {got_changed} vs {want_changed}"
        ms = ctx.last_morphology_ms()
        if want_changed == 0:
            assert np.array_equal(ctx.download_voxels(), data) and ms[0] >= 0 and ms[1] == -1, what
            continue
        any_change = True
        assert ms[0] >= 0 and ms[1] >= 0 and ms[2] >= 0, (what, ms)
        og, nodes = tc._check_rebuilt(ctx, ctx2, orc, gmin, vox, want, what)
        ctx2.build_leaf_triangles(None)                                  # ctx2 holds the fresh build of `want`
        t1, o1 = ctx.download_leaf_triangles()
        t2, o2 = ctx2.download_leaf_triangles()
        assert t1.tobytes() == t2.tobytes() and o1.tobytes() == o2.tobytes(), f"{what}: leaf triangles"
        tc._check_render(ctx, orc, og, nodes, view, pos, what)
        assert ctx.info().culling_active == 0
    assert any_change


@gpu
def test_gpu_morphology_rebuilds_resident_triangles(ctx, ctx2, orc, scenes, path):
    tc = _tc()
    g = scenes("sphere64").grid
    ctx.set_kernel(_hip().KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    ctx.build_leaf_triangles(None)
    radius = np.float32(1.5) * np.float32(g.voxel_size)
    want, changed = dr.morphology(g.data, dr.DILATE, dr.quantize(radius, g.voxel_size))
    assert changed > 0 and ctx.edit_morphology(dr.DILATE, radius) == changed
    assert all(m >= 0 for m in ctx.last_morphology_ms())
    og, nodes = tc._check_rebuilt(ctx, ctx2, orc, g.min, g.voxel_size, want, f"sphere64 dilate {path}")
    ctx2.build_leaf_triangles(None)
    t1, o1 = ctx.download_leaf_triangles()
    t2, o2 = ctx2.download_leaf_triangles()
    assert t1.tobytes() == t2.tobytes() and o1.tobytes() == o2.tobytes()
    wt, wo = orc.build_leaf_triangles(og, nodes)
    assert t1.tobytes() == np.asarray(wt, np.float32).tobytes() and o1.tobytes() == np.asarray(wo, np.int32).tobytes()


@gpu
@pytest.mark.parametrize("r_vox", [0.5, 1.0, 1.5, 2.5, 4.0])
def test_gpu_dilate_of_one_voxel_equals_the_sphere_brush(ctx, ctx2, r_vox):
    hip = _hip()
    dims = (21, 19, 17)
    gmin, vox = np.array([-2.0, 1.0, 0.5], np.float32), np.float32(0.25)
    for c in ((10, 9, 8), (0, 0, 0), (20, 18, 16)):
        g = np.zeros(dims[::-1], np.uint8)
        g[c[2], c[1], c[0]] = 1
        for k in (ctx, ctx2):
            k.set_kernel(hip.KERNEL_AUTO)
            k.build_octree(g, gmin, vox)
        centre = (gmin.astype(np.float64) + (np.asarray(c, np.float64) + 0.5) * float(vox)).astype(np.float32)
        radius = np.float32(r_vox) * vox
        a = ctx.edit_morphology(hip.MORPH_DILATE, radius)
        b = ctx2.edit_voxels(hip.make_brushes([centre], float(radius), hip.BRUSH_SPHERE, hip.EDIT_FILL))
        assert a == b, (c, r_vox, a, b)
        assert np.array_equal(ctx.download_voxels(), ctx2.download_voxels()), (c, r_vox)
        if a:
            assert ctx.download_nodes().tobytes() == ctx2.download_nodes().tobytes()


@gpu
def test_gpu_close_then_fill_cavities_makes_a_pinholed_box_solid(ctx):
    """A voxelized box with a pinhole through one wall: fillCavities alone leaves the shell (the inside reaches the outside),
    CLOSE by 1.5 voxels seals the hole, and fillCavities then gives a solid box."""
    hip = _hip()
    import component_ref as cr
    tc = _tc()
    n = 40
    vox = np.float32(0.25)
    gmin = np.zeros(3, np.float32)
    v, tris = tc._box_mesh([2.6, 2.6, 2.6], [7.4, 7.4, 7.4])
    ctx.voxelize_mesh(v, tris, vox, grid=((n, n, n), gmin, vox))
    shell = ctx.download_voxels()
    z, y, x = np.nonzero(shell)
    row = shell[n // 2, n // 2, x.min():x.max() + 1]
    t = int(np.argmin(row))
    assert 1 <= t <= 3
    # the pinhole: one voxel wide, through the -x wall at the centre of the face
    centre = (np.array([x.min() + t / 2.0, n // 2 + 0.5, n // 2 + 0.5]) * float(vox)).astype(np.float32)
    half = (np.array([t / 2.0 + 0.25, 0.25, 0.25]) * float(vox)).astype(np.float32)
    assert ctx.edit_voxels(hip.make_brushes([centre], [half], hip.BRUSH_BOX, hip.EDIT_CARVE)) == t
    holed = ctx.download_voxels()
    assert not holed[n // 2, n // 2, x.min():x.min() + t].any()
    assert ctx.edit_components(cr.SET_EMPTY, cr.CONN_FACE, cr.SELECT_ENCLOSED) == 0          # a shell it stays
    radius = np.float32(1.5) * vox
    want, changed = dr.morphology(holed, dr.CLOSE, dr.quantize(radius, vox))
    assert ctx.edit_morphology(hip.MORPH_CLOSE, radius) == changed > 0
    closed = ctx.download_voxels()
    assert np.array_equal(closed, want) and closed[n // 2, n // 2, x.min():x.min() + t].any()
    inside = ctx.edit_components(cr.SET_EMPTY, cr.CONN_FACE, cr.SELECT_ENCLOSED)
    assert inside > 1000
    solid = ctx.download_voxels()
    core = (slice(z.min() + t, z.max() + 1 - t), slice(y.min() + t, y.max() + 1 - t), slice(x.min() + t, x.max() + 1 - t))
    # solid: the closed shell with everything it encloses filled, no cavity left, the centre line one filled interval (the
    # voxelized walls themselves need not fill every voxel of their bounding box)
    assert np.array_equal(solid, cr.apply_selection(closed, cr.SET_EMPTY, cr.CONN_FACE, cr.SELECT_ENCLOSED)[0])
    assert solid[core].all() and solid[n // 2, n // 2, x.min():x.max() + 1].all()
    assert ctx.edit_components(cr.SET_EMPTY, cr.CONN_FACE, cr.SELECT_ENCLOSED) == 0


@gpu
def test_gpu_field_and_labels_are_dropped_when_the_grid_changes(ctx, scenes):
    hip = _hip()
    tc = _tc()
    g = scenes("sphere64").grid

    def gone():
        for read in (ctx.distance, ctx.distance_device):
            with pytest.raises(hip.RtoError) as e:
                read()
            assert e.value.code == hip.RTO_E_INVALID and "no distance field is resident" in str(e.value)

    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    gone()                                                              # never made
    ctx.distance_field(dr.SET_SOLID)
    ctx.distance()
    ctx.build_octree(g.data, g.min, g.voxel_size)                       # build
    gone()
    ctx.distance_field(dr.SET_EMPTY, np.float32(2.0) * g.voxel_size)
    corner = hip.make_brushes([np.asarray(g.min, np.float32) + np.float32(0.5) * g.voxel_size], 0.5 * float(g.voxel_size),
                              hip.BRUSH_SPHERE, hip.EDIT_FILL)
    assert ctx.edit_voxels(corner) == 1                                 # rto_edit_voxels
    gone()
    ctx.distance_field(dr.SET_SOLID)
    assert ctx.edit_components(1, 6, hip.SELECT_SMALLER_THAN, 2) == 1   # rto_edit_components: the corner voxel is debris
    gone()
    ctx.distance_field(dr.SET_SOLID)
    ctx.label_components(1, 6)
    assert ctx.edit_morphology(hip.MORPH_DILATE, g.voxel_size) > 0      # rto_edit_morphology: drops the labels too
    gone()
    with pytest.raises(hip.RtoError) as e:
        ctx.component_labels()
    assert e.value.code == hip.RTO_E_INVALID
    ctx.distance_field(dr.SET_SOLID)
    v, tris = tc._box_mesh([0.3, 0.3, 0.3], [0.7, 0.7, 0.7])
    ctx.voxelize_mesh(v, tris, np.float32(0.125), grid=((8, 8, 8), np.zeros(3, np.float32), np.float32(0.125)))     # voxelize
    gone()
    ctx.distance_field(dr.SET_SOLID)
    ctx.upload_octree(scenes("sphere64").nodes, g.min, g.voxel_size)    # upload: no grid either
    gone()


@gpu
def test_gpu_unchanged_morphology_touches_nothing(ctx, orc, scenes):
    from conftest import make_camera
    hip = _hip()
    full = np.ones((16, 16, 16), np.uint8)
    empty = np.zeros((16, 16, 16), np.uint8)
    g = scenes("sphere64").grid
    for data, gmin, vox, calls in (
            (g.data, g.min, g.voxel_size, [(op, 0.0) for op in OPS] + [(dr.DILATE, 0.4 / 64 * float(g.voxel_size))]),
            (full, GMIN, VOX, [(dr.CLOSE, 3.0 * float(VOX)), (dr.ERODE, 5.0 * float(VOX)), (dr.DILATE, float(VOX))]),
            (empty, GMIN, VOX, [(dr.OPEN, 3.0 * float(VOX)), (dr.DILATE, 2.0 * float(VOX))])):
        ctx.set_kernel(hip.KERNEL_AUTO)
        ctx.build_octree(data, gmin, vox)
        if data is g.data:                                               # triangles and a culled frustum state where there is a surface
            ctx.build_leaf_triangles(None)
            view, _ = make_camera(orc, 0.5, 0.7, 1.8)
            ctx.update_frustum(view, FOV, W / H, True)
            assert ctx.info().culling_active == 1
        table = ctx.label_components(0, 6)
        labels = ctx.component_labels()
        field, _ = ctx.distance_field(dr.SET_EMPTY, np.float32(3.0) * np.float32(vox))
        nodes, info = ctx.download_nodes(), bytes(ctx.info())
        tris = ctx.download_leaf_triangles() if data is g.data else None
        for op, radius in calls:
            assert ctx.edit_morphology(op, radius) == 0, (op, radius)
            assert bytes(ctx.info()) == info
            assert ctx.download_nodes().tobytes() == nodes.tobytes()
            if tris is not None:
                t2 = ctx.download_leaf_triangles()
                assert t2[0].tobytes() == tris[0].tobytes() and t2[1].tobytes() == tris[1].tobytes()
            assert np.array_equal(ctx.component_labels(), labels) and ctx.components().tobytes() == table.tobytes()
            assert np.array_equal(ctx.distance(), field)
            assert np.array_equal(ctx.download_voxels(), data)
    # a CLOSE whose intermediate grid differs and whose result does not: a solid cube inside a larger grid
    cube = np.zeros((16, 16, 16), np.uint8)
    cube[4:12, 4:12, 4:12] = 1
    assert dr.morphology(cube, dr.CLOSE, 64)[1] == 0 and dr.morphology(cube, dr.DILATE, 64)[1] > 0
    ctx.build_octree(cube, GMIN, VOX)
    field, _ = ctx.distance_field(dr.SET_SOLID)
    nodes = ctx.download_nodes()
    assert ctx.edit_morphology(dr.CLOSE, VOX) == 0
    assert np.array_equal(ctx.distance(), field) and ctx.download_nodes().tobytes() == nodes.tobytes()
    assert np.array_equal(ctx.download_voxels(), cube)


@gpu
def test_gpu_distance_errors_leave_the_context_untouched(ctx, orc, scenes):
    from conftest import assert_bit_exact, make_camera
    import ray_tracing_octrees_amd as rto
    hip = _hip()
    g = scenes("sphere64").grid
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    field, _ = ctx.distance_field(dr.SET_SOLID)
    nodes, info = ctx.download_nodes(), bytes(ctx.info())
    view, pos = make_camera(orc, 0.5, 0.7, 1.8)
    frame = hip.make_frame(view, pos, W / H, FOV, W, H)
    before = ctx.render_host(frame)
    L, h = ctx._L, ctx._h
    n = C.c_int64(-5)
    small = np.zeros(g.data.size - 1, np.int32)
    too_far = float(np.float32(g.voxel_size) * np.float32(2.0 ** 22 + 1))
    cases = [
        ("unknown set", lambda: L.rto_distance_field(h, 2, 1.0, None)),
        ("negative set", lambda: L.rto_distance_field(h, -1, 1.0, None)),
        ("NaN max_dist", lambda: L.rto_distance_field(h, 1, float("nan"), None)),
        ("negative max_dist", lambda: L.rto_distance_field(h, 1, -1.0, None)),
        ("-inf max_dist", lambda: L.rto_distance_field(h, 1, float("-inf"), None)),
        ("max_dist beyond 2^28 quanta", lambda: L.rto_distance_field(h, 1, too_far, None)),
        ("unknown op", lambda: L.rto_edit_morphology(h, 4, 1.0, C.byref(n))),
        ("negative op", lambda: L.rto_edit_morphology(h, -1, 1.0, C.byref(n))),
        ("NaN radius", lambda: L.rto_edit_morphology(h, 0, float("nan"), C.byref(n))),
        ("negative radius", lambda: L.rto_edit_morphology(h, 0, -0.5, C.byref(n))),
        ("infinite radius", lambda: L.rto_edit_morphology(h, 0, float("-inf"), C.byref(n))),
        ("radius beyond 2^28 quanta", lambda: L.rto_edit_morphology(h, 1, too_far, C.byref(n))),
        ("field capacity", lambda: L.rto_download_distance(h, small.ctypes.data, g.data.size - 1)),
    ]
    for what, call in cases:
        assert call() == hip.RTO_E_INVALID, what
        assert L.rto_last_error(h), what
        assert ctx.download_nodes().tobytes() == nodes.tobytes() and bytes(ctx.info()) == info, what
        assert np.array_equal(ctx.download_voxels(), g.data), what
        assert np.array_equal(ctx.distance(), field), what
    assert_bit_exact(ctx.render_host(frame), before, "the frame after the refusals")
    # through the host class: the same codes
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    assert rt.distanceField(1)[0] == hip.RTO_E_NO_OCTREE and rt.dilate(1.0) == hip.RTO_E_NO_OCTREE
    rt.setOctreeFromGrid(rto.VoxelGrid.from_array(g.data, g.min, g.voxel_size))
    assert rt.distanceField(2)[0] == hip.RTO_E_INVALID and rt.distanceField(1, float("nan"))[0] == hip.RTO_E_INVALID
    assert rt.dilate(-1.0) == hip.RTO_E_INVALID and rt.close(float("nan")) == hip.RTO_E_INVALID and rt.erode(too_far) == hip.RTO_E_INVALID
    assert np.array_equal(rt.grid(), g.data)
    # no resident grid, no octree
    ctx.upload_octree(scenes("sphere64").nodes, g.min, g.voxel_size)
    uploaded = ctx.render_host(frame)
    for call in (lambda: ctx.distance_field(dr.SET_SOLID), lambda: ctx.edit_morphology(dr.DILATE, g.voxel_size)):
        with pytest.raises(hip.RtoError) as e:
            call()
        assert e.value.code == hip.RTO_E_UNSUPPORTED
    assert L.rto_distance_field(h, 2, 1.0, None) == hip.RTO_E_INVALID      # an unknown set is reported before the missing grid
    assert_bit_exact(ctx.render_host(frame), uploaded, "the frame after the refusals (uploaded octree)")
    fresh = hip.Context(0)
    try:
        for call in (lambda: fresh.distance_field(dr.SET_SOLID), lambda: fresh.edit_morphology(dr.DILATE, 1.0)):
            with pytest.raises(hip.RtoError) as e:
                call()
            assert e.value.code == hip.RTO_E_NO_OCTREE
        assert fresh._L.rto_edit_morphology(fresh._h, 7, 1.0, None) == hip.RTO_E_INVALID
    finally:
        fresh.close()


@gpu
def test_gpu_host_class_distance_and_morphology(scenes):
    import ray_tracing_octrees_amd as rto
    hip = _hip()
    g = scenes("sphere64").grid
    data = np.ascontiguousarray(g.data, np.uint8)
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    rt.setOctreeFromGrid(rto.VoxelGrid.from_array(data, g.min, g.voxel_size))
    rc, d2, sm = rt.distanceField(dr.SET_SOLID)
    want = _ref("sphere64", data, dr.SET_SOLID)
    assert rc == 0 and np.array_equal(d2, want) and sm.tobytes() == dr.summary(want).tobytes()
    rc, d2, sm = rt.distanceField(dr.SET_EMPTY, np.float32(2.5) * np.float32(g.voxel_size))
    assert rc == 0 and np.array_equal(d2, dr.threshold(_ref("sphere64", data, dr.SET_EMPTY), 160))
    rc, thick = rt.thickestPoint()
    ws = dr.summary(_ref("sphere64", data, dr.SET_EMPTY))
    assert rc == 0 and thick is not None
    (i, j, k), t2, dist = thick
    assert t2 == ws["max_d2"] and i + 64 * (j + 64 * k) == ws["argmax"] and abs(dist - np.sqrt(float(t2)) * float(g.voxel_size)) < 1e-12
    cur = data
    for call, op, r in ((rt.close, dr.CLOSE, 2.5), (rt.erode, dr.ERODE, 1.0), (rt.dilate, dr.DILATE, 1.5), (rt.open, dr.OPEN, 1.5)):
        radius = np.float32(r) * np.float32(g.voxel_size)
        want, changed = dr.morphology(cur, op, dr.quantize(radius, g.voxel_size))
        assert call(float(radius)) == changed, op
        assert np.array_equal(rt.grid(), want), op
        cur = want
