"""Exposure fields (rto_exposure_field): the two statements of the rule in tests/exposure_ref.py against each
other (the open-cube definition in exact integers, and the template march), against the closed forms, against the host layer's CPU
form (host/Exposure.cpp) and, on the GPU, against the library bit for bit: field, summary and the device pointer's copy."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

import exposure_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("rto_exposure_field", "rto_download_exposure", "rto_exposure_device", "rto_last_exposure_ms")
MODES = (er.EXPO_ALL, er.EXPO_SKIN)
REACHES = (1, 3, None)
# VGPRs and LDS bytes the build gives; a kernel that grows past its line here has changed
EXPO_VGPR = {"k_expo_bits": 37, "k_expo_select": 14, "k_expo_march": 11, "k_expo_summary": 22}
EXPO_LDS = {"k_expo_bits": 0, "k_expo_select": 0, "k_expo_march": 0, "k_expo_summary": 96}
W7 = [1 + i % 7 for i in range(len(er.D))]
W7_ZERO = [0 if i == 5 else w for i, w in enumerate(W7)]


def _hip():
    from ray_tracing_octrees_amd import hip
    return hip


def _tc():
    import test_components as tc          # its scenes and its checks of a context
    return tc


# ================================================================ grids
def _seeded(x, y, z, fill):
    return (np.random.default_rng(1000 + x + fill).random((z, y, x)) < fill / 100).astype(np.uint8)


TILE_SIZED = ((31, 7, 7), (32, 8, 8), (33, 9, 9), (65, 17, 17))
SEEDED = {f"s{x}x{y}x{z}_{fill}": (x, y, z, fill) for (x, y, z) in (*TILE_SIZED, (5, 3, 2), (40, 1, 1)) for fill in (10, 30)}
WALLS = {f"wall_{'xyz'[axis]}{at}{'_hole' if hole else ''}": (axis, at, hole) for axis, at in ((0, 31), (0, 32), (1, 7), (1, 8), (2, 7), (2, 8))
         for hole in (False, True)}


def _wall(axis, at, hole):
    """A one-voxel SOLID wall across 65 x 17 x 17 at a word boundary (x) or a 32 x 8 x 8 tile face, with a one-voxel hole or none."""
    g = np.zeros((17, 17, 65), np.uint8)
    index = [slice(None)] * 3
    index[2 - axis] = at
    g[tuple(index)] = 1
    if hole:
        centre = [8, 8, 30]
        centre[2 - axis] = at
        g[tuple(centre)] = 0
    return g


def _named(name):
    if name in SEEDED:
        return _seeded(*SEEDED[name])
    return _wall(*WALLS[name])


_BLOCKED = {}
_REF = {}


def _ref(name, g, dirs, weights, mode, reach, counts=None):
    """The rule's field and summary by the template march, made once per case and left unchanged; the blocked mask of a (grid,
    direction, reach) is shared by every case that needs it."""
    r = er.NO_LIMIT if reach is None else reach

    def blocked(grid, d, rr):
        key = (name, d, rr)
        if key not in _BLOCKED:
            _BLOCKED[key] = er.blocked_by_template(grid, d, rr)
            _BLOCKED[key].setflags(write=False)
        return _BLOCKED[key]

    key = (name, tuple(tuple(int(c) for c in d) for d in dirs), None if weights is None else tuple(weights), mode, r)
    if key not in _REF or counts is not None:
        e, s = er.exposure(g, dirs, weights, mode, r, blocked, counts)
        e.setflags(write=False)
        _REF[key] = (e, s)
    return _REF[key]


# ================================================================ CPU: the rule
@pytest.mark.parametrize("dims", [(7, 5, 4), (5, 3, 2)])
def test_the_definition_equals_the_template_march(dims):
    """(a) == (b) for every direction of D and every start voxel, with no reach and with reach 2."""
    x, y, z = dims
    g = (np.random.default_rng(x).random((z, y, x)) < 0.3).astype(np.uint8)
    for d in er.D:
        for reach in (er.NO_LIMIT, 2):
            assert np.array_equal(er.blocked_by_definition(g, d, reach), er.blocked_by_template(g, d, reach)), (d, reach)


def test_template_properties():
    """The last entry is d / gcd, the length is the number of distinct crossing times, the max-norm never decreases, and every
    component moves one way only.  The length is odd (the times are symmetric about 1 / 2, which an odd component crosses), so a
    row of four entries is padded by three zeros or by one: D holds both."""
    rests = set()
    for d in er.D:
        t = er.template(d)
        p = er.primitive(d)
        assert tuple(t[-1]) == p, d
        times = {Fraction(2 * m + 1, 2 * abs(c)) for c in p for m in range(abs(c))}
        assert len(t) == len(times) and len(t) % 2 == 1, d
        far = np.abs(t).max(axis=1)
        assert far[0] >= 1 and (np.diff(far) >= 0).all(), d
        steps = np.diff(np.vstack([np.zeros((1, 3), np.int64), t]), axis=0)
        assert (steps * np.sign(p) >= 0).all() and (np.abs(steps) <= 1).all() and (np.abs(steps).sum(axis=1) >= 1).all(), d
        rests.add(len(t) % 4)
    assert rests == {1, 3}
    assert len(er.template((1, 1, 1))) == 1 and len(er.template((1, 2, 3))) == 5
    assert np.array_equal(er.template((2, 2, 0)), er.template((1, 1, 0)))
    assert len(er.template((253, 255, 254))) == max(len(er.template(d)) for d in er.D) <= 765


def _closed_forms(run):
    """run(g, dirs, weights, mode, reach) -> (e, summary).  The closed forms of DESIGN.md section 25."""
    g = np.zeros((21, 21, 21), np.uint8)
    g[10, 10, 10] = 1
    for d, reach, want in (((1, 0, 0), None, 10), ((1, 1, 1), None, 10), ((1, 2, 3), None, 17), ((3, -1, 2), None, 17), ((-2, 5, 0), None, 14),
                           ((1, 2, 3), 3, 5)):
        e, s = run(g, [d], None, er.EXPO_ALL, reach)
        assert int((e == 0).sum()) == want == int(s["dark"]) and e[10, 10, 10] == -1, (d, reach)
        assert int(s["evaluated"]) == g.size - 1 and int(s["open"]) == g.size - 1 - want and int(s["total"]) == g.size - 1 - want
    # a full SOLID layer k = 0 under empty space: e = the sum of w_d over c >= 0 wherever no ray can leave the grid sideways on its
    # way down.  Beyond the grid is open sky, so a ray with c < 0 from (i, j, k) is blocked exactly when it meets the layer's top
    # plane strictly inside the grid's footprint, at (i + 1/2 + a t, j + 1/2 + b t) with t = (k - 1/2) / |c|.
    g = np.zeros((6, 5, 9), np.uint8)
    g[0] = 1
    up = [d[2] >= 0 or (d[0] == 0 and d[1] == 0) for d in er.D]
    dirs, weights = [d for d, u in zip(er.D, up) if u], [w for w, u in zip(W7, up) if u]
    want = sum(w for d, w in zip(dirs, weights) if d[2] >= 0)
    e, s = run(g, dirs, weights, er.EXPO_ALL, None)                      # upward, level and straight down: the issue's closed form
    assert (e[0] == -1).all() and (e[1:] == want).all() and int(s["evaluated"]) == 5 * 5 * 9 and int(s["total"]) == want * 5 * 5 * 9
    full = np.full(g.shape, -1, np.int64)
    for k in range(1, 6):
        for j in range(5):
            for i in range(9):
                full[k, j, i] = 0
                for (a, b, c), w in zip(er.D, W7):
                    t = Fraction(2 * k - 1, 2 * abs(c)) if c < 0 else None
                    if t is None or not (0 < Fraction(2 * i + 1, 2) + a * t < 9 and 0 < Fraction(2 * j + 1, 2) + b * t < 5):
                        full[k, j, i] += w
    assert full[1, 2, 4] == sum(w for d, w in zip(er.D, W7) if d[2] >= 0 or d == (255, 1, -1)) and full[5, 0, 0] > full[1, 2, 4]
    e, s = run(g, er.D, W7, er.EXPO_ALL, None)                           # all of D
    assert np.array_equal(e, full) and int(s["evaluated"]) == 5 * 5 * 9 and int(s["total"]) == int(full[1:].sum())
    e, s = run(g, er.D, W7, er.EXPO_SKIN, None)                          # only layer k = 1 is evaluated
    assert (e[0] == -1).all() and np.array_equal(e[1], full[1]) and (e[2:] == -1).all() and int(s["evaluated"]) == 5 * 9
    # corner cutting
    g = np.ones((2, 2, 2), np.uint8)
    g[0, 0, 0] = g[1, 1, 1] = 0
    e, s = run(g, [(1, 1, 1), (1, 1, 0), (1, 0, 0), (1, 2, 3)], [1, 2, 4, 8], er.EXPO_ALL, None)
    assert e[0, 0, 0] == 1 and e[1, 1, 1] == 15 and int((e == -1).sum()) == 6 and int(s["evaluated"]) == 2 and int(s["open"]) == 1
    # a full grid: nothing is evaluated
    g = np.ones((3, 4, 5), np.uint8)
    for mode in MODES:
        e, s = run(g, er.D, None, mode, None)
        assert (e == -1).all() and s.tobytes() == bytes(32)
    # an empty grid
    g = np.zeros((3, 4, 5), np.uint8)
    e, s = run(g, er.D, None, er.EXPO_SKIN, None)
    assert (e == -1).all() and s.tobytes() == bytes(32)
    e, s = run(g, er.D, W7, er.EXPO_ALL, None)
    assert (e == sum(W7)).all() and int(s["open"]) == int(s["evaluated"]) == g.size and int(s["dark"]) == 0
    # a direction given twice counts twice; (2, 2, 0) is (1, 1, 0)
    g = _seeded(5, 3, 2, 30)
    one, _ = run(g, [(1, 1, 0)], None, er.EXPO_ALL, None)
    two, _ = run(g, [(2, 2, 0), (1, 1, 0)], None, er.EXPO_ALL, None)
    assert np.array_equal(np.where(one >= 0, 2 * one, -1), two)


def _host_run(g, dirs, weights, mode, reach):
    import ray_tracing_octrees_amd as rto
    rc, e, s = rto.VoxelGrid.from_array(g, (0.0, 0.0, 0.0), 1.0).exposureField(dirs, weights, mode, er.NO_LIMIT if reach is None else reach)
    assert rc == 0
    return e, s


def test_closed_forms():
    _closed_forms(lambda g, d, w, m, r: er.exposure(g, d, w, m, er.NO_LIMIT if r is None else r))
    _closed_forms(lambda g, d, w, m, r: er.exposure(g, d, w, m, er.NO_LIMIT if r is None else r, er.blocked_by_definition) if g.size <= 240
                  else er.exposure(g, d, w, m, er.NO_LIMIT if r is None else r))
    _closed_forms(_host_run)


@pytest.mark.parametrize("name", [*sorted(SEEDED), *sorted(WALLS)])
def test_reference_equals_the_host_layers_march(name):
    """tests/exposure_ref.py against exposureFieldCPU (host/Exposure.cpp), summary bytes included, on the GPU tests' grids; on the
    tile-sized seeded grids the share of blocked (voxel, direction) pairs is neither nothing nor everything."""
    g = _named(name)
    for mode in MODES:
        for reach in REACHES:
            for weights in ((None, W7, W7_ZERO) if reach is None or name in WALLS else (None,)):
                counts = {} if reach is None and weights is None and name in SEEDED and SEEDED[name][:3] in TILE_SIZED else None
                want, ws = _ref(name, g, er.D, weights, mode, reach, counts)
                got, gs = _host_run(g, er.D, weights, mode, reach)
                assert np.array_equal(got, want) and gs.tobytes() == ws.tobytes(), (name, mode, reach, weights, gs, ws)
                if counts is not None:
                    share = counts["blocked"] / counts["pairs"]
                    print(f"{name} mode {mode}: blocked share {share:.3f}")
                    assert 0.2 <= share <= 0.85, (name, mode, share)


def test_host_layer_refusals_and_quantize_directions():
    import ray_tracing_octrees_amd as rto
    hip = _hip()
    g = _seeded(5, 3, 2, 30)
    vg = rto.VoxelGrid.from_array(g, (0.0, 0.0, 0.0), 1.0)
    ok = [(1, 0, 0), (0, 1, 0)]
    big = 2 ** 31 - 1
    for args in ((None,), ([(1, 1, 1)] * 1025,), ([(1, 0, 0), (0, 0, 0)],), ([(0, -256, 1)],), (ok, [1, -1]), (ok, [big, 1]), (ok, None, 2), (ok, None, -1),
                 (ok, None, 1, 0), (ok, None, 0, -5)):
        rc, e, _ = vg.exposureField(*args)
        assert rc == hip.RTO_E_INVALID and e is None, args
        with pytest.raises(ValueError):
            er.exposure(g, *args)
    assert vg.exposureField(ok, [big - 1, 1])[0] == 0 and vg.exposureField([(1, 1, 1)] * 1024)[0] == 0
    assert vg.exposureField([(255, -255, 255)], None, 0, 1)[0] == 0
    # the helper: scaled to the largest component, rounded, divided by the gcd
    q = hip.quantize_directions([[0.0, 0.0, 2.5], [1.0, 1.0, 0.0], [-3.0, 1.0, 0.5], [0.3, -0.2, 0.1]])
    assert q.dtype == np.int32 and q.tolist() == [[0, 0, 1], [1, 1, 0], [-255, 85, 42], [3, -2, 1]]
    assert hip.quantize_directions([[0.3, -0.2, 0.1]], 3).tolist() == [[3, -2, 1]]
    assert hip.quantize_directions([[4.0, 2.0, 0.0]], 2).tolist() == [[2, 1, 0]]
    q = hip.quantize_directions(er.hemisphere(64))
    assert q.shape == (64, 3) and (np.abs(q).max(axis=1) <= 255).all() and (q[:, 2] > 0).all() and len({tuple(d) for d in q.tolist()}) == 64
    assert (np.gcd.reduce(np.abs(q), axis=1) == 1).all()
    for bad in ([[0.0, 0.0, 0.0]], [[1.0, float("nan"), 0.0]], [[float("inf"), 0.0, 0.0]]):
        with pytest.raises(ValueError):
            hip.quantize_directions(bad)
    for bad in (0, 256):
        with pytest.raises(ValueError):
            hip.quantize_directions([[1.0, 0.0, 0.0]], bad)


def test_exposure_abi_layout_and_exports():
    """sizeof(rto_expo_summary) == 32 with the fields where EXPO_SUMMARY_DTYPE puts them; the constants; the new symbols are exported."""
    hip = _hip()
    assert hip.EXPO_SUMMARY_DTYPE.itemsize == 32 and er.SUMMARY_DTYPE == hip.EXPO_SUMMARY_DTYPE
    fields = ("evaluated", "total", "dark", "open")
    assert [hip.EXPO_SUMMARY_DTYPE.fields[f][1] for f in fields] == [0, 8, 16, 24]
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.fail("no C compiler: the header's layout cannot be checked")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "abi.c")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "rto_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d %d %d %d %d\\n", '
                    'sizeof(rto_expo_summary), offsetof(rto_expo_summary, evaluated), offsetof(rto_expo_summary, total), '
                    'offsetof(rto_expo_summary, dark), offsetof(rto_expo_summary, open), RTO_EXPO_ALL, RTO_EXPO_SKIN, RTO_EXPO_MAX_COMP, '
                    'RTO_EXPO_MAX_DIRS, RTO_EXPO_NO_LIMIT); return 0; }\n')
        exe = os.path.join(tmp, "abi")
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert out == [str(v) for v in (32, 0, 8, 16, 24, er.EXPO_ALL, er.EXPO_SKIN, er.MAX_COMP, er.MAX_DIRS, er.NO_LIMIT)]
    assert (er.EXPO_ALL, er.EXPO_SKIN, er.MAX_COMP, er.MAX_DIRS, er.NO_LIMIT) == (hip.EXPO_ALL, hip.EXPO_SKIN, hip.EXPO_MAX_COMP, hip.EXPO_MAX_DIRS,
                                                                                  hip.EXPO_NO_LIMIT)
    L = hip.load()
    header = open(os.path.join(ROOT, "include", "rto_hip.h")).read()
    for s in SYMS:
        assert s in hip.SYMBOLS and hasattr(L, s), s
        assert s + "(" in header, s


def test_exposure_kernels_keep_their_budgets():
    """The built assembly (the product's flags): every k_expo_* kernel without scratch, spills or v_mfma, within the VGPR and LDS
    figures DESIGN.md section 25 states; the march reads its template rows through scalar loads and holds no atomic."""
    import test_isa_contract as isa
    asm = isa.built_asm()
    if asm is None:
        pytest.fail("no hipcc: the budget cannot be checked")
    meta = isa.kernel_meta(asm)
    names = [k for k in meta if "k_expo_" in k]
    assert len(names) == 6, names              # bits x2, select x2, march, summary
    seen = set()
    for k in names:
        m = meta[k]
        base = next(b for b in EXPO_VGPR if b in k)
        seen.add(base)
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (k, m)
        assert m["vgpr"] <= EXPO_VGPR[base], (k, m)
        entry = re.search(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\.group_segment_fixed_size).)*?\.name:\s+" + re.escape(k) + r"\n", asm, re.S)
        assert entry and int(entry.group(1)) <= EXPO_LDS[base], (k, entry and entry.group(1))
        ins = isa.body(asm, k[len("_ZN3rto"):])
        assert not any(t.startswith(("scratch_", "buffer_load", "buffer_store")) or "v_mfma" in t for t in ins), k
        if base == "k_expo_march":
            assert any(t.startswith("s_load_dwordx4") for t in ins) and not any("atomic" in t or t.startswith("ds_") for t in ins), k
    assert seen == set(EXPO_VGPR)


def test_sanitizer_script_reports_nothing():
    """tools/sanitize_exposure.sh: host/Exposure.cpp as a stand-alone program under AddressSanitizer and UBSan."""
    if not shutil.which("g++"):
        pytest.fail("no g++: the sanitizer build cannot be made")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize_exposure.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "exposure selftest ok" in r.stdout and "UBSan reports: 0" in r.stdout and "ASan reports: 0" in r.stdout, r.stdout


# ================================================================ GPU
gpu = pytest.mark.gpu
W, H, FOV = 128, 96, 45.0
GMIN, VOX = np.array([-0.5, -0.5, -0.5], np.float32), np.float32(1.0 / 64)


def _build(ctx, grid, gmin=GMIN, vox=VOX):
    ctx.set_kernel(_hip().KERNEL_AUTO)
    ctx.build_octree(grid, gmin, vox)


def _check(ctx, g, want, ws, dirs, weights, mode, reach, what):
    got, gs = ctx.exposure_field(dirs, weights, mode, reach)
    assert got.dtype == np.int32 and got.shape == g.shape, what
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} voxels differ"
    assert gs.tobytes() == ws.tobytes(), (what, gs, ws)
    p = ctx.exposure_device()
    assert p and _tc()._d2h(p, 4 * g.size).tobytes() == want.tobytes(), f"{what}: the device pointer's copy"
    ms = ctx.last_exposure_ms()
    assert all(t >= 0 for t in ms), (what, ms)
    return got


def _check_field(ctx, name, g, dirs, weights, mode, reach):
    want, ws = _ref(name, g, dirs, weights, mode, reach)
    return _check(ctx, g, want, ws, dirs, weights, mode, reach, f"{name} n {len(dirs)} weights {weights is not None} mode {mode} reach {reach}")


@gpu
@pytest.mark.parametrize("name", sorted(SEEDED))
def test_gpu_seeded_grids_equal_the_rule(ctx, name):
    """e, the summary and the device copy bit for bit: both modes, reach 1, 3 and none, with D and unit weights; with no reach also
    with weights 1 + index % 7 and with a zero weight among them."""
    g = _named(name)
    _build(ctx, g)
    for mode in MODES:
        for reach in REACHES:
            _check_field(ctx, name, g, er.D, None, mode, reach)
        _check_field(ctx, name, g, er.D, W7, mode, None)
        _check_field(ctx, name, g, er.D, W7_ZERO, mode, None)


@gpu
@pytest.mark.parametrize("name", sorted(WALLS))
def test_gpu_walls_at_word_and_tile_edges(ctx, name):
    """A one-voxel wall at x = 31, x = 32, y = 7, y = 8, z = 7, z = 8 of 65 x 17 x 17, whole and with a one-voxel hole: rays cross
    the word boundary and every tile face from both sides."""
    g = _named(name)
    _build(ctx, g)
    for mode in MODES:
        for reach in REACHES:
            e = _check_field(ctx, name, g, er.D, W7, mode, reach)
        assert (e[g == 1] == -1).all() and (e[g == 0] >= 0).any() and (e[e >= 0] < sum(W7)).any(), name


@gpu
@pytest.mark.parametrize("x", [1, 63, 64, 65, 255, 256, 257])
def test_gpu_list_sizes_around_a_wave_and_a_workgroup(ctx, x):
    """Mode ALL on an empty x * 1 * 1 grid: the list is every voxel, one entry, a wave or a workgroup less one, whole, and one more."""
    g = np.zeros((1, 1, x), np.uint8)
    _build(ctx, g)
    for reach in (1, None):
        e = _check_field(ctx, f"empty{x}", g, er.D, W7, er.EXPO_ALL, reach)
        assert (e == sum(W7)).all()
    got, s = ctx.exposure_field(er.D, W7, er.EXPO_SKIN)                 # nothing is listed: no march and no summary launch
    assert (got == -1).all() and s.tobytes() == bytes(32)
    assert ctx.last_exposure_ms()[1] >= 0


@gpu
@pytest.mark.parametrize("dims", [(32, 3, 3), (64, 5, 2), (96, 2, 3), (31, 3, 3), (63, 5, 2), (97, 2, 3), (32, 17, 15), (32, 16, 16), (32, 257, 1)])
def test_gpu_wide_and_narrow_bit_rows(ctx, dims):
    """k_expo_bits takes its wide form when dimX % 32 == 0: one, two and three words a row, and the sizes one voxel off; 255, 256
    and 257 words are a workgroup of k_expo_bits and k_expo_select less one, whole, and one more."""
    x, y, z = dims
    name = f"rows{x}x{y}x{z}"
    g = (np.random.default_rng(x).random((z, y, x)) < 0.2).astype(np.uint8)
    g[:, :, -1] = 1                                                      # the last bit of the last word of every row
    g[0, 0, -1] = 0
    _build(ctx, g)
    for mode in MODES:
        _check_field(ctx, name, g, er.D, None, mode, None)


@gpu
def test_gpu_a_list_beyond_the_summarys_grid(ctx):
    """k_expo_summary runs at most 4,096 workgroups and strides: 128 x 128 x 66 with a SOLID floor and one SOLID voxel above it lists
    1,064,959 voxels."""
    g = np.zeros((66, 128, 128), np.uint8)
    g[0] = 1
    g[40, 64, 64] = 1
    _build(ctx, g, np.array([-1.0, -1.0, -0.5], np.float32))
    dirs, weights = [(0, 0, 1), (0, 0, -1), (1, 0, 0)], [1, 2, 4]
    e = _check_field(ctx, "floor128", g, dirs, weights, er.EXPO_ALL, None)
    assert int((e >= 0).sum()) == 65 * 128 * 128 - 1 > 4096 * 256
    assert (e[1:40, 64, 64] == 4).all() and (e[41:, 64, 64] == 5).all() and e[40, 64, :64].tolist() == [1] * 64 and (e[1:, 0, 0] == 5).all()


@gpu
@pytest.mark.parametrize("n", [1, 64, 65, 1024])
def test_gpu_direction_counts(ctx, n):
    """D repeated cyclically to n directions, with weights that sum past 16 bits."""
    name = "s33x9x9_30"
    g = _named(name)
    _build(ctx, g)
    dirs = [er.D[i % len(er.D)] for i in range(n)]
    weights = [1 + 97 * (i % 11) for i in range(n)]
    for mode in MODES:
        _check_field(ctx, name, g, dirs, weights, mode, None)
        _check_field(ctx, name, g, dirs, None, mode, 3)


@gpu
def test_gpu_the_longest_period(ctx):
    """(253, 255, 254): 761 entries, 191 rows of the template, alone and at the largest weight."""
    name = "s65x17x17_10"
    g = _named(name)
    _build(ctx, g)
    for d in ((253, 255, 254), (-253, -255, 254), (255, 1, -1)):
        for mode in MODES:
            _check_field(ctx, name, g, [d], [2 ** 31 - 1], mode, None)
            _check_field(ctx, name, g, [d], None, mode, 3)


@gpu
def test_gpu_closed_forms(ctx):
    def run(g, dirs, weights, mode, reach):
        _build(ctx, g)
        return ctx.exposure_field(dirs, weights, mode, reach)
    _closed_forms(run)


@gpu
def test_gpu_sphere64_sky_view_equals_the_host_layer(ctx, scenes):
    """SKIN with 64 quantized directions of the upper hemisphere, against host/Exposure.cpp; and through the host class."""
    import ray_tracing_octrees_amd as rto
    hip = _hip()
    g = scenes("sphere64").grid
    data = np.ascontiguousarray(g.data, np.uint8)
    dirs = hip.quantize_directions(er.hemisphere(64))
    weights = np.maximum(1, np.rint(100 * er.hemisphere(64)[:, 2])).astype(np.int32)
    vg = rto.VoxelGrid.from_array(data, g.min, g.voxel_size)
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(data, g.min, g.voxel_size)
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    assert rt.exposureField(dirs)[0] == hip.RTO_E_NO_OCTREE and rt.exposure()[0] != 0
    rt.setOctreeFromGrid(rto.VoxelGrid.from_array(data, g.min, g.voxel_size))
    assert rt.exposure()[0] == hip.RTO_E_INVALID                        # no field yet
    for w, reach in ((None, None), (weights, None), (weights, 16)):
        rc, want, ws = vg.exposureField(dirs, w, hip.EXPO_SKIN, hip.EXPO_NO_LIMIT if reach is None else reach)
        total = int((weights if w is not None else np.ones(64, np.int32)).sum())
        assert rc == 0 and int(ws["evaluated"]) > 0 and 0 < int(ws["total"]) < total * int(ws["evaluated"])       # some rays blocked, some open
        _check(ctx, data, want, ws, dirs, w, hip.EXPO_SKIN, reach, f"sphere64 reach {reach}")
        rc, s = rt.exposureField(dirs, w, hip.EXPO_SKIN, hip.EXPO_NO_LIMIT if reach is None else reach)
        assert rc == 0 and s.tobytes() == ws.tobytes()
        rc, e = rt.exposure()
        assert rc == 0 and np.array_equal(e, want)
    assert rt.exposureField([(0, 0, 0)])[0] == hip.RTO_E_INVALID and rt.exposureField(dirs, None, 7)[0] == hip.RTO_E_INVALID
    assert np.array_equal(rt.exposure()[1], want) and np.array_equal(rt.grid(), data)


@gpu
def test_gpu_exposure_field_is_dropped_when_the_grid_changes_and_touches_nothing_else(ctx, orc, scenes):
    from conftest import assert_bit_exact, make_camera
    hip = _hip()
    tc = _tc()
    g = scenes("sphere64").grid
    data = np.ascontiguousarray(g.data, np.uint8)
    dirs = hip.quantize_directions(er.hemisphere(16))

    def gone():
        for read in (ctx.exposure, ctx.exposure_device):
            with pytest.raises(hip.RtoError) as e:
                read()
            assert e.value.code == hip.RTO_E_INVALID and "no exposure field is resident" in str(e.value)

    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(data, g.min, g.voxel_size)
    gone()                                                              # never made
    view, pos = make_camera(orc, 0.5, 0.7, 1.8)
    frame = hip.make_frame(view, pos, W / H, FOV, W, H)
    before = ctx.render_host(frame)
    # labels and the distance fields resident before the call are byte-identical after it
    table = ctx.label_components(1, 6)
    labels = ctx.component_labels()
    dist, _ = ctx.distance_field(1)
    geo, _ = ctx.geodesic_field([0], 0, 26, 200)
    thick, _ = ctx.thickness_field(1, 4 * float(g.voxel_size))
    skel, _ = ctx.skeleton_field(1, 26, 1, (), 2)
    nodes, info = ctx.download_nodes(), bytes(ctx.info())
    first, s1 = ctx.exposure_field(dirs, None, hip.EXPO_SKIN)
    assert np.array_equal(ctx.component_labels(), labels) and ctx.components().tobytes() == table.tobytes()
    assert np.array_equal(ctx.distance(), dist) and np.array_equal(ctx.geodesic(), geo) and np.array_equal(ctx.thickness(), thick)
    assert np.array_equal(ctx.skeleton(), skel)
    assert ctx.download_nodes().tobytes() == nodes.tobytes() and bytes(ctx.info()) == info and np.array_equal(ctx.download_voxels(), data)
    assert_bit_exact(ctx.render_host(frame), before, "the frame after exposure_field")
    og = orc.Grid(data.shape[::-1], g.min, g.voxel_size, data)
    tc._check_render(ctx, orc, og, orc.build_flat_octree(og), view, pos, "after exposure_field")
    # the other fields' calls leave it alone, and a second call replaces the first
    ctx.label_components(0, 26)
    ctx.distance_field(0)
    ctx.geodesic_field([0])
    ctx.skeleton_field()
    assert np.array_equal(ctx.exposure(), first)
    second, s2 = ctx.exposure_field(dirs[:5], [3, 1, 4, 1, 5], hip.EXPO_ALL, 4)
    assert second.shape == first.shape and int(s2["evaluated"]) == int((data == 0).sum()) > int(s1["evaluated"])
    assert np.array_equal(ctx.exposure(), second) and not np.array_equal(second, first)
    # every call that changes or replaces the grid drops it
    ctx.build_octree(data, g.min, g.voxel_size)                         # build
    gone()
    ctx.exposure_field(dirs)
    corner = hip.make_brushes([np.asarray(g.min, np.float32) + np.float32(0.5) * g.voxel_size], 0.5 * float(g.voxel_size),
                              hip.BRUSH_SPHERE, hip.EDIT_FILL)
    assert ctx.edit_voxels(corner) == 1                                 # rto_edit_voxels
    gone()
    ctx.exposure_field(dirs)
    assert ctx.edit_skeleton(1, 26, 0, (), 1) > 0                       # rto_edit_skeleton
    gone()
    ctx.exposure_field(dirs)
    v, tris = tc._box_mesh([0.3, 0.3, 0.3], [0.7, 0.7, 0.7])
    ctx.voxelize_mesh(v, tris, np.float32(0.125), grid=((8, 8, 8), np.zeros(3, np.float32), np.float32(0.125)))     # voxelize
    gone()
    e, _ = ctx.exposure_field(dirs)
    assert e.shape == (8, 8, 8)
    ctx.upload_octree(scenes("sphere64").nodes, g.min, g.voxel_size)    # upload: no grid either
    gone()


@gpu
def test_gpu_exposure_errors_leave_the_context_untouched(ctx, orc, scenes):
    from conftest import assert_bit_exact, make_camera
    hip = _hip()
    g = scenes("sphere64").grid
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    dirs = hip.quantize_directions(er.hemisphere(8))
    field, _ = ctx.exposure_field(dirs, None, hip.EXPO_SKIN, 5)
    nodes, info = ctx.download_nodes(), bytes(ctx.info())
    view, pos = make_camera(orc, 0.5, 0.7, 1.8)
    frame = hip.make_frame(view, pos, W / H, FOV, W, H)
    before = ctx.render_host(frame)
    L, h = ctx._L, ctx._h
    nvox = g.data.size
    i32 = lambda v: np.asarray(v, np.int32)
    ok, zero, far = i32([1, 0, 0, 0, 1, 0]), i32([1, 0, 0, 0, 0, 0]), i32([1, 0, 0, 0, 256, 0])
    neg, heavy, fine = i32([1, -1]), i32([2 ** 31 - 1, 1]), i32([2 ** 31 - 2, 1])
    many = np.ones(3 * 1025, np.int32)
    small = np.zeros(nvox - 1, np.int32)
    NL = hip.EXPO_NO_LIMIT
    cases = [
        ("NULL dirs", lambda: L.rto_exposure_field(h, None, None, 2, 1, NL, None)),
        ("n = 0", lambda: L.rto_exposure_field(h, ok.ctypes.data, None, 0, 1, NL, None)),
        ("n < 0", lambda: L.rto_exposure_field(h, ok.ctypes.data, None, -2, 1, NL, None)),
        ("n = 1025", lambda: L.rto_exposure_field(h, many.ctypes.data, None, 1025, 1, NL, None)),
        ("a zero direction", lambda: L.rto_exposure_field(h, zero.ctypes.data, None, 2, 1, NL, None)),
        ("a component of 256", lambda: L.rto_exposure_field(h, far.ctypes.data, None, 2, 1, NL, None)),
        ("a negative weight", lambda: L.rto_exposure_field(h, ok.ctypes.data, neg.ctypes.data, 2, 1, NL, None)),
        ("W = 2^31", lambda: L.rto_exposure_field(h, ok.ctypes.data, heavy.ctypes.data, 2, 1, NL, None)),
        ("unknown mode", lambda: L.rto_exposure_field(h, ok.ctypes.data, None, 2, 2, NL, None)),
        ("negative mode", lambda: L.rto_exposure_field(h, ok.ctypes.data, None, 2, -1, NL, None)),
        ("reach = 0", lambda: L.rto_exposure_field(h, ok.ctypes.data, None, 2, 1, 0, None)),
        ("reach < 0", lambda: L.rto_exposure_field(h, ok.ctypes.data, None, 2, 1, -7, None)),
        ("field capacity", lambda: L.rto_download_exposure(h, small.ctypes.data, nvox - 1)),
        ("NULL out", lambda: L.rto_download_exposure(h, None, nvox)),
    ]
    for what, call in cases:
        assert call() == hip.RTO_E_INVALID, what
        assert L.rto_last_error(h), what
        assert ctx.download_nodes().tobytes() == nodes.tobytes() and bytes(ctx.info()) == info, what
        assert np.array_equal(ctx.download_voxels(), g.data), what
        assert np.array_equal(ctx.exposure(), field), what
    assert_bit_exact(ctx.render_host(frame), before, "the frame after the refusals")
    # the order of the refusals: of several faults the first in the list is the one reported
    bad_w = neg.ctypes.data
    order = [((None, bad_w, 0, 5, 0), "dirs is NULL"), ((far.ctypes.data, bad_w, 0, 5, 0), "n is not in"), ((zero.ctypes.data, bad_w, 2, 5, 0), "a direction is zero"),
             ((far.ctypes.data, bad_w, 2, 5, 0), "a component is beyond"), ((ok.ctypes.data, bad_w, 2, 5, 0), "a weight is negative"),
             ((ok.ctypes.data, heavy.ctypes.data, 2, 5, 0), "sum to more than"), ((ok.ctypes.data, fine.ctypes.data, 2, 5, 0), "unknown mode"),
             ((ok.ctypes.data, fine.ctypes.data, 2, 0, 0), "reach is below 1")]
    for args, text in order:
        assert L.rto_exposure_field(h, *args, None) == hip.RTO_E_INVALID and text in L.rto_last_error(h).decode(), (args, L.rto_last_error(h))
    assert np.array_equal(ctx.exposure(), field) and np.array_equal(ctx.download_voxels(), g.data)
    assert L.rto_exposure_field(h, ok.ctypes.data, fine.ctypes.data, 2, 0, 1, None) == 0          # the largest W, no summary asked for
    assert ctx.last_exposure_ms()[2] == -1 and int(ctx.exposure().max()) == 2 ** 31 - 1
    # no resident grid, no octree: after the arguments
    ctx.upload_octree(scenes("sphere64").nodes, g.min, g.voxel_size)
    uploaded = ctx.render_host(frame)
    with pytest.raises(hip.RtoError) as e:
        ctx.exposure_field(dirs)
    assert e.value.code == hip.RTO_E_UNSUPPORTED
    assert L.rto_exposure_field(h, zero.ctypes.data, None, 2, 1, NL, None) == hip.RTO_E_INVALID    # a zero direction is reported before the missing grid
    assert_bit_exact(ctx.render_host(frame), uploaded, "the frame after the refusals (uploaded octree)")
    fresh = hip.Context(0)
    try:
        with pytest.raises(hip.RtoError) as e:
            fresh.exposure_field(dirs)
        assert e.value.code == hip.RTO_E_NO_OCTREE
        assert fresh._L.rto_exposure_field(fresh._h, ok.ctypes.data, None, 2, 9, NL, None) == hip.RTO_E_INVALID
        with pytest.raises(hip.RtoError) as e:
            fresh.exposure()
        assert e.value.code == hip.RTO_E_INVALID
    finally:
        fresh.close()
