"""Skeletons (rto_skeleton_field / rto_edit_skeleton): the rule of tests/skeleton_ref.py against a second
witness of the simple-point test (scipy.ndimage.label), against the closed forms, against the invariants the rule promises
(pieces, Euler number, pieces of the complement), against the host layer's CPU form (host/Skeleton.cpp) and, on the GPU, against
the library bit for bit."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import component_ref as cr
import measure_ref as mr
import skeleton_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("rto_skeleton_field", "rto_download_skeleton", "rto_skeleton_device", "rto_edit_skeleton", "rto_last_skeleton_ms",
        "rto_last_skeleton_edit_ms", "rto_debug_skeleton_passes", "rto_debug_set_skeleton_look")
SETS = (sr.SET_SOLID, sr.SET_EMPTY)
MODES = ((sr.CONN_FULL, sr.SKEL_TOPOLOGY), (sr.CONN_FULL, sr.SKEL_CURVE), (sr.CONN_FACE, sr.SKEL_TOPOLOGY))
TILE = (32, 8, 8)           # k_skel_step's tile, x, y, z (rto_skeleton.inc)
# VGPRs and LDS bytes the build gives; a kernel that grows past its line here has changed
SKEL_VGPR = {"k_skel_init": 41, "k_skel_anchors": 7, "k_skel_mark": 31, "k_skel_step": 22, "k_skel_summary": 16, "k_skel_flip": 6}
SKEL_LDS = {"k_skel_init": 0, "k_skel_anchors": 0, "k_skel_mark": 0, "k_skel_step": 1064, "k_skel_summary": 48, "k_skel_flip": 16}


def _hip():
    from ray_tracing_octrees_amd import hip
    return hip


def _hip_host():
    from ray_tracing_octrees_amd import host
    return host.load()


def _tc():
    import test_components as tc          # its scenes and its checks of a rebuilt context
    return tc


# ================================================================ grids
def _random(shape_xyz, fill, seed):
    x, y, z = shape_xyz
    return (np.random.default_rng(seed).random((z, y, x)) < fill).astype(np.uint8)


def _placed(shape, dims_xyz, at_xyz):
    """`shape` inside an empty grid of dims_xyz with its first voxel at at_xyz."""
    g = np.zeros(dims_xyz[::-1], np.uint8)
    z, y, x = shape.shape
    g[at_xyz[2]:at_xyz[2] + z, at_xyz[1]:at_xyz[1] + y, at_xyz[0]:at_xyz[0] + x] = shape
    return g


def _plate(axis):
    """Two voxels thick across the first tile boundary of `axis`: x = 31 | 32, y = 7 | 8, z = 7 | 8."""
    g = np.zeros((16, 16, 64), np.uint8)
    lo = TILE[axis] - 1
    if axis == 0:
        g[:, :, lo:lo + 2] = 1
    elif axis == 1:
        g[:, lo:lo + 2, :] = 1
    else:
        g[lo:lo + 2, :, :] = 1
    return g


def _lin(g, ijk):
    return int(ijk[0] + g.shape[2] * (ijk[1] + g.shape[1] * ijk[2]))


RANDOM = {f"r{x}x{y}x{z}_{int(fill * 10)}": ((x, y, z), fill, 100 * x + int(fill * 10))
          for (x, y, z) in ((31, 7, 7), (32, 8, 8), (33, 9, 9), (65, 17, 17), (5, 3, 2), (40, 1, 1)) for fill in (0.7, 0.9)}
SHAPES = {"ball": lambda: sr.ball(21, 8), "torus": lambda: sr.torus(33, 10, 4), "bar": sr.bar, "shell": lambda: sr.shell(25, 7, 11),
          "block": sr.block}
# the closed forms' shapes across the corner of tiles at (32, 8, 8)
CORNER = {"torus_corner": lambda: _placed(sr.torus(33, 10, 4), (70, 44, 44), (15, 3, 3)),
          "bar_corner": lambda: _placed(sr.bar(), (66, 12, 12), (12, 5, 6)),
          "shell_corner": lambda: _placed(sr.shell(25, 7, 11), (50, 32, 32), (19, 3, 2))}
PLATES = {"plate_x": lambda: _plate(0), "plate_y": lambda: _plate(1), "plate_z": lambda: _plate(2)}
GPU_GRIDS = [*sorted(RANDOM), "block", *sorted(PLATES), *sorted(CORNER)]
CPU_GRIDS = [*sorted(RANDOM), *sorted(SHAPES), *sorted(PLATES), *sorted(CORNER)]


def _named(name):
    if name in RANDOM:
        return _random(*RANDOM[name])
    for table in (SHAPES, CORNER, PLATES):
        if name in table:
            return table[name]()
    raise KeyError(name)


_REF = {}


def _ref(name, g, set, conn, mode, anchors=(), max_passes=None):
    """The rule's field and summary, made once per case and left unchanged."""
    key = (name, set, conn, mode, tuple(int(a) for a in anchors), max_passes)
    if key not in _REF:
        k, s = sr.skeleton(g, set, conn, mode, anchors, sr.NO_LIMIT if max_passes is None else max_passes)
        k.setflags(write=False)
        _REF[key] = (k, s)
    return _REF[key]


# ================================================================ CPU: the simple-point test
def _simple_scipy(mask, conn):
    """The definition by scipy.ndimage.label on the 3 x 3 x 3 block."""
    from scipy import ndimage
    cube = np.array([(mask >> b) & 1 for b in range(27)], dtype=bool).reshape(3, 3, 3)        # [dz, dy, dx]
    cube[1, 1, 1] = False
    s26, s6 = np.ones((3, 3, 3), bool), ndimage.generate_binary_structure(3, 1)
    d = np.abs(np.indices((3, 3, 3)) - 1).sum(0)
    n18, n6 = (d >= 1) & (d <= 2), d == 1
    out = ~cube
    out[1, 1, 1] = False
    big, small = (cube, out) if conn == sr.CONN_FULL else (out, cube)
    if ndimage.label(big, s26)[1] != 1:
        return False
    lab, _ = ndimage.label(small & n18, s6)
    return len(set(lab[small & n6].tolist())) == 1


@pytest.mark.parametrize("conn", [sr.CONN_FULL, sr.CONN_FACE])
def test_simple_point_test_equals_scipy_label(conn):
    """20,000 random blocks, every block of at most 3 voxels and their complements: the flood by shifts (the kernel's form), the
    walk over cells and the host layer's test all say what scipy.ndimage.label says."""
    rng = np.random.default_rng(5 + conn)
    masks = set(int(m) for m in rng.integers(0, 1 << 27, 20000))
    few = {0}
    for a in range(27):
        for b in range(a, 27):
            for c in range(b, 27):
                few.add((1 << a) | (1 << b) | (1 << c))
    masks |= few | {~m & sr.ALL27 for m in few}
    masks = sorted(masks)
    fast = sr.simple(np.asarray(masks, np.uint32), conn)
    L = _hip_host()
    for m, f in zip(masks, fast):
        want = _simple_scipy(m, conn)
        assert bool(f) == want, (hex(m), conn)
        assert bool(L.rtoh_skeleton_simple(m, conn)) == want, (hex(m), conn)
    for m in masks[::97]:
        assert sr.simple_slow(m, conn) == _simple_scipy(m, conn), (hex(m), conn)


def test_the_shifts_are_masked_to_27_bits():
    """Bit 24 is (dx, dy, dz) = (-1, 1, 1) and has no neighbour at dy + 1.  Shifted by 3 without a mask it becomes bit 27, and the
    shift by 9 that follows brings it back as bit 18, (-1, -1, 1): two voxels that are two apart along y would count as joined."""
    for m in ((1 << 24) | (1 << 18), (1 << 24) | (1 << 0), (1 << 26) | (1 << 20), (1 << 8) | (1 << 2)):
        assert not sr.simple(np.asarray([m], np.uint32), sr.CONN_FULL)[0] and not _simple_scipy(m, sr.CONN_FULL), hex(m)
        assert not _hip_host().rtoh_skeleton_simple(m, sr.CONN_FULL), hex(m)


# ================================================================ CPU: closed forms and invariants
def _euler(mask, conn):
    return int(mr.measure_set(mask, conn)["euler"])


def _pieces(mask, conn):
    return len(cr.label(mask.astype(np.uint8), cr.SET_SOLID, conn)[1])


def _check_invariants(g, set, conn, k, what):
    """Pieces and Euler number of X under its connectivity, pieces of the complement under the dual one on the grid padded by one
    empty layer: the same before and after."""
    before = g == (1 if set == sr.SET_SOLID else 0)
    after = k == 0
    dual = sr.CONN_FACE if conn == sr.CONN_FULL else sr.CONN_FULL
    assert _pieces(before, conn) == _pieces(after, conn), what
    assert _euler(before, conn) == _euler(after, conn), what
    assert _pieces(~np.pad(before, 1), dual) == _pieces(~np.pad(after, 1), dual), what


def test_closed_forms():
    full, face, topo, curve = sr.CONN_FULL, sr.CONN_FACE, sr.SKEL_TOPOLOGY, sr.SKEL_CURVE
    ball, torus, bar, shell, block = (_named(n) for n in ("ball", "torus", "bar", "shell", "block"))
    assert int(ball.sum()) == 2109

    def kept_passes(name, g, conn, mode):
        s = _ref(name, g, sr.SET_SOLID, conn, mode)[1]
        return int(s["kept"]), int(s["passes"])
    assert kept_passes("ball", ball, full, topo) == (1, 8)
    assert kept_passes("ball", ball, full, curve)[0] == 15
    assert kept_passes("ball", ball, face, topo)[0] == 1
    assert kept_passes("torus", torus, full, topo)[0] == 56 and _euler(_ref("torus", torus, 1, full, topo)[0] == 0, full) == 0
    assert kept_passes("torus", torus, face, topo)[0] == 80
    assert kept_passes("torus", torus, full, curve)[0] == 128
    assert kept_passes("bar", bar, full, topo)[0] == 1
    assert kept_passes("bar", bar, full, curve) == (40, 2)
    k = _ref("bar", bar, 1, full, curve)[0]
    assert (k[2, 2, 2:38] == 0).all()                                    # its axis between the two end caps
    assert kept_passes("shell", shell, full, topo)[0] == 854 and _euler(_ref("shell", shell, 1, full, topo)[0] == 0, full) == 2
    assert kept_passes("block", block, full, topo) == (1, 30)
    # the cavity of the shell stays a cavity
    assert _pieces(~np.pad(_ref("shell", shell, 1, full, topo)[0] == 0, 1), face) == 2


@pytest.mark.parametrize("name", CPU_GRIDS)
def test_rule_preserves_pieces_euler_number_and_the_complements_pieces(name):
    g = _named(name)
    for set in SETS:
        for conn, mode in MODES:
            if name == "block" and set == sr.SET_EMPTY:
                continue                                                 # no voxel of the set
            k, s = _ref(name, g, set, conn, mode)
            assert ((k == -1) == (g != (1 if set == sr.SET_SOLID else 0))).all()
            assert int(s["kept"]) + int(s["removed"]) == int((k >= 0).sum())
            _check_invariants(g, set, conn, k, (name, set, conn, mode))


@pytest.mark.parametrize("name", ["torus", "r33x9x9_7", "shell_corner"])
def test_rule_limited_run_is_the_thresholded_one_and_a_second_run_removes_nothing(name):
    g = _named(name)
    for set in SETS:
        for conn, mode in MODES:
            full = _ref(name, g, set, conn, mode)[0]
            for m in (1, 3):
                k = _ref(name, g, set, conn, mode, (), m)[0]
                assert np.array_equal(k >= 0, full >= 0) and np.array_equal(k == 0, (full == 0) | (full > m)), (name, set, conn, mode, m)
                assert np.array_equal(k[k > 0], full[k > 0])
            out, changed = sr.edit(g, set, conn, mode)
            assert changed == int((full > 0).sum())
            assert sr.edit(out, set, conn, mode)[1] == 0


def test_rule_anchors():
    """An anchor is never removed; two anchors in a box leave a curve from one to the other whose pieces and Euler number are the
    box's."""
    g = np.ones((9, 9, 30), np.uint8)
    a, b = _lin(g, (0, 4, 4)), _lin(g, (29, 4, 4))
    k, s = sr.skeleton(g, anchors=[a, b, b])
    flat = k.reshape(-1)
    assert flat[a] == 0 and flat[b] == 0 and 30 <= int(s["kept"]) < 45
    kept = k == 0
    assert _pieces(kept, sr.CONN_FULL) == 1 and _euler(kept, sr.CONN_FULL) == 1
    # every voxel of the curve but its two ends has two neighbours on it
    nb = sr.masks_at(kept, np.nonzero(kept))
    counts = sorted(bin(int(m) & sr.N26).count("1") for m in nb)
    assert counts[:2] == [1, 1] and counts[2] >= 2
    # anchors outside the set are ignored
    k2, _ = sr.skeleton(g, sr.SET_EMPTY, anchors=[a])
    assert (k2 == -1).all()


# ================================================================ CPU: the host layer
@pytest.mark.parametrize("name", CPU_GRIDS)
def test_reference_equals_the_host_layers_thinning(name):
    """tests/skeleton_ref.py against skeletonFieldCPU / thinCPU (host/Skeleton.cpp), summary bytes included."""
    import ray_tracing_octrees_amd as rto
    g = _named(name)
    vg = rto.VoxelGrid.from_array(g, (0.0, 0.0, 0.0), 1.0)
    anchors = [0, g.size - 1, g.size // 2, g.size // 2]
    for set in SETS:
        for conn, mode in MODES:
            for a, m in (((), None), ((), 1), ((), 3), (anchors, None)):
                want, ws = _ref(name, g, set, conn, mode, a, m)
                rc, k, s = vg.skeletonField(set, conn, mode, a, sr.NO_LIMIT if m is None else m)
                assert rc == 0 and np.array_equal(k, want), (name, set, conn, mode, a, m)
                assert s.tobytes() == ws.tobytes(), (name, set, conn, mode, a, m, s)
            edit = rto.VoxelGrid.from_array(g, (0.0, 0.0, 0.0), 1.0)
            want, changed = sr.edit(g, set, conn, mode)
            assert edit.thin(set, conn, mode) == changed and np.array_equal(edit.data, want), (name, set, conn, mode)
            assert edit.thin(set, conn, mode) == 0


def test_host_layer_refusals():
    import ray_tracing_octrees_amd as rto
    hip = _hip()
    g = _named("r5x3x2_7")
    vg = rto.VoxelGrid.from_array(g, (0.0, 0.0, 0.0), 1.0)
    for args in ((2, 26, 0), (-1, 26, 0), (1, 18, 0), (1, 26, 2), (1, 6, 1), (1, 26, 0, [0], 0), (1, 26, 0, [-1]), (1, 26, 0, [g.size])):
        rc, out, _ = vg.skeletonField(*args)
        assert rc == hip.RTO_E_INVALID and out is None, args
        assert vg.thin(*args) == hip.RTO_E_INVALID and np.array_equal(vg.data, g), args
        with pytest.raises(ValueError):
            sr.skeleton(g, *args)


def test_skeleton_abi_layout_and_exports():
    """sizeof(rto_skel_summary) == 32 with the fields where SKEL_SUMMARY_DTYPE puts them; the new symbols are exported."""
    hip = _hip()
    assert hip.SKEL_SUMMARY_DTYPE.itemsize == 32 and sr.SUMMARY_DTYPE == hip.SKEL_SUMMARY_DTYPE
    fields = ("kept", "removed", "passes", "reserved")
    assert [hip.SKEL_SUMMARY_DTYPE.fields[f][1] for f in fields] == [0, 8, 16, 24]
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.fail("no C compiler: the header's layout cannot be checked")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "abi.c")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "rto_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d %d %d\\n", '
                    'sizeof(rto_skel_summary), offsetof(rto_skel_summary, kept), offsetof(rto_skel_summary, removed), '
                    'offsetof(rto_skel_summary, passes), offsetof(rto_skel_summary, reserved), RTO_SKEL_TOPOLOGY, RTO_SKEL_CURVE, '
                    'RTO_SKEL_NO_LIMIT); return 0; }\n')
        exe = os.path.join(tmp, "abi")
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert out == [str(v) for v in (32, 0, 8, 16, 24, sr.SKEL_TOPOLOGY, sr.SKEL_CURVE, sr.NO_LIMIT)]
    assert (sr.SKEL_TOPOLOGY, sr.SKEL_CURVE, sr.NO_LIMIT) == (hip.SKEL_TOPOLOGY, hip.SKEL_CURVE, hip.SKEL_NO_LIMIT)
    L = hip.load()
    header = open(os.path.join(ROOT, "include", "rto_hip.h")).read()
    for s in SYMS:
        assert s in hip.SYMBOLS and hasattr(L, s), s
        assert s + "(" in header, s


def test_skeleton_kernels_keep_their_budgets():
    """The built assembly (the product's flags): every k_skel_* kernel without scratch, spills or v_mfma, within the VGPR and LDS
    figures DESIGN.md section 23 states."""
    import test_isa_contract as isa
    asm = isa.built_asm()
    if asm is None:
        pytest.fail("no hipcc: the budget cannot be checked")
    meta = isa.kernel_meta(asm)
    names = [k for k in meta if "k_skel_" in k]
    assert len(names) == 10, names              # init x2, anchors, mark x2, step x3, summary, flip
    seen = set()
    for k in names:
        m = meta[k]
        base = next(b for b in SKEL_VGPR if b in k)
        seen.add(base)
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (k, m)
        assert m["vgpr"] <= SKEL_VGPR[base], (k, m)
        entry = re.search(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\.group_segment_fixed_size).)*?\.name:\s+" + re.escape(k) + r"\n", asm, re.S)
        assert entry and int(entry.group(1)) <= SKEL_LDS[base], (k, entry and entry.group(1))
        ins = isa.body(asm, k[len("_ZN3rto"):])
        assert not any(t.startswith(("scratch_", "buffer_load", "buffer_store")) or "v_mfma" in t for t in ins), k
    assert seen == set(SKEL_VGPR)


def test_sanitizer_script_reports_nothing():
    """tools/sanitize_skeleton.sh: host/Skeleton.cpp as a stand-alone program under AddressSanitizer and UBSan."""
    if not shutil.which("g++"):
        pytest.fail("no g++: the sanitizer build cannot be made")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize_skeleton.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "skeleton selftest ok" in r.stdout and "UBSan reports: 0" in r.stdout and "ASan reports: 0" in r.stdout, r.stdout


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


def _check_field(ctx, name, g, set, conn, mode, anchors=(), max_passes=None):
    want, ws = _ref(name, g, set, conn, mode, anchors, max_passes)
    what = f"{name} set {set} conn {conn} mode {mode} anchors {len(anchors)} max_passes {max_passes}"
    got, gs = ctx.skeleton_field(set, conn, mode, anchors, max_passes)
    assert got.dtype == np.int32 and got.shape == g.shape, what
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} voxels differ"
    assert gs.tobytes() == ws.tobytes(), (what, gs, ws)
    ms = ctx.last_skeleton_ms()
    assert all(t >= 0 for t in ms), (what, ms)
    launches, tiles = ctx.skeleton_passes()
    ran = int(ws["passes"]) + (0 if max_passes is not None and int(ws["passes"]) == max_passes else 1)
    assert launches % 9 == 0 and launches >= 9 * ran and tiles >= 1, (what, launches, tiles)
    return got


@gpu
@pytest.mark.parametrize("name", GPU_GRIDS)
def test_gpu_field_and_summary_equal_the_rule(ctx, name):
    """k and the summary bit for bit, both sets, FULL / TOPOLOGY, FULL / CURVE and FACE / TOPOLOGY, with max_passes 1, 3 and none."""
    g = _named(name)
    _build(ctx, g)
    for set in SETS:
        for conn, mode in MODES:
            for m in (None, 1, 3):
                _check_field(ctx, name, g, set, conn, mode, (), m)


@gpu
def test_gpu_anchors(ctx):
    """Anchors on both sides of a tile face and far apart in a full grid; 1,000 anchors with duplicates and voxels outside the set."""
    g = np.ones((16, 16, 64), np.uint8)
    _build(ctx, g)
    anchors = [_lin(g, p) for p in ((31, 8, 8), (32, 8, 8), (31, 7, 8), (31, 8, 7), (2, 2, 2), (61, 13, 13))]
    for conn, mode in MODES:
        k = _check_field(ctx, "ones64", g, sr.SET_SOLID, conn, mode, anchors)
        assert (k.reshape(-1)[anchors] == 0).all()
    name = "r65x17x17_7"
    g = _named(name)
    _build(ctx, g)
    many = np.random.default_rng(9).integers(0, g.size, 1000)
    many[500:] = many[:500]
    assert (g.reshape(-1)[many] == 0).any() and (g.reshape(-1)[many] == 1).any()
    for set in SETS:
        for conn, mode in MODES:
            _check_field(ctx, name, g, set, conn, mode, many.tolist())


@gpu
def test_gpu_looks_change_no_byte(ctx):
    """The full block, whose central tile is quiet until the front arrives: the field is the same bit for bit whether the host
    looks at the device after every pass or after every 8 (and 64).  The figures are printed for DESIGN.md."""
    g = _named("block")
    _build(ctx, g)
    try:
        for conn, mode in MODES:
            fields = []
            for look in (1, 8, 64):
                ctx.debug_set_skeleton_look(look)
                fields.append(_check_field(ctx, "block", g, sr.SET_SOLID, conn, mode).tobytes())
                print(f"block conn {conn} mode {mode} look {look}: launches, tiles run = {ctx.skeleton_passes()}, ms = {ctx.last_skeleton_ms()}")
            assert fields[0] == fields[1] == fields[2]
        for bad in (0, 65, -1):
            with pytest.raises(_hip().RtoError) as e:
                ctx.debug_set_skeleton_look(bad)
            assert e.value.code == _hip().RTO_E_INVALID
    finally:
        ctx.debug_set_skeleton_look(8)
    # the worklist: with looks of 1 the block runs fewer tiles than every tile in every sub-step
    ctx.debug_set_skeleton_look(1)
    try:
        _check_field(ctx, "block", g, sr.SET_SOLID, sr.CONN_FULL, sr.SKEL_TOPOLOGY)
        launches, tiles = ctx.skeleton_passes()
        assert launches == 9 * 31 and tiles < 8 * 31 * 27, (launches, tiles)
    finally:
        ctx.debug_set_skeleton_look(8)


@gpu
def test_gpu_skeleton_device_pointer_holds_the_download(ctx):
    name = "r33x9x9_7"
    g = _named(name)
    _build(ctx, g)
    got, _ = ctx.skeleton_field(sr.SET_SOLID, sr.CONN_FULL, sr.SKEL_CURVE)
    p = ctx.skeleton_device()
    assert p and _tc()._d2h(p, 4 * g.size).tobytes() == got.tobytes() == _ref(name, g, sr.SET_SOLID, sr.CONN_FULL, sr.SKEL_CURVE)[0].tobytes()
    assert ctx.skeleton().tobytes() == got.tobytes()


def _edit_cases():
    return [("solid full curve", sr.SET_SOLID, sr.CONN_FULL, sr.SKEL_CURVE, None), ("solid face topology 2 passes", sr.SET_SOLID, sr.CONN_FACE, sr.SKEL_TOPOLOGY, 2),
            ("empty full topology 3 passes", sr.SET_EMPTY, sr.CONN_FULL, sr.SKEL_TOPOLOGY, 3)]


@gpu
@pytest.mark.parametrize("triangles", [False, True])
@pytest.mark.parametrize("name", ["odd37", "sphere64"])
def test_gpu_edits_equal_the_rule_and_a_fresh_build(ctx, ctx2, orc, scenes, camera, name, path, triangles):
    """The grid is the rule's; the nodes are a fresh build's on a second context; the frame is the oracle's; resident leaf triangles
    are rebuilt; pieces and Euler number on the same context are what they were; a second edit changes nothing."""
    tc = _tc()
    hip = _hip()
    data, gmin, vox, view, pos = tc._scene(orc, scenes, camera, name)
    ctx.set_kernel(hip.KERNEL_AUTO)
    for label, set, conn, mode, m in _edit_cases():
        what = f"{name} {path} {label} triangles {triangles}"
        ctx.build_octree(data, gmin, vox)
        if triangles:
            ctx.build_leaf_triangles(None)
        pieces = len(ctx.label_components(set, conn))
        euler = int(ctx.measure_components()[1]["euler"])
        k = _ref(name, data, set, conn, mode, (), m)[0]
        want = data.copy()
        want[k > 0] = 0 if set == sr.SET_SOLID else 1
        want_changed = int((k > 0).sum())
        assert want_changed > 0
        assert ctx.edit_skeleton(set, conn, mode, (), m) == want_changed, what
        ms = ctx.last_skeleton_edit_ms()
        assert ms[0] >= 0 and ms[1] >= 0 and (ms[2] >= 0) == triangles, (what, ms)
        og, nodes = tc._check_rebuilt(ctx, ctx2, orc, gmin, vox, want, what)
        if triangles:
            ctx2.build_leaf_triangles(None)
            t1, o1 = ctx.download_leaf_triangles()
            t2, o2 = ctx2.download_leaf_triangles()
            assert t1.tobytes() == t2.tobytes() and o1.tobytes() == o2.tobytes(), f"{what}: leaf triangles"
        tc._check_render(ctx, orc, og, nodes, view, pos, what)
        assert ctx.info().culling_active == 0
        assert len(ctx.label_components(set, conn)) == pieces, what
        assert int(ctx.measure_components()[1]["euler"]) == euler, what
        if m is None:
            assert ctx.edit_skeleton(set, conn, mode) == 0, what
            assert np.array_equal(ctx.download_voxels(), want), what


@gpu
def test_gpu_skeleton_field_is_dropped_when_the_grid_changes_and_kept_when_it_does_not(ctx, orc, scenes):
    from conftest import make_camera
    hip = _hip()
    g = scenes("sphere64").grid
    data = np.ascontiguousarray(g.data, np.uint8)

    def gone():
        for read in (ctx.skeleton, ctx.skeleton_device):
            with pytest.raises(hip.RtoError) as e:
                read()
            assert e.value.code == hip.RTO_E_INVALID and "no skeleton field is resident" in str(e.value)

    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(data, g.min, g.voxel_size)
    gone()                                                              # never made
    ctx.skeleton_field()
    ctx.skeleton()
    ctx.build_octree(data, g.min, g.voxel_size)                         # build
    gone()
    # the other fields survive a skeleton_field call, and it survives theirs
    table = ctx.label_components(1, 6)
    labels = ctx.component_labels()
    dist, _ = ctx.distance_field(1)
    geo, _ = ctx.geodesic_field([0], 0, 26, 200)
    skel, _ = ctx.skeleton_field(sr.SET_SOLID, sr.CONN_FULL, sr.SKEL_CURVE, (), 2)
    assert np.array_equal(ctx.component_labels(), labels) and ctx.components().tobytes() == table.tobytes()
    assert np.array_equal(ctx.distance(), dist) and np.array_equal(ctx.geodesic(), geo)
    ctx.label_components(0, 26)
    ctx.distance_field(0)
    ctx.geodesic_field([0])
    assert np.array_equal(ctx.skeleton(), skel)
    # an edit that changes nothing touches nothing: here every voxel is an anchor
    ctx.build_leaf_triangles(None)
    view, _ = make_camera(orc, 0.5, 0.7, 1.8)
    ctx.update_frustum(view, FOV, W / H, True)
    assert ctx.info().culling_active == 1
    nodes, info = ctx.download_nodes(), bytes(ctx.info())
    every = np.arange(data.size, dtype=np.int64)
    assert ctx.edit_skeleton(sr.SET_SOLID, sr.CONN_FULL, sr.SKEL_TOPOLOGY, every) == 0
    assert bytes(ctx.info()) == info and ctx.info().culling_active == 1 and ctx.download_nodes().tobytes() == nodes.tobytes()
    assert np.array_equal(ctx.skeleton(), skel) and np.array_equal(ctx.download_voxels(), data)
    ms = ctx.last_skeleton_edit_ms()
    assert ms[0] >= 0 and ms[1] == -1 and ms[2] == -1
    corner = hip.make_brushes([np.asarray(g.min, np.float32) + np.float32(0.5) * g.voxel_size], 0.5 * float(g.voxel_size),
                              hip.BRUSH_SPHERE, hip.EDIT_FILL)
    assert ctx.edit_voxels(corner) == 1                                 # rto_edit_voxels
    gone()
    ctx.skeleton_field()
    ctx.label_components(1, 6)
    ctx.distance_field(1)
    ctx.geodesic_field([0])
    assert ctx.edit_skeleton(sr.SET_SOLID, sr.CONN_FULL, sr.SKEL_TOPOLOGY, (), 1) > 0       # rto_edit_skeleton: drops all of them
    gone()
    for read in (ctx.component_labels, ctx.distance, ctx.geodesic):
        with pytest.raises(hip.RtoError) as e:
            read()
        assert e.value.code == hip.RTO_E_INVALID
    ctx.skeleton_field()
    ctx.upload_octree(scenes("sphere64").nodes, g.min, g.voxel_size)    # upload: no grid either
    gone()


@gpu
def test_gpu_skeleton_errors_leave_the_context_untouched(ctx, orc, scenes):
    from conftest import assert_bit_exact, make_camera
    import ray_tracing_octrees_amd as rto
    hip = _hip()
    g = scenes("sphere64").grid
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    field, _ = ctx.skeleton_field(sr.SET_SOLID, sr.CONN_FULL, sr.SKEL_CURVE, (), 2)
    nodes, info = ctx.download_nodes(), bytes(ctx.info())
    view, pos = make_camera(orc, 0.5, 0.7, 1.8)
    frame = hip.make_frame(view, pos, W / H, FOV, W, H)
    before = ctx.render_host(frame)
    L, h = ctx._L, ctx._h
    n = C.c_int64(-5)
    nvox = g.data.size
    ok = np.asarray([0, 1], np.int64)
    low, high = np.asarray([0, -1], np.int64), np.asarray([nvox, 0], np.int64)
    small = np.zeros(nvox - 1, np.int32)
    NL = hip.SKEL_NO_LIMIT
    cases = [
        ("unknown set", lambda: L.rto_skeleton_field(h, 2, 26, 0, ok.ctypes.data, 2, NL, None)),
        ("negative set", lambda: L.rto_skeleton_field(h, -1, 26, 0, ok.ctypes.data, 2, NL, None)),
        ("unknown connectivity", lambda: L.rto_skeleton_field(h, 1, 18, 0, ok.ctypes.data, 2, NL, None)),
        ("unknown mode", lambda: L.rto_skeleton_field(h, 1, 26, 2, ok.ctypes.data, 2, NL, None)),
        ("CURVE with FACE", lambda: L.rto_skeleton_field(h, 1, 6, 1, ok.ctypes.data, 2, NL, None)),
        ("n < 0", lambda: L.rto_skeleton_field(h, 1, 26, 0, ok.ctypes.data, -1, NL, None)),
        ("NULL anchors", lambda: L.rto_skeleton_field(h, 1, 26, 0, None, 2, NL, None)),
        ("max_passes = 0", lambda: L.rto_skeleton_field(h, 1, 26, 0, ok.ctypes.data, 2, 0, None)),
        ("negative anchor", lambda: L.rto_skeleton_field(h, 1, 26, 0, low.ctypes.data, 2, NL, None)),
        ("anchor == voxels", lambda: L.rto_skeleton_field(h, 1, 26, 0, high.ctypes.data, 2, NL, None)),
        ("edit: unknown set", lambda: L.rto_edit_skeleton(h, 2, 26, 0, ok.ctypes.data, 2, NL, C.byref(n))),
        ("edit: unknown connectivity", lambda: L.rto_edit_skeleton(h, 1, 7, 0, ok.ctypes.data, 2, NL, C.byref(n))),
        ("edit: unknown mode", lambda: L.rto_edit_skeleton(h, 1, 26, -1, ok.ctypes.data, 2, NL, C.byref(n))),
        ("edit: CURVE with FACE", lambda: L.rto_edit_skeleton(h, 0, 6, 1, None, 0, NL, C.byref(n))),
        ("edit: NULL anchors", lambda: L.rto_edit_skeleton(h, 1, 26, 0, None, 1, NL, C.byref(n))),
        ("edit: max_passes = -3", lambda: L.rto_edit_skeleton(h, 1, 26, 0, None, 0, -3, C.byref(n))),
        ("edit: anchor out of range", lambda: L.rto_edit_skeleton(h, 1, 26, 0, high.ctypes.data, 2, NL, C.byref(n))),
        ("field capacity", lambda: L.rto_download_skeleton(h, small.ctypes.data, nvox - 1)),
    ]
    for what, call in cases:
        assert call() == hip.RTO_E_INVALID, what
        assert L.rto_last_error(h), what
        assert ctx.download_nodes().tobytes() == nodes.tobytes() and bytes(ctx.info()) == info, what
        assert np.array_equal(ctx.download_voxels(), g.data), what
        assert np.array_equal(ctx.skeleton(), field), what
    assert_bit_exact(ctx.render_host(frame), before, "the frame after the refusals")
    # the order of the refusals: of several faults the first in the list is the one reported
    order = [((2, 18, 5, None, -1, 0), "unknown set"), ((1, 18, 5, None, -1, 0), "connectivity must be"), ((1, 26, 5, None, -1, 0), "unknown mode"),
             ((1, 6, 1, None, -1, 0), "needs RTO_CONN_FULL"), ((1, 26, 0, None, -1, 0), "n is negative"), ((1, 26, 0, None, 2, 0), "anchors is NULL"),
             ((1, 26, 0, high.ctypes.data, 2, 0), "max_passes is below 1"), ((1, 26, 0, high.ctypes.data, 2, 1), "an anchor is not a voxel")]
    for entry in (L.rto_skeleton_field, L.rto_edit_skeleton):
        for args, text in order:
            assert entry(h, *args, None) == hip.RTO_E_INVALID and text in L.rto_last_error(h).decode(), (args, L.rto_last_error(h))
    assert np.array_equal(ctx.skeleton(), field) and np.array_equal(ctx.download_voxels(), g.data)
    assert L.rto_skeleton_field(h, 1, 26, 1, None, 0, 2, None) == 0                       # no anchors at all is a call like any other
    assert np.array_equal(ctx.skeleton(), field)
    # through the host class: the same codes
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    assert rt.skeletonField()[0] == hip.RTO_E_NO_OCTREE and rt.thin() == hip.RTO_E_NO_OCTREE
    rt.setOctreeFromGrid(rto.VoxelGrid.from_array(g.data, g.min, g.voxel_size))
    assert rt.skeletonField(2)[0] == hip.RTO_E_INVALID and rt.skeletonField(1, 6, 1)[0] == hip.RTO_E_INVALID
    assert rt.skeletonField(1, 26, 0, [nvox])[0] == hip.RTO_E_INVALID and rt.thin(0, 0) == hip.RTO_E_INVALID
    assert rt.centreline(-1, 0)[0] == hip.RTO_E_INVALID
    assert np.array_equal(rt.grid(), g.data)
    # no resident grid, no octree
    ctx.upload_octree(scenes("sphere64").nodes, g.min, g.voxel_size)
    uploaded = ctx.render_host(frame)
    for call in (lambda: ctx.skeleton_field(), lambda: ctx.edit_skeleton()):
        with pytest.raises(hip.RtoError) as e:
            call()
        assert e.value.code == hip.RTO_E_UNSUPPORTED
    assert L.rto_skeleton_field(h, 2, 26, 0, ok.ctypes.data, 2, NL, None) == hip.RTO_E_INVALID   # an unknown set is reported before the missing grid
    assert_bit_exact(ctx.render_host(frame), uploaded, "the frame after the refusals (uploaded octree)")
    fresh = hip.Context(0)
    try:
        for call in (lambda: fresh.skeleton_field(), lambda: fresh.edit_skeleton()):
            with pytest.raises(hip.RtoError) as e:
                call()
            assert e.value.code == hip.RTO_E_NO_OCTREE
        assert fresh._L.rto_edit_skeleton(fresh._h, 7, 26, 0, ok.ctypes.data, 2, NL, None) == hip.RTO_E_INVALID
    finally:
        fresh.close()


@gpu
def test_gpu_host_class_skeleton(scenes):
    import ray_tracing_octrees_amd as rto
    g = scenes("sphere64").grid
    data = np.ascontiguousarray(g.data, np.uint8)
    vg = rto.VoxelGrid.from_array(data, g.min, g.voxel_size)
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    rt.setOctreeFromGrid(rto.VoxelGrid.from_array(data, g.min, g.voxel_size))
    for set, conn, mode, anchors, m in ((1, 26, 1, [], sr.NO_LIMIT), (0, 6, 0, [0, 5], 3)):
        rc, k, sm = rt.skeletonField(set, conn, mode, anchors, m)
        wrc, want, wsm = vg.skeletonField(set, conn, mode, anchors, m)
        assert rc == wrc == 0 and np.array_equal(k, want) and sm.tobytes() == wsm.tobytes() and sm["removed"] > 0
    a, b = 0, data.size - 1
    assert data.reshape(-1)[a] == 0 and data.reshape(-1)[b] == 0
    rc, line = rt.centreline(a, b)
    want = vg.skeletonField(0, 26, 0, [a, b])[1]
    assert rc == 0 and np.array_equal(line, np.flatnonzero(want.reshape(-1) == 0)) and a in line and b in line
    assert np.array_equal(rt.grid(), data)                              # centreline edits nothing
    edit = rto.VoxelGrid.from_array(data, g.min, g.voxel_size)
    changed = edit.thin(1, 26, 1)
    assert rt.thin() == changed > 0
    assert np.array_equal(rt.grid(), edit.data)
    assert rt.thin() == 0
    assert np.array_equal(rt.grid(), edit.data)
