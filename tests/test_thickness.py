"""Local thickness fields (rto_thickness_field, rto_download_thickness, rto_thickness_device, rto_thickness_histogram,
rto_last_thickness_ms, Context.thickness_field, RayTracerBVH::thicknessField / thinnestPoint / thicknessHistogram).  CPU: the numpy
rule (tests/thickness_ref.py) stated twice, the closed form of a slab, invariants, the host layer's comparator, the ABI, the kernels'
budgets, the sanitizer script.  GPU: field, histogram and summary bit for bit against the rule for both media at radii of 1, 1.5, 2,
4 and 8 voxels (c = 1, 2, 4, 16, 64) on grids chosen around k_thick_gather's tile and halo; state and errors."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import distance_ref as dr
import thickness_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("rto_thickness_field", "rto_download_thickness", "rto_thickness_device", "rto_thickness_histogram", "rto_last_thickness_ms",
        "rto_debug_thickness_table")
MEDIA = (tr.SET_SOLID, tr.SET_EMPTY)
RADII_VOX = (1.0, 1.5, 2.0, 4.0, 8.0)
CAPS = (1, 2, 4, 16, 64)                          # c of those radii
# what the build gives: VGPRs, and LDS bytes per workgroup
THICK_VGPR = {"k_thick_gather": 58, "k_thick_summary": 12}
THICK_LDS = {"k_thick_gather": 22544, "k_thick_summary": 304}
GATHER_BLOCK_BYTES = 46 * 22 * 22                 # the tile and a halo of 7 voxels, as bytes


def _hip():
    from ray_tracing_octrees_amd import hip
    return hip


def _tc():
    import test_components as tc          # its checks of a context and its device copy
    return tc


def _mq(r_vox):
    return int(np.floor(r_vox * 64.0 + 0.5))


# ================================================================ grids
def _random(shape_xyz, fill, seed):
    x, y, z = shape_xyz
    return (np.random.default_rng(seed).random((z, y, x)) < fill).astype(np.uint8)


SEEDED = {f"r{x}x{y}x{z}_{fill}": ((x, y, z), fill / 100.0, 1000 + x + fill)
          for (x, y, z) in ((31, 7, 7), (32, 8, 8), (33, 9, 9), (65, 17, 17), (5, 3, 2)) for fill in (80, 90)}
SLAB_DIMS = {0: (48, 10, 10), 1: (10, 24, 10), 2: (10, 10, 24)}     # (dimX, dimY, dimZ); the tile face is at x = 32, y = 8, z = 8
SLAB_FACE = {0: 32, 1: 8, 2: 8}


def _slab(axis, w):
    """A wall w voxels wide across the whole grid, straddling the first tile face of `axis` (w = 1: the voxel in front of it)."""
    dx, dy, dz = SLAB_DIMS[axis]
    g = np.zeros((dz, dy, dx), np.uint8)
    a0 = SLAB_FACE[axis] - (w + 1) // 2
    sl = [slice(None)] * 3
    sl[2 - axis] = slice(a0, a0 + w)
    g[tuple(sl)] = 1
    return g


def _cube(centre):
    """A 15 x 15 x 15 cube about `centre` (x, y, z) in 65 x 33 x 33."""
    g = np.zeros((33, 33, 65), np.uint8)
    x, y, z = centre
    g[z - 7:z + 8, y - 7:y + 8, x - 7:x + 8] = 1
    return g


CUBES = {"cube_last": (31, 15, 15), "cube_first": (32, 16, 16)}    # the centre is the last / the first voxel of a tile on every axis


def _shell40():
    """The voxels of a 40^3 grid whose centres lie between radii 12 and 15 of the grid's centre."""
    a = np.arange(40, dtype=np.float64) + 0.5 - 20.0
    r2 = a[:, None, None] ** 2 + a[None, :, None] ** 2 + a[None, None, :] ** 2
    return ((r2 >= 144.0) & (r2 <= 225.0)).astype(np.uint8)


def _named_grid(name, scenes=None):
    if name in SEEDED:
        return _random(*SEEDED[name])
    if name in CUBES:
        return _cube(CUBES[name])
    if name.startswith("slab"):
        return _slab(int(name[4]), int(name[6:]))
    if name == "shell40":
        return _shell40()
    if name == "full":
        return np.ones((12, 20, 40), np.uint8)
    if name == "empty":
        return np.zeros((12, 20, 40), np.uint8)
    return np.ascontiguousarray(scenes(name).grid.data, np.uint8)


SMALL = lambda name: name in SEEDED or name.startswith("slab") or name in ("full", "empty")    # noqa: E731  (brute-force D)
_D, _REF = {}, {}


def _radius(name, grid, medium):
    """The unclipped d2 to the other set, once per (grid, medium): distance_ref's brute force on the small grids, its separable form
    (in reach of 8 voxels: what lies beyond clips to c anyway) on the others."""
    key = (name, medium)
    if key not in _D:
        d = dr.brute_force(grid, 1 - medium) if SMALL(name) else dr.separable(grid, 1 - medium, 512)
        d.setflags(write=False)
        _D[key] = d
    return _D[key]


def _ref(name, grid, medium, c):
    """(t2, bins, summary) of the rule, computed once and shared."""
    key = (name, medium, c)
    if key not in _REF:
        D = tr.clipped_radius(grid, medium, c, lambda g, s: _radius(name, grid, medium))
        t2 = tr.gather(D, c, np.int64 if grid.size < 500000 else np.uint8)
        t2.setflags(write=False)
        _REF[key] = (t2, tr.histogram(t2, c), tr.summary(t2, c))
    return _REF[key]


# ================================================================ CPU: the rule
def test_rule_caps():
    vs = np.float32(1.0 / 64)
    for r, c in zip(RADII_VOX, CAPS):
        assert tr.cap(np.float32(r) * vs, vs) == c == tr.cap_of_quanta(_mq(r))
    assert tr.cap(np.float32(8.05) * vs, vs) == 64                      # 515 quanta: floor(515^2 / 4096) = 64
    for bad in (np.nan, -1.0, 0.0, float(np.float32(0.99) * vs), 1e9):
        with pytest.raises(ValueError) as e:
            tr.cap(bad, vs)
        assert not isinstance(e.value, tr.Unsupported), bad
    for far in (np.inf, float(np.float32(8.2) * vs), float(np.float32(100.0) * vs)):
        with pytest.raises(tr.Unsupported):
            tr.cap(far, vs)
    assert [tr.isqrt_below(c) for c in (1, 2, 4, 5, 16, 17, 64)] == [0, 1, 1, 2, 3, 4, 7]
    assert len(tr.offsets(64)) == 2103 and len(tr.offsets(16)) == 251 and tr.offsets(1) == [(0, 0, 0, 0)]


@pytest.mark.parametrize("name", ["r5x3x2_80", "r5x3x2_90", "r31x7x7_80", "r31x7x7_90", "r33x9x9_90", "slab0_5"])
def test_rule_two_statements_agree(name):
    g = _named_grid(name)
    for m in MEDIA:
        for c in CAPS:
            D = tr.clipped_radius(g, m, c)
            a = tr.gather(D, c)
            assert np.array_equal(a, tr.scatter(D, c)), (name, m, c)
            assert np.array_equal(a, tr.gather(D, c, np.uint8)), (name, m, c)
            assert np.array_equal(a, _ref(name, g, m, c)[0])


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_rule_slab_closed_form(axis):
    """A wall w voxels wide holds min(((w + 1) div 2)^2, c) throughout, as material and as a gap."""
    for w in range(1, 10):
        g = _slab(axis, w)
        for c in (16, 64):
            want = min(((w + 1) // 2) ** 2, c)
            t2 = tr.field(g, tr.SET_SOLID, c)
            assert (t2[g == 1] == want).all() and (t2[g == 0] == 0).all(), (axis, w, c)
            gap = tr.field(1 - g, tr.SET_EMPTY, c)
            assert np.array_equal(gap, t2), (axis, w, c)


@pytest.mark.parametrize("name", sorted(SEEDED))
def test_rule_invariants(name):
    g = _named_grid(name)
    for m in MEDIA:
        for c in CAPS:
            t2, bins, sm = _ref(name, g, m, c)
            D = np.minimum(_radius(name, g, m).astype(np.int64), c)
            med = g == m
            assert t2.dtype == np.int32 and (t2 >= D).all()
            assert (t2[med] >= 1).all() and (t2[med] <= c).all() and (t2[~med] == 0).all()
            assert bins[0] == 0 and bins.sum() == med.sum() == sm["medium"] and sm["thin"] == bins[:c].sum()
            if c > 1:
                lower = _ref(name, g, m, CAPS[CAPS.index(c) - 1])[0]
                assert (np.minimum(t2, CAPS[CAPS.index(c) - 1]) >= lower).all()      # the capped field is never higher than the clipped larger one


def test_rule_full_and_empty_grids():
    full, empty = _named_grid("full"), _named_grid("empty")
    for c in CAPS:
        for g, m in ((full, tr.SET_SOLID), (empty, tr.SET_EMPTY)):      # all medium: nothing to measure from, c everywhere
            t2 = tr.field(g, m, c)
            assert (t2 == c).all()
            sm = tr.summary(t2, c)
            assert (sm["min_t2"], sm["argmin"], sm["thin"], sm["medium"]) == (c, 0, 0, g.size)
            assert tr.histogram(t2, c)[c] == g.size
        for g, m in ((full, tr.SET_EMPTY), (empty, tr.SET_SOLID)):      # no medium
            t2 = tr.field(g, m, c)
            assert (t2 == 0).all() and tr.histogram(t2, c).sum() == 0
            sm = tr.summary(t2, c)
            assert (sm["min_t2"], sm["argmin"], sm["thin"], sm["medium"]) == (-1, -1, 0, 0)


def test_rule_shell_and_cube_values():
    g = _shell40()
    t2 = _ref("shell40", g, tr.SET_SOLID, 64)[0]
    assert sorted(np.unique(t2[g == 1])) == [2, 3, 4, 5]
    for name, (x, y, z) in CUBES.items():
        gc = _named_grid(name)
        assert np.minimum(_radius(name, gc, tr.SET_SOLID), 64)[z, y, x] == 64
        assert (x % 32, y % 8, z % 8) in ((31, 7, 7), (0, 0, 0))
        t = _ref(name, gc, tr.SET_SOLID, 64)[0]
        assert t[z, y, x] == 64 and t[z, y, x + 7] == 64 and t[z - 7, y - 7, x - 7] < 64


HOST_GRIDS = [*sorted(SEEDED), *sorted(CUBES), *[f"slab{a}_{w}" for a in (0, 1, 2) for w in range(1, 10)], "shell40", "full", "empty"]


def _check_host(name, g, radii=RADII_VOX):
    import ray_tracing_octrees_amd as rto
    vg = rto.VoxelGrid.from_array(g, (0.0, 0.0, 0.0), 1.0)
    for m in MEDIA:
        for r in radii:
            c = tr.cap_of_quanta(_mq(r))
            want, wbins, wsm = _ref(name, g, m, c)
            rc, t2, bins, sm = vg.thicknessField(m, _mq(r))
            assert rc == 0 and np.array_equal(t2, want), (name, m, c)
            assert np.array_equal(bins, wbins) and sm.tobytes() == wsm.tobytes(), (name, m, c, sm, wsm)
    return vg


@pytest.mark.parametrize("name", HOST_GRIDS)
def test_reference_equals_the_host_layers_comparator(name):
    """tests/thickness_ref.py against thicknessFieldCPU (host/Thickness.cpp)."""
    hip = _hip()
    vg = _check_host(name, _named_grid(name))
    for bad, code in (((2, 64), hip.RTO_E_INVALID), ((-1, 64), hip.RTO_E_INVALID), ((1, -1), hip.RTO_E_INVALID), ((1, 0), hip.RTO_E_INVALID),
                      ((1, 63), hip.RTO_E_INVALID), ((1, (1 << 28) + 1), hip.RTO_E_INVALID), ((1, 516), hip.RTO_E_UNSUPPORTED),
                      ((0, 1 << 28), hip.RTO_E_UNSUPPORTED)):
        rc, t2, bins, _ = vg.thicknessField(*bad)
        assert rc == code and t2 is None and bins is None, bad
    assert vg.thicknessField(1, 515)[0] == 0                           # floor(515^2 / 4096) = 64, floor(516^2 / 4096) = 65


def test_host_layer_calgary(scenes):
    g = _named_grid("calgary", scenes)
    _check_host("calgary", g, (4.0,))


def test_thickness_abi_layout_and_exports():
    """sizeof(rto_thick_summary) == 32 with the fields where THICK_SUMMARY_DTYPE puts them; the constant; the new symbols are exported."""
    hip = _hip()
    assert hip.THICK_SUMMARY_DTYPE.itemsize == 32 and tr.SUMMARY_DTYPE == hip.THICK_SUMMARY_DTYPE
    fields = ("min_t2", "argmin", "thin", "medium")
    assert [hip.THICK_SUMMARY_DTYPE.fields[f][1] for f in fields] == [0, 8, 16, 24]
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.fail("no C compiler: the header's layout cannot be checked")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "abi.c")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "rto_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d %d %d\\n", '
                    'sizeof(rto_thick_summary), offsetof(rto_thick_summary, min_t2), offsetof(rto_thick_summary, argmin), '
                    'offsetof(rto_thick_summary, thin), offsetof(rto_thick_summary, medium), RTO_THICK_MAX_C, RTO_SET_SOLID, RTO_SET_EMPTY); '
                    'return 0; }\n')
        exe = os.path.join(tmp, "abi")
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert out == [str(v) for v in (32, 0, 8, 16, 24, hip.THICK_MAX_C, hip.SET_SOLID, hip.SET_EMPTY)]
    assert (tr.MAX_C, tr.SET_SOLID, tr.SET_EMPTY) == (hip.THICK_MAX_C, hip.SET_SOLID, hip.SET_EMPTY) == (64, 1, 0)
    L = hip.load()
    header = open(os.path.join(ROOT, "include", "rto_hip.h")).read()
    for s in SYMS:
        assert s in hip.SYMBOLS and hasattr(L, s), s
        assert s + "(" in header, s
    for m in ("thickness_field", "thickness", "thickness_device", "thickness_histogram", "last_thickness_ms"):
        assert callable(getattr(hip.Context, m)), m


def _lds_bytes(asm_text):
    md = asm_text[asm_text.index(".amdgpu_metadata"):]
    return {m.group(2): int(m.group(1)) for m in re.finditer(r"\.group_segment_fixed_size: (\d+)\n(?:(?!\.group_segment_fixed_size).)*?\.name:\s+(\S+)\n", md, re.S)}


def test_thickness_kernels_keep_their_budgets():
    """The built assembly (the product's flags): two k_thick_* kernels, without scratch, spills or v_mfma, at the VGPR counts and LDS
    sizes DESIGN.md section 21 states; the gather holds its block as bytes (46 x 22 x 22 of them), reads it with byte loads and its
    offset table with scalar loads."""
    import test_isa_contract as isa
    asm = isa.built_asm()
    if asm is None:
        pytest.fail("no hipcc: the budget cannot be checked")
    meta = isa.kernel_meta(asm)
    lds = _lds_bytes(asm)
    names = [k for k in meta if "k_thick_" in k]
    assert len(names) == 2, names                # gather, summary: no template forms
    seen = set()
    for k in names:
        m = meta[k]
        base = next(b for b in THICK_VGPR if b in k)
        seen.add(base)
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (k, m)
        assert m["vgpr"] <= THICK_VGPR[base], (k, m)
        assert lds[k] <= THICK_LDS[base], (k, lds[k])
        ins = isa.body(asm, k[len("_ZN3rto"):])
        assert not any(t.startswith(("scratch_", "buffer_load", "buffer_store")) or "v_mfma" in t for t in ins), k
    assert seen == set(THICK_VGPR)
    g = next(k for k in names if "k_thick_gather" in k)
    assert GATHER_BLOCK_BYTES <= lds[g] < GATHER_BLOCK_BYTES + 512
    ins = isa.body(asm, g[len("_ZN3rto"):])
    assert sum(t.startswith("ds_read_u8") for t in ins) >= 8 and any(t.startswith("ds_write_b8") for t in ins)
    assert any(t.startswith("s_load_dwordx4") for t in ins)             # the offsets, four at a time
    s = next(k for k in names if "k_thick_summary" in k)
    ins = isa.body(asm, s[len("_ZN3rto"):])
    assert any(t.startswith("ds_add_u32") for t in ins) and any(t.startswith("global_atomic_umin_x2") for t in ins)


def test_sanitizer_script_reports_nothing():
    """tools/sanitize_thickness.sh: host/Thickness.cpp as a stand-alone program under AddressSanitizer and UBSan."""
    if not shutil.which("g++"):
        pytest.fail("no g++: the sanitizer build cannot be made")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize_thickness.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "thickness selftest ok" in r.stdout and "UBSan reports: 0" in r.stdout and "ASan reports: 0" in r.stdout, r.stdout


# ================================================================ GPU
gpu = pytest.mark.gpu
W, H, FOV = 128, 96, 45.0
GMIN, VOX = np.array([-0.5, -0.5, -0.5], np.float32), np.float32(1.0 / 64)


def _build(ctx, grid, gmin=GMIN, vox=VOX):
    ctx.set_kernel(_hip().KERNEL_AUTO)
    ctx.build_octree(grid, gmin, vox)


def _check_fields(ctx, name, g, vox, radii=RADII_VOX):
    for m in MEDIA:
        for r in radii:
            radius = np.float32(r) * np.float32(vox)
            c = tr.cap(radius, vox)
            assert c == tr.cap_of_quanta(_mq(r)), (r, vox)
            want, wbins, wsm = _ref(name, g, m, c)
            what = f"{name} medium {m} c {c}"
            got, gs = ctx.thickness_field(m, radius)
            assert got.dtype == np.int32 and got.shape == g.shape, what
            assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} voxels differ"
            bins = ctx.thickness_histogram()
            assert bins.dtype == np.int64 and np.array_equal(bins, wbins), (what, bins, wbins)
            assert gs.tobytes() == wsm.tobytes(), (what, gs, wsm)
            assert all(t >= 0 for t in ctx.last_thickness_ms()), what


FIELD_GRIDS = [*sorted(SEEDED), *sorted(CUBES), "shell40", "full", "empty"]


@gpu
@pytest.mark.parametrize("name", FIELD_GRIDS)
def test_gpu_field_histogram_and_summary_equal_the_rule(ctx, name):
    g = _named_grid(name)
    _build(ctx, g)
    _check_fields(ctx, name, g, VOX)


@gpu
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_gpu_slabs_across_a_tile_face(ctx, axis):
    for w in range(1, 10):
        name = f"slab{axis}_{w}"
        g = _named_grid(name)
        _build(ctx, g)
        _check_fields(ctx, name, g, VOX)
        got, _ = ctx.thickness_field(tr.SET_SOLID, np.float32(8.0) * VOX)
        assert (got[g == 1] == ((w + 1) // 2) ** 2).all(), (axis, w)


@gpu
def test_gpu_field_of_calgary_equals_the_rule(ctx, scenes):
    sc = scenes("calgary").grid
    g = np.ascontiguousarray(sc.data, np.uint8)
    ctx.set_kernel(_hip().KERNEL_AUTO)
    ctx.build_octree(g, sc.min, sc.voxel_size)
    _check_fields(ctx, "calgary", g, np.float32(sc.voxel_size), (4.0,))


@gpu
def test_gpu_offset_table_is_kept_per_cap_and_never_stale():
    """The gather's table is built once per c and kept across calls, media and grids; a change of c builds another, and going back
    builds again.  Every call equals the rule, so a table of the wrong c would show."""
    hip = _hip()
    c = hip.Context(0)
    try:
        assert c.thickness_table() == (0, 0)
        a, b = "r65x17x17_80", "r33x9x9_90"
        ga, gb = _named_grid(a), _named_grid(b)
        steps = [(a, ga, 4.0, 16, 1), (a, ga, 4.0, 16, 1), (b, gb, 4.0, 16, 1), (b, gb, 8.0, 64, 2), (a, ga, 8.0, 64, 2), (a, ga, 2.0, 4, 3),
                 (a, ga, 4.0, 16, 4), (a, ga, 4.0, 16, 4)]
        for name, g, r, cap, built in steps:
            _build(c, g)                                                 # a new grid drops the field, not the table
            for m in MEDIA:
                got, gs = c.thickness_field(m, np.float32(r) * VOX)
                want, wbins, wsm = _ref(name, g, m, cap)
                assert np.array_equal(got, want) and np.array_equal(c.thickness_histogram(), wbins) and gs.tobytes() == wsm.tobytes(), (name, r, m)
                assert c.thickness_table() == (cap, built), (name, r, m, c.thickness_table())
        with pytest.raises(hip.RtoError):
            c.thickness_field(tr.SET_SOLID, np.float32(0.5) * VOX)       # a refusal builds nothing
        assert c.thickness_table() == (16, 4)
    finally:
        c.close()


@gpu
def test_gpu_thickness_device_pointer_holds_the_download(ctx):
    name = "r33x9x9_80"
    g = _named_grid(name)
    _build(ctx, g)
    got, _ = ctx.thickness_field(tr.SET_SOLID, np.float32(4.0) * VOX)
    p = ctx.thickness_device()
    assert p and _tc()._d2h(p, 4 * g.size).tobytes() == got.tobytes() == _ref(name, g, tr.SET_SOLID, 16)[0].tobytes()
    assert ctx.thickness().tobytes() == got.tobytes()


@gpu
def test_gpu_thickness_leaves_a_resident_euclidean_field_alone(ctx):
    name = "r65x17x17_80"
    g = _named_grid(name)
    _build(ctx, g)
    for s, max_dist in ((dr.SET_SOLID, np.inf), (dr.SET_EMPTY, np.float32(2.5) * VOX)):
        field, _ = ctx.distance_field(s, max_dist)
        p = ctx.distance_device()
        for m in MEDIA:
            ctx.thickness_field(m, np.float32(4.0) * VOX)
            assert ctx.distance_device() == p and ctx.distance().tobytes() == field.tobytes(), (s, m)
            assert _tc()._d2h(p, 4 * g.size).tobytes() == field.tobytes()


@gpu
def test_gpu_thickness_is_dropped_by_a_change_and_survives_none(ctx, scenes):
    hip = _hip()
    g = scenes("sphere64").grid

    def gone():
        for read in (ctx.thickness, ctx.thickness_device, ctx.thickness_histogram):
            with pytest.raises(hip.RtoError) as e:
                read()
            assert e.value.code == hip.RTO_E_INVALID and "no thickness field is resident" in str(e.value)

    radius = np.float32(2.0) * np.float32(g.voxel_size)
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    gone()                                                              # never made
    field, _ = ctx.thickness_field(tr.SET_SOLID, radius)
    bins = ctx.thickness_histogram()
    corner_centre = np.asarray(g.min, np.float32) + np.float32(0.5) * g.voxel_size
    carve = hip.make_brushes([corner_centre], 0.5 * float(g.voxel_size), hip.BRUSH_SPHERE, hip.EDIT_CARVE)
    assert ctx.edit_voxels(carve) == 0                                  # the corner is empty already: changed = 0
    assert ctx.edit_morphology(hip.MORPH_DILATE, 0.0) == 0
    assert np.array_equal(ctx.thickness(), field) and np.array_equal(ctx.thickness_histogram(), bins)
    fill = hip.make_brushes([corner_centre], 0.5 * float(g.voxel_size), hip.BRUSH_SPHERE, hip.EDIT_FILL)
    assert ctx.edit_voxels(fill) == 1                                   # changed > 0
    gone()
    ctx.thickness_field(tr.SET_EMPTY, radius)
    assert ctx.edit_components(1, 6, hip.SELECT_SMALLER_THAN, 2) == 1   # the corner voxel is debris
    gone()
    ctx.thickness_field(tr.SET_SOLID, radius)
    assert ctx.edit_morphology(hip.MORPH_DILATE, g.voxel_size) > 0
    gone()
    ctx.thickness_field(tr.SET_SOLID, radius)
    ctx.build_octree(g.data, g.min, g.voxel_size)                       # a new grid
    gone()
    ctx.thickness_field(tr.SET_SOLID, radius)
    ctx.upload_octree(scenes("sphere64").nodes, g.min, g.voxel_size)    # no grid at all
    gone()


@gpu
def test_gpu_thickness_refusals_leave_the_context_untouched(ctx, orc, scenes):
    from conftest import make_camera
    hip = _hip()
    tc = _tc()
    sc = scenes("sphere64")
    g = sc.grid
    vs = np.float32(g.voxel_size)
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    labels_table = ctx.label_components(1, 6)
    labels = ctx.component_labels()
    dist, _ = ctx.distance_field(dr.SET_SOLID)
    geo, _ = ctx.geodesic_field([0], hip.SET_EMPTY, hip.CONN_FACE)
    thick, _ = ctx.thickness_field(tr.SET_SOLID, np.float32(4.0) * vs)
    bins = ctx.thickness_histogram()
    ms = ctx.last_thickness_ms()
    table = ctx.thickness_table()
    nodes, info = ctx.download_nodes(), bytes(ctx.info())
    view, pos = make_camera(orc, 0.5, 0.7, 1.8)
    L, h = ctx._L, ctx._h
    small = np.zeros(g.data.size - 1, np.int32)
    few = np.zeros(16, np.int64)
    too_far = float(vs * np.float32(2.0 ** 22 + 1))
    INV, UNS = hip.RTO_E_INVALID, hip.RTO_E_UNSUPPORTED
    cases = [
        ("unknown medium", INV, lambda: L.rto_thickness_field(h, 2, float(vs), None)),
        ("negative medium", INV, lambda: L.rto_thickness_field(h, -1, float(vs), None)),
        ("unknown medium before a radius above 8 voxels", INV, lambda: L.rto_thickness_field(h, 2, float("inf"), None)),
        ("NaN radius", INV, lambda: L.rto_thickness_field(h, 1, float("nan"), None)),
        ("negative radius", INV, lambda: L.rto_thickness_field(h, 1, -1.0, None)),
        ("-inf radius", INV, lambda: L.rto_thickness_field(h, 0, float("-inf"), None)),
        ("radius beyond 2^28 quanta", INV, lambda: L.rto_thickness_field(h, 1, too_far, None)),
        ("radius 0", INV, lambda: L.rto_thickness_field(h, 1, 0.0, None)),
        ("radius under one voxel", INV, lambda: L.rto_thickness_field(h, 0, float(np.float32(0.99) * vs), None)),
        ("radius above 8 voxels", UNS, lambda: L.rto_thickness_field(h, 1, float(np.float32(8.2) * vs), None)),
        ("infinite radius", UNS, lambda: L.rto_thickness_field(h, 0, float("inf"), None)),
        ("field capacity", INV, lambda: L.rto_download_thickness(h, small.ctypes.data, g.data.size - 1)),
        ("histogram capacity", INV, lambda: L.rto_thickness_histogram(h, few.ctypes.data, 16, None)),
    ]
    for what, code, call in cases:
        assert call() == code, what
        assert L.rto_last_error(h), what
        assert ctx.download_nodes().tobytes() == nodes.tobytes() and bytes(ctx.info()) == info, what
        assert np.array_equal(ctx.download_voxels(), g.data), what
        assert np.array_equal(ctx.thickness(), thick) and np.array_equal(ctx.thickness_histogram(), bins), what
        assert ctx.last_thickness_ms() == ms, what
        assert ctx.thickness_table() == table, what
        assert np.array_equal(ctx.distance(), dist) and np.array_equal(ctx.geodesic(), geo), what
        assert np.array_equal(ctx.component_labels(), labels) and ctx.components().tobytes() == labels_table.tobytes(), what
    tc._check_render(ctx, orc, g, sc.nodes, view, pos, "the frame after the refusals")
    # a grid the 32-bit transform cannot serve: dt_check_grid's refusal
    line = np.zeros((1, 1, 46342), np.uint8)
    line[0, 0, 0] = 1
    _build(ctx, line, np.zeros(3, np.float32), np.float32(1.0))
    with pytest.raises(hip.RtoError) as e:
        ctx.thickness_field(tr.SET_SOLID, 2.0)
    assert e.value.code == UNS and "diagonal" in str(e.value)
    assert np.array_equal(ctx.download_voxels(), line)
    # no resident grid, no octree
    ctx.upload_octree(sc.nodes, g.min, g.voxel_size)
    with pytest.raises(hip.RtoError) as e:
        ctx.thickness_field(tr.SET_SOLID, np.float32(2.0) * vs)
    assert e.value.code == UNS
    assert L.rto_thickness_field(h, 2, float(vs), None) == INV            # an unknown medium is reported before the missing grid
    assert L.rto_thickness_field(h, 1, 0.0, None) == INV                  # and so is a radius under one voxel
    tc._check_render(ctx, orc, g, sc.nodes, view, pos, "the frame after the refusals (uploaded octree)")
    fresh = hip.Context(0)
    try:
        with pytest.raises(hip.RtoError) as e:
            fresh.thickness_field(tr.SET_SOLID, 1.0)
        assert e.value.code == hip.RTO_E_NO_OCTREE
        assert fresh._L.rto_thickness_field(fresh._h, 7, 1.0, None) == INV
        ms3 = (C.c_float * 3)()
        assert fresh._L.rto_last_thickness_ms(fresh._h, ms3) == 0 and tuple(ms3) == (-1.0, -1.0, -1.0)
    finally:
        fresh.close()
    with pytest.raises(ValueError):
        ctx.thickness_field(tr.SET_SOLID)                               # the radius has no default


@gpu
def test_gpu_host_class_thickness(scenes):
    import ray_tracing_octrees_amd as rto
    hip = _hip()
    g = scenes("sphere64").grid
    data = np.ascontiguousarray(g.data, np.uint8)
    vs = np.float32(g.voxel_size)
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    assert rt.thicknessField(1, 1.0)[0] == hip.RTO_E_NO_OCTREE and rt.thinnestPoint(1, 1.0)[0] == hip.RTO_E_NO_OCTREE
    rt.setOctreeFromGrid(rto.VoxelGrid.from_array(data, g.min, g.voxel_size))
    assert rt.thicknessHistogram()[0] == hip.RTO_E_INVALID              # none made yet
    for m in MEDIA:
        want, wbins, wsm = _ref("sphere64", data, m, 16)
        rc, t2, sm = rt.thicknessField(m, float(np.float32(4.0) * vs))
        assert rc == 0 and np.array_equal(t2, want) and sm.tobytes() == wsm.tobytes()
        rc, bins = rt.thicknessHistogram()
        assert rc == 0 and np.array_equal(bins, wbins)
        rc, thin = rt.thinnestPoint(m, float(np.float32(4.0) * vs))
        assert rc == 0 and thin is not None
        (i, j, k), t, n_thin, width = thin
        assert t == wsm["min_t2"] and i + 64 * (j + 64 * k) == wsm["argmin"] and n_thin == wsm["thin"]
        assert abs(width - 2.0 * np.sqrt(float(t)) * float(vs)) < 1e-12
    assert rt.thicknessField(2, float(vs))[0] == hip.RTO_E_INVALID and rt.thicknessField(1, float("nan"))[0] == hip.RTO_E_INVALID
    assert rt.thicknessField(1, float("inf"))[0] == hip.RTO_E_UNSUPPORTED and rt.thinnestPoint(0, 0.0)[0] == hip.RTO_E_INVALID
    assert np.array_equal(rt.grid(), data)
