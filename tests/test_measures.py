"""Component measures (rto_measure_components, rto_download_measures, rto_measures_device, rto_last_measure_ms,
Context.measure_components / component_measures / topology, hip.measure_physical, measureComponentsCPU, RayTracerBVH::measureComponents
/ surfaceArea / centroid / topology).  CPU: the numpy rule (tests/measure_ref.py) stated twice, closed forms, invariants, topology
against scipy, the host layer's comparator, measure_physical, the ABI, the kernels' budgets, the sanitizer script.  GPU: table and
total bit for bit against the rule for both sets and both connectivities on grids chosen around k_measure's tile and halo; state and
errors."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import component_ref as cr
import measure_ref as mr
from test_components import CONNS, GMIN, SETS, TILE, VOX, _box_mesh, _build, _checkerboard, _corner_slabs, ctx2, path   # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("rto_measure_components", "rto_download_measures", "rto_measures_device", "rto_last_measure_ms")
# what the build gives; a kernel that grows past its line here has changed
MS_VGPR = {"k_measureILb1ELb1E": 56, "k_measureILb1ELb0E": 56, "k_measureILb0ELb1E": 56, "k_measureILb0ELb0E": 56, "k_measure_fold": 58,
           "k_measure_total": 88}
MS_LDS = {"k_measureI": 1120, "k_measure_fold": 656, "k_measure_total": 640}


def _hip():
    from ray_tracing_octrees_amd import hip
    return hip


def _same(got, want, what):
    gt, gtot = got
    wt, wtot = want
    assert gt.dtype == wt.dtype and len(gt) == len(wt), f"{what}: {len(gt)} records vs {len(wt)}"
    for f in mr.MEASURE_DTYPE.names:
        assert np.array_equal(gt[f], wt[f]), f"{what}: table field {f}, first at record {int(np.argwhere(gt[f] != wt[f])[0][0])}"
        assert np.array_equal(gtot[f], wtot[f]), f"{what}: total field {f}: {gtot[f]} vs {wtot[f]}"


# ================================================================ grids
def _cube():
    g = np.zeros((7, 7, 7), np.uint8)
    g[1:6, 1:6, 1:6] = 1
    return g


def _shell():
    g = _cube()
    g[3, 3, 3] = 0
    return g


def _ring():
    g = np.zeros((3, 7, 7), np.uint8)
    g[1, 1:6, 1:6] = 1
    g[1, 2:5, 2:5] = 0
    return g


def _corner_pair():
    g = np.zeros((4, 4, 4), np.uint8)
    g[1, 1, 1] = g[2, 2, 2] = 1
    return g


def _frame():
    """The 12 edges of a 9^3 cube."""
    g = np.zeros((11, 11, 11), np.uint8)
    c = g[1:10, 1:10, 1:10]
    for a in (0, 8):
        for b in (0, 8):
            c[a, b, :] = c[a, :, b] = c[:, a, b] = 1
    return g


def _linked_rings():
    g = np.zeros((9, 9, 12), np.uint8)
    g[4, 1:8, 1:8] = 1                     # a ring in the plane z = 4 ...
    g[4, 2:7, 2:7] = 0
    h = np.zeros_like(g)
    h[1:8, 4, 4:11] = 1                    # ... and one in the plane y = 4 through its hole
    h[2:7, 4, 5:10] = 0
    return g | h


def _random(shape_xyz, fill, seed):
    x, y, z = shape_xyz
    return (np.random.default_rng(seed).random((z, y, x)) < fill).astype(np.uint8)


def _at_tile_corner(kind):
    """A shape centred on the corner (32, 8, 8) shared by eight tiles, in a grid of 2 x 2 x 2 tiles."""
    g = np.zeros((2 * TILE[2], 2 * TILE[1], 2 * TILE[0]), np.uint8)
    cx, cy, cz = TILE
    if kind == "block":
        g[cz - 1:cz + 1, cy - 1:cy + 1, cx - 1:cx + 1] = 1
    else:                                   # a 6 x 6 ring, two voxels thick along z, and the same turned into the other two planes
        g[cz - 1:cz + 1, cy - 3:cy + 3, cx - 3:cx + 3] = 1
        g[cz - 1:cz + 1, cy - 2:cy + 2, cx - 2:cx + 2] = 0
        if kind == "rings3":
            h = np.zeros_like(g)
            h[cz - 3:cz + 3, cy - 1:cy + 1, cx - 3:cx + 3] = 1
            h[cz - 2:cz + 2, cy - 1:cy + 1, cx - 2:cx + 2] = 0
            g |= h
            h[:] = 0
            h[cz - 3:cz + 3, cy - 3:cy + 3, cx - 1:cx + 1] = 1
            h[cz - 2:cz + 2, cy - 2:cy + 2, cx - 1:cx + 1] = 0
            g |= h
    return g


def _face_slab(d):
    """A one-voxel slab on grid face d (-x, +x, -y, +y, -z, +z) of a 34 x 10 x 9 grid."""
    g = np.zeros((9, 10, 34), np.uint8)
    index = [slice(None)] * 3
    index[2 - d // 2] = -1 if d % 2 else 0
    g[tuple(index)] = 1
    return g


RANDOM_GRIDS = {f"random_{x}x{y}x{z}_{int(fill * 100)}": ((x, y, z), fill, 300 + i)
                for i, ((x, y, z), fill) in enumerate([(s, f) for s in ((31, 7, 7), (32, 8, 8), (33, 9, 9), (65, 17, 17), (5, 3, 2), (1, 1, 1))
                                                       for f in (0.2, 0.5, 0.8)])}
NAMED = {"cube": _cube, "shell": _shell, "ring": _ring, "corner_pair": _corner_pair, "frame": _frame, "linked_rings": _linked_rings,
         "full": lambda: np.ones((12, 20, 40), np.uint8), "empty": lambda: np.zeros((12, 20, 40), np.uint8),
         "checkerboard33": lambda: _checkerboard(33), "corner_block": lambda: _at_tile_corner("block"),
         "corner_ring": lambda: _at_tile_corner("ring"), "corner_rings3": lambda: _at_tile_corner("rings3"), "corner_slabs": _corner_slabs,
         "full_4096x2x2": lambda: np.ones((2, 2, 4096), np.uint8), "row_32768": lambda: np.ones((1, 1, 32768), np.uint8),
         **{f"face_slab_{d}": (lambda d=d: _face_slab(d)) for d in range(6)}}


def _named_grid(name, scenes=None):
    if name in RANDOM_GRIDS:
        return _random(*RANDOM_GRIDS[name])
    if name in NAMED:
        return NAMED[name]()
    return np.ascontiguousarray(scenes(name).grid.data, np.uint8)


_REF = {}


def _ref(name, grid, s, conn):
    """The rule's answer (labels, component table, measure table, total), computed once per (grid, set, connectivity) and shared."""
    key = (name, s, conn)
    if key not in _REF:
        out = mr.measure_grid(grid, s, conn)
        for a in out:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


# ================================================================ the rule (CPU)
SMALL = ["cube", "shell", "ring", "corner_pair", "frame", "linked_rings", "corner_block", "corner_rings3", "random_5x3x2_50",
         "random_1x1x1_80", "random_31x7x7_20", "random_33x9x9_50", "random_65x17x17_20", "random_65x17x17_80"]


@pytest.mark.parametrize("name", SMALL)
def test_the_two_statements_of_the_rule_agree(name):
    g = _named_grid(name)
    for s in SETS:
        for conn in CONNS:
            labels, comps, table, total = _ref(name, g, s, conn)
            t2, tot2 = mr.measure_by_piece(labels, len(comps), conn)
            _same((table, total), (t2, tot2), f"{name} set {s} conn {conn}")
            assert np.array_equal(table["voxels"], comps["voxels"])
            _same((table, total), (table, mr.total_of(table)), "the total row is the sum of the records")
            if conn == cr.CONN_FULL:                                  # every face has two sides: a voxel of the set or an exposure
                assert np.array_equal(2 * table["cells"][:, 2], 6 * table["voxels"] + table["faces"].sum(axis=1))


@pytest.mark.parametrize("name,full,face", [("cube", 1, 1), ("shell", 2, 2), ("ring", 0, 0), ("corner_pair", 1, 2)])
def test_rule_euler_numbers_of_the_named_shapes(name, full, face):
    g = _named_grid(name)
    assert int(_ref(name, g, 1, cr.CONN_FULL)[3]["euler"]) == full
    assert int(_ref(name, g, 1, cr.CONN_FACE)[3]["euler"]) == face


@pytest.mark.parametrize("a,b,c", [(1, 1, 1), (5, 5, 5), (4, 3, 2), (1, 7, 2), (9, 1, 1)])
def test_rule_closed_forms_of_a_solid_box(a, b, c):
    g = np.zeros((c + 2, b + 3, a + 1), np.uint8)
    g[1:1 + c, 2:2 + b, 1:1 + a] = 1
    for conn in CONNS:
        labels, comps = cr.label(g, 1, conn)
        table, total = mr.measure(labels, len(comps), conn)
        assert len(table) == 1 and table[0].tobytes() == total.tobytes()
        assert list(total["faces"]) == [b * c, b * c, a * c, a * c, a * b, a * b] and total["voxels"] == a * b * c
        if conn == cr.CONN_FULL:
            want = [(a + 1) * (b + 1) * (c + 1), a * (b + 1) * (c + 1) + (a + 1) * b * (c + 1) + (a + 1) * (b + 1) * c,
                    a * b * (c + 1) + a * (b + 1) * c + (a + 1) * b * c]
        else:
            want = [(a - 1) * b * c + a * (b - 1) * c + a * b * (c - 1), (a - 1) * (b - 1) * c + (a - 1) * b * (c - 1) + a * (b - 1) * (c - 1),
                    (a - 1) * (b - 1) * (c - 1)]
        assert list(total["cells"]) == want and total["euler"] == 1
        i = np.arange(1, 1 + a)
        assert total["sum"][0] == i.sum() * b * c and total["sum2"][0] == (i * i).sum() * b * c
        assert total["sum2"][5] == np.arange(2, 2 + b).sum() * np.arange(1, 1 + c).sum() * a


@pytest.mark.parametrize("name,want", [("cube", (1, 0, 0)), ("shell", (1, 0, 1)), ("ring", (1, 1, 0)), ("frame", (1, 5, 0)),
                                       ("linked_rings", (2, 2, 0))])
def test_rule_topology_of_the_named_shapes(name, want):
    for conn in CONNS:
        assert mr.topology(_named_grid(name), 1, conn) == want, conn


def test_rule_topology_against_scipy():
    """Seeded random grids: pieces and cavities equal scipy.ndimage.label's counts (the complement under the dual connectivity,
    components that touch no grid face), and the tunnels that the Euler number then leaves are never negative."""
    ndi = pytest.importorskip("scipy.ndimage")
    structure = {cr.CONN_FACE: ndi.generate_binary_structure(3, 1), cr.CONN_FULL: ndi.generate_binary_structure(3, 3)}
    rng = np.random.default_rng(11)
    for fill in (0.2, 0.5, 0.8):
        for _ in range(4):
            g = (rng.random((9, 10, 11)) < fill).astype(np.uint8)
            for s in SETS:
                for conn in CONNS:
                    dual = cr.CONN_FULL if conn == cr.CONN_FACE else cr.CONN_FACE
                    _, b0 = ndi.label(g == s, structure[conn])
                    lab, n = ndi.label(g != s, structure[dual])
                    edge = np.unique(np.concatenate([lab[0].ravel(), lab[-1].ravel(), lab[:, 0].ravel(), lab[:, -1].ravel(),
                                                     lab[:, :, 0].ravel(), lab[:, :, -1].ravel()]))
                    b2 = n - len(edge[edge > 0])
                    pieces, tunnels, cavities = mr.topology(g, s, conn)
                    assert (pieces, cavities) == (b0, b2) and tunnels >= 0, (fill, s, conn)


@pytest.mark.parametrize("name", SMALL + ["checkerboard33", "full_4096x2x2", "face_slab_1", "face_slab_4"])
def test_reference_equals_the_host_layers_loops(name):
    from ray_tracing_octrees_amd import host
    g = _named_grid(name)
    for s in SETS:
        for conn in CONNS:
            labels, comps, table, total = _ref(name, g, s, conn)
            rc, t, tot = host.measureComponentsCPU(labels, len(comps), conn)
            assert rc == 0
            _same((t, tot), (table, total), f"{name} set {s} conn {conn}")


def test_host_layer_refusals():
    from ray_tracing_octrees_amd import hip, host
    labels = np.zeros((2, 3, 4), np.int32)
    assert host.measureComponentsCPU(labels, 1, 18)[0] == hip.RTO_E_INVALID
    assert host.measureComponentsCPU(labels, 0, 6)[0] == hip.RTO_E_INVALID                  # label 0 with no component
    assert host.measureComponentsCPU(np.zeros((1, 1, 32769), np.int32), 1, 6)[0] == hip.RTO_E_UNSUPPORTED
    rc, t, tot = host.measureComponentsCPU(np.full((2, 3, 4), -1, np.int32), 0, 26)
    assert rc == 0 and len(t) == 0 and tot.tobytes() == bytes(160)


def test_measure_physical_equals_the_direct_mean_and_covariance():
    """Within 1e-9 of the grid's extent (squared for the covariance): float64 sums of at most 1e5 terms err below 1e-11 relative, so
    this only keeps a wrong formula from passing."""
    hip = _hip()
    g = _random((33, 21, 17), 0.4, 5)
    g[2:9, 3:20, 4:30] = 1                                             # one elongated part among the debris
    gmin, vs = np.array([-3.5, 2.25, 10.0]), 0.125
    labels, comps, table, total = mr.measure_grid(g, 1, cr.CONN_FACE)
    phys = hip.measure_physical(table, gmin, vs)
    extent = vs * max(g.shape)
    big = int(np.argmax(table["voxels"]))
    for c in (big, 0, len(table) - 1):
        mean, cov = mr.physical_direct(labels, c, gmin, vs)
        assert np.abs(phys["centroid"][c] - mean).max() <= 1e-9 * extent
        assert np.abs(phys["covariance"][c] - cov).max() <= 1e-9 * extent * extent
        assert phys["volume"][c] == table["voxels"][c] * vs ** 3 and phys["area"][c] == table["faces"][c].sum() * vs ** 2
        w, v = phys["axes_variance"][c], phys["axes"][c]
        assert np.all(np.diff(w) >= 0) and np.abs(cov @ v - v * w).max() <= 1e-9 * extent * extent
    one = hip.measure_physical(total, gmin, vs)                         # a single record
    mean, cov = mr.physical_direct(np.where(labels >= 0, 0, -1), 0, gmin, vs)
    assert np.abs(one["centroid"] - mean).max() <= 1e-9 * extent and np.abs(one["covariance"] - cov).max() <= 1e-9 * extent * extent
    # the part is longest along x: its first principal axis (largest variance, last column) is x
    assert abs(phys["axes"][big][0, 2]) > 0.9


def test_measure_abi_layout_and_exports():
    """sizeof(rto_measure) == 160 with the fields where MEASURE_DTYPE puts them; the new symbols are exported."""
    hip = _hip()
    assert hip.MEASURE_DTYPE.itemsize == 160 and hip.MEASURE_DTYPE == mr.MEASURE_DTYPE
    fields = ("voxels", "faces", "cells", "euler", "sum", "sum2")
    assert [hip.MEASURE_DTYPE.fields[f][1] for f in fields] == [0, 8, 56, 80, 88, 112]
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.fail("no C compiler: the header's layout cannot be checked")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "abi.c")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "rto_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", '
                    'sizeof(rto_measure), offsetof(rto_measure, voxels), offsetof(rto_measure, faces), offsetof(rto_measure, cells), '
                    'offsetof(rto_measure, euler), offsetof(rto_measure, sum), offsetof(rto_measure, sum2), RTO_MEASURE_MAX_DIM); return 0; }\n')
        exe = os.path.join(tmp, "abi")
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert out == [str(v) for v in (160, 0, 8, 56, 80, 88, 112, hip.MEASURE_MAX_DIM)]
    L = hip.load()
    header = open(os.path.join(ROOT, "include", "rto_hip.h")).read()
    for s in SYMS:
        assert s in hip.SYMBOLS and hasattr(L, s), s
        assert s + "(" in header, s
    assert hip.COMPONENT_DTYPE.itemsize == 48                           # rto_component is what it was


def test_measure_kernels_keep_their_budgets():
    """The built assembly (the product's flags): the four k_measure kernels, k_measure_fold and k_measure_total without scratch, spills or v_mfma, at
    the VGPR and LDS figures DESIGN.md section 22 states; the 16-byte forms load label rows with dwordx4; the table is written with
    64-bit atomic adds that return nothing."""
    import test_isa_contract as isa
    asm = isa.built_asm()
    if asm is None:
        pytest.fail("no hipcc: the budget cannot be checked")
    meta = isa.kernel_meta(asm)
    names = [k for k in meta if "k_measure" in k]
    assert len(names) == 6, names
    seen = set()
    for k in names:
        m = meta[k]
        base = next(b for b in MS_VGPR if b in k)
        seen.add(base)
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (k, m)
        assert m["vgpr"] <= MS_VGPR[base], (k, m)
        lds = _lds_of(asm, k)
        assert lds <= next(v for b, v in MS_LDS.items() if b in k), (k, lds)
        ins = isa.body(asm, k[len("_ZN3rto"):])
        assert not any(t.startswith(("scratch_", "buffer_load", "buffer_store")) or "v_mfma" in t for t in ins), k
        assert any(t.startswith("global_atomic_add_x2") for t in ins), k
        assert not any(t.startswith("global_atomic") and "sc0" in t for t in ins), k      # no returning atomic: nothing is read back
        if "k_measureILb1E" in k:
            assert any(t.startswith("global_load_dwordx4") for t in ins), k
    assert seen == set(MS_VGPR)


def _lds_of(asm, kernel):
    """.group_segment_fixed_size of one kernel, from the metadata."""
    import re
    md = asm[asm.index(".amdgpu_metadata"):]
    for block in md.split("  - .agpr_count:")[1:]:
        if re.search(r"\.name:\s+" + re.escape(kernel) + r"\n", block):
            return int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
    raise AssertionError(kernel)


def test_sanitizer_script_reports_nothing():
    """tools/sanitize_measure.sh: host/Measure.cpp as a stand-alone program under AddressSanitizer and UBSan."""
    if not shutil.which("g++"):
        pytest.fail("no g++: the sanitizer build cannot be made")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize_measure.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "measure selftest ok" in r.stdout and "UBSan reports: 0" in r.stdout and "ASan reports: 0" in r.stdout, r.stdout


# ================================================================ GPU
gpu = pytest.mark.gpu


def _gpu_measures(ctx, s, conn):
    ctx.label_components(s, conn)
    return ctx.measure_components()


def _check_grid(ctx, name, g):
    _build(ctx, g)
    for s in SETS:
        for conn in CONNS:
            what = f"{name} set {s} conn {conn}"
            _, comps, table, total = _ref(name, g, s, conn)
            got = _gpu_measures(ctx, s, conn)
            _same(got, (table, total), what)
            assert np.array_equal(got[0]["voxels"], ctx.components()["voxels"]), what
            _same((ctx.component_measures(), got[1]), (table, total), what + " (read again)")
            assert all(m >= 0 for m in ctx.last_measure_ms()), what


GPU_GRIDS = [*sorted(RANDOM_GRIDS), "full", "empty", "checkerboard33", "corner_block", "corner_ring", "corner_rings3", "corner_slabs",
             *[f"face_slab_{d}" for d in range(6)], "full_4096x2x2", "cube", "shell", "frame", "linked_rings"]


@gpu
@pytest.mark.parametrize("name", GPU_GRIDS)
def test_gpu_table_and_total_equal_the_rule(ctx, name):
    _check_grid(ctx, name, _named_grid(name))


@gpu
def test_gpu_measures_on_both_build_paths(ctx, path):
    _check_grid(ctx, "random_33x9x9_50", _named_grid("random_33x9x9_50"))


@gpu
def test_gpu_shapes_of_the_stress_grids(ctx):
    """What the stress grids are there for: the checkerboard is one record per voxel under FACE and one under FULL; the long row's
    sum of ii is above 2^32 and one label spans every wave; the block at the tile corner owns cells in all eight tiles."""
    g = _checkerboard(33)
    _build(ctx, g)
    t, total = _gpu_measures(ctx, 1, cr.CONN_FACE)
    assert len(t) == int(g.sum()) and np.all(t["euler"] == 1) and np.all(t["faces"] == 1) and total["cells"].sum() == 0
    t, total = _gpu_measures(ctx, 1, cr.CONN_FULL)
    assert len(t) == 1 and t[0].tobytes() == total.tobytes()
    g = _named_grid("full_4096x2x2")
    _build(ctx, g)
    _, total = _gpu_measures(ctx, 1, cr.CONN_FACE)
    assert int(total["sum2"][0]) == 4 * 22898104320 > 2 ** 32 and int(total["voxels"]) == 16384 and int(total["euler"]) == 1
    g = _at_tile_corner("block")
    _build(ctx, g)
    _, total = _gpu_measures(ctx, 1, cr.CONN_FACE)
    assert list(total["cells"]) == [12, 6, 1] and list(total["faces"]) == [4] * 6
    _, total = _gpu_measures(ctx, 1, cr.CONN_FULL)
    assert list(total["cells"]) == [27, 54, 36] and int(total["euler"]) == 1


@gpu
@pytest.mark.parametrize("name", ["sphere64", "calgary"])
def test_gpu_scenes_equal_the_host_layers_loops(ctx, scenes, name):
    from ray_tracing_octrees_amd import host
    g = scenes(name).grid
    hip = _hip()
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    for s in SETS:
        for conn in CONNS:
            got = _gpu_measures(ctx, s, conn)
            rc, table, total = host.measureComponentsCPU(ctx.component_labels(), len(got[0]), conn)
            assert rc == 0
            _same(got, (table, total), f"{name} set {s} conn {conn}")


@gpu
@pytest.mark.parametrize("name,want", [("shell", (1, 0, 1)), ("ring", (1, 1, 0)), ("frame", (1, 5, 0)), ("linked_rings", (2, 2, 0))])
def test_gpu_topology_of_the_named_shapes(ctx, name, want):
    g = _named_grid(name)
    _build(ctx, g)
    for conn in CONNS:
        assert ctx.topology(1, conn) == want, conn
        # the set's labelling and measures are what stays resident
        _, comps, table, total = _ref(name, g, 1, conn)
        assert ctx.components().tobytes() == comps.tobytes()
        _same((ctx.component_measures(), total), (table, total), name)


@gpu
def test_gpu_measure_device_pointer_and_physical(ctx, scenes):
    from test_components import _d2h
    hip = _hip()
    g = scenes("sphere64").grid
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    table, total = _gpu_measures(ctx, 1, cr.CONN_FACE)
    ptr, n = ctx.component_measures_device()
    assert ptr and n == len(table)
    assert bytes(_d2h(ptr, n * 160)) == table.tobytes()
    phys = hip.measure_physical(total, g.min, g.voxel_size)
    mean, cov = mr.physical_direct(np.where(np.asarray(g.data) == 1, 0, -1), 0, g.min, g.voxel_size)
    extent = float(g.voxel_size) * 64
    assert np.abs(phys["centroid"] - mean).max() <= 1e-9 * extent and np.abs(phys["covariance"] - cov).max() <= 1e-9 * extent * extent


@gpu
def test_gpu_host_layer_measures(scenes):
    """RayTracerBVH::measureComponents / surfaceArea / centroid / topology on the shell."""
    import ray_tracing_octrees_amd as rto
    hip = _hip()
    g = _shell()
    vg = rto.VoxelGrid.from_array(g, GMIN, VOX)
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    assert rt.measureComponents(1, 6)[0] == hip.RTO_E_NO_OCTREE and rt.topology(1, 6)[0] == hip.RTO_E_NO_OCTREE
    rt.setOctreeFromGrid(vg)
    for conn in CONNS:
        _, comps, table, total = _ref("shell", g, 1, conn)
        rc, t, tot = rt.measureComponents(1, conn)
        assert rc == 0
        _same((t, tot), (table, total), f"shell conn {conn}")
        assert rt.topology(1, conn) == (0, (1, 0, 1))
    rc, area = rt.surfaceArea(1)
    assert rc == 0 and area == float(total["faces"].sum()) * float(VOX) ** 2
    rc, c = rt.centroid(1)
    want = hip.measure_physical(total, GMIN, VOX)["centroid"]
    assert rc == 0 and np.abs(np.asarray(c) - want).max() <= 1e-12
    assert rt.measureComponents(2, 6)[0] == hip.RTO_E_INVALID and rt.topology(1, 18)[0] == hip.RTO_E_INVALID


@gpu
def test_gpu_measures_go_when_the_labels_go(ctx, scenes):
    hip = _hip()
    g = scenes("sphere64").grid

    def gone():
        for read in (ctx.component_measures, ctx.component_measures_device):
            with pytest.raises(hip.RtoError) as e:
                read()
            assert e.value.code == hip.RTO_E_INVALID and "no measures are resident" in str(e.value)

    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    gone()
    with pytest.raises(hip.RtoError) as e:                             # measure before any labelling
        ctx.measure_components()
    assert e.value.code == hip.RTO_E_INVALID and "no labels are resident" in str(e.value)
    comps = ctx.label_components(cr.SET_SOLID, cr.CONN_FACE)
    gone()                                                              # labelled, not measured
    ms = ctx.last_components_ms()
    table, total = ctx.measure_components()
    assert ctx.components().tobytes() == comps.tobytes() and ctx.last_components_ms() == ms      # the labelling is as it was
    assert ctx.component_measures().tobytes() == table.tobytes()
    # an edit that changes nothing keeps labels and measures
    assert ctx.edit_components(cr.SET_SOLID, cr.CONN_FACE, cr.SELECT_SMALLER_THAN, 1) == 0
    assert ctx.component_measures().tobytes() == table.tobytes() and ctx.components().tobytes() == comps.tobytes()
    # a fresh labelling drops the measures
    ctx.label_components(cr.SET_SOLID, cr.CONN_FULL)
    gone()
    ctx.measure_components()
    corner = hip.make_brushes([np.asarray(g.min, np.float32) + np.float32(0.5) * g.voxel_size], 0.5 * float(g.voxel_size),
                              hip.BRUSH_SPHERE, hip.EDIT_FILL)
    assert ctx.edit_voxels(corner) == 1                                 # an edit that changes a voxel
    gone()
    ctx.label_components(cr.SET_EMPTY, cr.CONN_FACE)
    ctx.measure_components()
    ctx.build_octree(g.data, g.min, g.voxel_size)                       # a build
    gone()
    ctx.label_components(cr.SET_SOLID, cr.CONN_FACE)
    ctx.measure_components()
    v, tris = _box_mesh([0.3, 0.3, 0.3], [0.7, 0.7, 0.7])
    ctx.voxelize_mesh(v, tris, np.float32(0.125), grid=((8, 8, 8), np.zeros(3, np.float32), np.float32(0.125)))     # voxelize
    gone()
    fresh = hip.Context(0)
    try:
        with pytest.raises(hip.RtoError) as e:
            fresh.measure_components()
        assert e.value.code == hip.RTO_E_INVALID
        assert fresh.last_measure_ms() == (-1.0, -1.0)
    finally:
        fresh.close()


@gpu
def test_gpu_measure_errors_leave_the_context_untouched(ctx, scenes):
    hip = _hip()
    g = scenes("sphere64").grid
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    comps = ctx.label_components(cr.SET_EMPTY, cr.CONN_FACE)
    table, total = ctx.measure_components()
    assert len(table) >= 1
    L, h = ctx._L, ctx._h
    n = C.c_int64(-5)
    buf = np.zeros(len(table), hip.MEASURE_DTYPE)
    assert L.rto_download_measures(h, buf.ctypes.data, len(table) - 1, C.byref(n)) == hip.RTO_E_INVALID
    assert L.rto_last_error(h)
    assert ctx.component_measures().tobytes() == table.tobytes() and ctx.components().tobytes() == comps.tobytes()
    assert L.rto_download_measures(h, None, 0, C.byref(n)) == 0 and n.value == len(table)
    assert L.rto_measure_components(h, None) == 0                       # the total may be NULL
    assert ctx.component_measures().tobytes() == table.tobytes()


@gpu
def test_gpu_largest_dimension(ctx):
    """32768 x 1 x 1 measures correctly (the sum of ii is above 2^43); 32769 x 1 x 1 is refused and the labels stay."""
    hip = _hip()
    g = _named_grid("row_32768")
    g[0, 0, 1000] = 0                                                   # two pieces
    _build(ctx, g)
    for conn in CONNS:
        labels, comps = cr.label(g, 1, conn)
        _same(_gpu_measures(ctx, 1, conn), mr.measure(labels, len(comps), conn), f"32768 conn {conn}")
    g = np.ones((1, 1, 32769), np.uint8)
    _build(ctx, g)
    comps = ctx.label_components(cr.SET_SOLID, cr.CONN_FACE)
    with pytest.raises(hip.RtoError) as e:
        ctx.measure_components()
    assert e.value.code == hip.RTO_E_UNSUPPORTED and "32768" in str(e.value)
    assert ctx.components().tobytes() == comps.tobytes()
    with pytest.raises(hip.RtoError) as e:
        ctx.component_measures()
    assert e.value.code == hip.RTO_E_INVALID
