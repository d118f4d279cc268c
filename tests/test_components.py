"""Connected components (rto_label_components, rto_download_components / _labels, rto_labels_device, rto_edit_components,
Context.label_components / edit_components, RayTracerBVH::labelComponents / removeDebris / fillCavities / keepLargest).  CPU: the
numpy rule (tests/component_ref.py) on hand-made grids, against a flood fill, against the host layer's breadth-first search and,
where scipy is present, against scipy.ndimage.label; the ABI; the kernels' budgets.  GPU: labels and table bit for bit against the
rule on grids chosen around the 32 x 8 x 8 tile; edits against the rule, a fresh build and the oracle's frame; state and errors."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import component_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("rto_label_components", "rto_download_components", "rto_download_labels", "rto_labels_device", "rto_last_components_ms",
        "rto_debug_components_passes", "rto_edit_components")
SETS = (cr.SET_SOLID, cr.SET_EMPTY)
CONNS = (cr.CONN_FACE, cr.CONN_FULL)
TILE = (32, 8, 8)           # k_cc_local's tile, x, y, z (rto_components.inc)
# VGPRs the build gives; a kernel that grows past its line here has changed
CC_VGPR = {"k_cc_local": 38, "k_cc_merge": 20, "k_cc_flatten": 14, "k_scan_countsILi256Ejj": 24, "k_cc_rank": 26, "k_cc_label": 8,
           "k_cc_stats": 28, "k_cc_touches": 8, "k_cc_largest": 8, "k_cc_select": 4, "k_cc_flip": 28}


def _hip():
    from ray_tracing_octrees_amd import hip
    return hip


def _same(got, want, what):
    gl, gt = got
    wl, wt = want
    assert gl.shape == wl.shape and gl.dtype == np.int32, what
    assert np.array_equal(gl, wl), f"{what}: labels differ at {int((gl != wl).sum())} voxels"
    assert len(gt) == len(wt), f"{what}: {len(gt)} components vs {len(wt)}"
    for f in ("root", "voxels", "lo", "hi", "touches", "reserved"):
        assert np.array_equal(gt[f], wt[f]), f"{what}: table field {f}"


# ================================================================ grids
def _random(shape_xyz, fill, seed):
    x, y, z = shape_xyz
    return (np.random.default_rng(seed).random((z, y, x)) < fill).astype(np.uint8)


def _odd37():
    rng = np.random.default_rng(5)
    dims = (37, 53, 29)
    z, y, x = np.mgrid[0:dims[2], 0:dims[1], 0:dims[0]]
    blob = ((x - 18) ** 2 / 15.0 ** 2 + (y - 26) ** 2 / 22.0 ** 2 + (z - 14) ** 2 / 12.0 ** 2) <= 1.0
    return (blob & (rng.random(blob.shape) < 0.97)).astype(np.uint8)


def _checkerboard(n):
    z, y, x = np.mgrid[0:n, 0:n, 0:n]
    return ((x + y + z) % 2 == 0).astype(np.uint8)


def _serpentine(n):
    """A one-voxel-wide path through n^3 (n even): a snake over the rows of every second layer, the layers joined end to end."""
    g = np.zeros((n, n, n), np.uint8)
    layers = list(range(0, n, 2))
    for li, z in enumerate(layers):
        rows = list(range(0, n, 2))
        for ri, y in enumerate(rows):
            g[z, y, :] = 1
            if ri + 1 < len(rows):
                g[z, y + 1, n - 1 if ri % 2 == 0 else 0] = 1
        end = (rows[-1], 0 if len(rows) % 2 == 0 else n - 1)          # where the snake that started at (y 0, x 0) ends
        if li + 1 < len(layers):
            y, x = end if li % 2 == 0 else (0, 0)
            g[z + 1, y, x] = 1
    return g


def _corner_slabs():
    """Two blocks that meet only across the corner shared by the tiles (0, 0, 0) and (1, 1, 1)."""
    g = np.zeros((2 * TILE[2], 2 * TILE[1], 2 * TILE[0]), np.uint8)
    g[:TILE[2], :TILE[1], :TILE[0]] = 1
    g[TILE[2]:, TILE[1]:, TILE[0]:] = 1
    return g


RANDOM_GRIDS = {f"random_{x}x{y}x{z}_{int(fill * 100)}": ((x, y, z), fill, 100 + i)
                for i, ((x, y, z), fill) in enumerate([(s, f) for s in ((17, 9, 5), (33, 33, 33)) for f in (0.2, 0.31, 0.5, 0.7)]
                                                      + [((65, 33, 17), 0.31)])}


def _named_grid(name, scenes=None):
    if name in RANDOM_GRIDS:
        return _random(*RANDOM_GRIDS[name])
    if name == "one_filled":
        return np.ones((1, 1, 1), np.uint8)
    if name == "one_empty":
        return np.zeros((1, 1, 1), np.uint8)
    if name == "3x2x5":
        return _random((3, 2, 5), 0.5, 7)
    if name == "tile_plus_1":
        return _random((TILE[0] + 1, TILE[1] + 1, TILE[2] + 1), 0.4, 8)
    if name == "tile_minus_1":
        return _random((TILE[0] - 1, TILE[1] - 1, TILE[2] - 1), 0.4, 9)
    if name == "odd37":
        return _odd37()
    if name == "checkerboard33":
        return _checkerboard(33)
    if name == "serpentine48":
        return _serpentine(48)
    if name == "corner_slabs":
        return _corner_slabs()
    if name == "full":
        return np.ones((12, 20, 40), np.uint8)
    if name == "empty":
        return np.zeros((12, 20, 40), np.uint8)
    return np.ascontiguousarray(scenes(name).grid.data, np.uint8)


_REF = {}


def _ref(name, grid, s, conn):
    """The rule's answer, computed once per (grid, set, connectivity) and shared."""
    key = (name, s, conn)
    if key not in _REF:
        l, t = cr.label(grid, s, conn)
        l.setflags(write=False)
        t.setflags(write=False)
        _REF[key] = (l, t)
    return _REF[key]


# ================================================================ CPU: the rule
def _two(at_a, at_b, shape=(3, 3, 3)):
    g = np.zeros(shape, np.uint8)
    g[at_a[::-1]] = 1
    g[at_b[::-1]] = 1
    return g


def test_rule_edge_and_corner_contact_join_only_under_full_connectivity():
    for b in ((1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1)):              # by an edge (three ways) and by a corner
        g = _two((0, 0, 0), b)
        lf, tf = cr.label(g, cr.SET_SOLID, cr.CONN_FACE)
        lu, tu = cr.label(g, cr.SET_SOLID, cr.CONN_FULL)
        assert len(tf) == 2 and len(tu) == 1, b
        assert list(tf["voxels"]) == [1, 1] and list(tu["voxels"]) == [2]
        assert lf[0, 0, 0] == 0 and lf[b[::-1]] == 1 and lu[0, 0, 0] == 0 and lu[b[::-1]] == 0
    g = _two((0, 0, 0), (1, 0, 0))                                      # by a face: one under both
    assert len(cr.label(g, cr.SET_SOLID, cr.CONN_FACE)[1]) == 1


def test_rule_canonical_numbering_and_roots():
    g = np.zeros((2, 3, 4), np.uint8)
    g[1, 2, 3] = 1
    g[0, 0, 2] = 1
    g[0, 2, 0] = 1
    l, t = cr.label(g, cr.SET_SOLID, cr.CONN_FACE)
    assert list(t["root"]) == [2, 8, 23] and l[0, 0, 2] == 0 and l[0, 2, 0] == 1 and l[1, 2, 3] == 2
    assert (l[g == 0] == -1).all()
    le, te = cr.label(g, cr.SET_EMPTY, cr.CONN_FACE)
    assert len(te) == 1 and te["root"][0] == 0 and te["voxels"][0] == 21 and (le[g == 1] == -1).all()


def test_rule_all_but_largest_keeps_the_smaller_root_on_a_tie():
    g = np.zeros((1, 1, 8), np.uint8)
    g[0, 0, [0, 1, 3, 4, 6]] = 1                                        # sizes 2, 2, 1
    out, changed = cr.apply_selection(g, cr.SET_SOLID, cr.CONN_FACE, cr.SELECT_ALL_BUT_LARGEST)
    assert changed == 3 and list(out[0, 0]) == [1, 1, 0, 0, 0, 0, 0, 0]
    g[0, 0, 5] = 1                                                      # sizes 2, 3, and 6 joins: 2, 4
    out, changed = cr.apply_selection(g, cr.SET_SOLID, cr.CONN_FACE, cr.SELECT_ALL_BUT_LARGEST)
    assert changed == 2 and list(out[0, 0]) == [0, 0, 0, 1, 1, 1, 1, 0]


def test_rule_touches_bits():
    g = np.zeros((4, 5, 6), np.uint8)
    for (x, y, z), want in (((0, 2, 2), 1), ((2, 0, 2), 2), ((2, 2, 0), 4), ((5, 2, 2), 8), ((2, 4, 2), 16), ((2, 2, 3), 32),
                            ((2, 2, 2), 0), ((0, 0, 0), 7), ((5, 4, 3), 56)):
        g[:] = 0
        g[z, y, x] = 1
        assert cr.label(g, cr.SET_SOLID, cr.CONN_FACE)[1]["touches"][0] == want, (x, y, z)
    g[:] = 1
    assert cr.label(g, cr.SET_SOLID, cr.CONN_FACE)[1]["touches"][0] == 63
    one = np.ones((1, 1, 1), np.uint8)
    assert cr.label(one, cr.SET_SOLID, cr.CONN_FULL)[1]["touches"][0] == 63     # index 0 is also index dim - 1


def test_rule_hollow_box_is_enclosed_until_it_has_a_hole():
    g = np.zeros((9, 9, 9), np.uint8)
    g[2:7, 2:7, 2:7] = 1
    g[3:6, 3:6, 3:6] = 0
    l, t = cr.label(g, cr.SET_EMPTY, cr.CONN_FACE)
    assert len(t) == 2 and t["touches"][0] == 63 and t["touches"][1] == 0 and t["voxels"][1] == 27
    out, changed = cr.apply_selection(g, cr.SET_EMPTY, cr.CONN_FACE, cr.SELECT_ENCLOSED)
    assert changed == 27 and out[2:7, 2:7, 2:7].all() and out.sum() == 125
    g[4, 4, 6] = 0                                                      # a one-voxel hole in the +x wall
    l, t = cr.label(g, cr.SET_EMPTY, cr.CONN_FACE)
    assert len(t) == 1
    out, changed = cr.apply_selection(g, cr.SET_EMPTY, cr.CONN_FACE, cr.SELECT_ENCLOSED)
    assert changed == 0 and np.array_equal(out, g)
    g[4, 4, 6] = 1
    g[2, 2, 2] = 0                                                      # a missing corner voxel opens it only to 26-connectivity
    assert len(cr.label(g, cr.SET_EMPTY, cr.CONN_FACE)[1]) == 2 and len(cr.label(g, cr.SET_EMPTY, cr.CONN_FULL)[1]) == 1


def test_rule_smaller_than_and_containing():
    g = np.zeros((1, 1, 8), np.uint8)
    g[0, 0, [0, 2, 3]] = 1
    for arg, want in ((0, 0), (1, 0), (2, 1), (3, 3)):
        out, changed = cr.apply_selection(g, cr.SET_SOLID, cr.CONN_FACE, cr.SELECT_SMALLER_THAN, arg)
        assert changed == want, arg
    out, changed = cr.apply_selection(g, cr.SET_SOLID, cr.CONN_FACE, cr.SELECT_CONTAINING, 3)
    assert changed == 2 and list(out[0, 0]) == [1, 0, 0, 0, 0, 0, 0, 0]
    out, changed = cr.apply_selection(g, cr.SET_SOLID, cr.CONN_FACE, cr.SELECT_NOT_CONTAINING, 3)
    assert changed == 1 and list(out[0, 0]) == [0, 0, 1, 1, 0, 0, 0, 0]
    for sel in (cr.SELECT_CONTAINING, cr.SELECT_NOT_CONTAINING):        # voxel 1 is EMPTY: not in the set, nothing selected
        out, changed = cr.apply_selection(g, cr.SET_SOLID, cr.CONN_FACE, sel, 1)
        assert changed == 0 and np.array_equal(out, g)
    out, changed = cr.apply_selection(g, cr.SET_EMPTY, cr.CONN_FACE, cr.SELECT_CONTAINING, 1)
    assert changed == 1 and list(out[0, 0]) == [1, 1, 1, 1, 0, 0, 0, 0]


@pytest.mark.parametrize("name", ["3x2x5", "random_17x9x5_31", "random_17x9x5_50", "one_filled", "one_empty"])
def test_reference_equals_the_flood_fill_statement(name):
    g = _named_grid(name)
    for s in SETS:
        for conn in CONNS:
            _same(_ref(name, g, s, conn), cr.brute_force(g, s, conn), f"{name} set {s} conn {conn}")


@pytest.mark.parametrize("name", sorted(n for n in RANDOM_GRIDS if "65x" not in n))
def test_reference_equals_the_host_layers_search(name):
    """tests/component_ref.py against labelComponentsCPU / applyComponentSelectionCPU (host/Components.cpp) on seeded random grids."""
    import ray_tracing_octrees_amd as rto
    g = _named_grid(name)
    first_solid, first_empty = int(np.flatnonzero(g.reshape(-1) == 1)[0]), int(np.flatnonzero(g.reshape(-1) == 0)[0])
    for s in SETS:
        for conn in CONNS:
            vg = rto.VoxelGrid.from_array(g, (0.0, 0.0, 0.0), 1.0)
            _same(vg.labelComponents(s, conn), _ref(name, g, s, conn), f"{name} set {s} conn {conn}")
            inside = first_solid if s == cr.SET_SOLID else first_empty
            for sel, arg in ((cr.SELECT_SMALLER_THAN, 4), (cr.SELECT_ALL_BUT_LARGEST, 0), (cr.SELECT_ENCLOSED, 0),
                             (cr.SELECT_CONTAINING, inside), (cr.SELECT_NOT_CONTAINING, inside),
                             (cr.SELECT_CONTAINING, first_empty if s == cr.SET_SOLID else first_solid)):
                vg = rto.VoxelGrid.from_array(g, (0.0, 0.0, 0.0), 1.0)
                want, want_changed = cr.apply_selection(g, s, conn, sel, arg)
                assert vg.applyComponentSelection(s, conn, sel, arg) == want_changed, (name, s, conn, sel)
                assert np.array_equal(vg.data, want), (name, s, conn, sel)
    vg = rto.VoxelGrid.from_array(g, (0.0, 0.0, 0.0), 1.0)
    for bad in ((2, 6, 0, 0), (1, 18, 0, 0), (1, 6, 5, 0), (1, 6, 0, -1), (1, 6, 3, -1), (1, 6, 3, g.size), (1, 6, 4, g.size)):
        assert vg.applyComponentSelection(*bad) == -1 and np.array_equal(vg.data, g), bad


def test_reference_partition_equals_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for name in sorted(RANDOM_GRIDS):
        g = _named_grid(name)
        for s in SETS:
            for conn in CONNS:
                want, n = ndi.label(g == s, structure=ndi.generate_binary_structure(3, 1 if conn == cr.CONN_FACE else 3))
                l, t = _ref(name, g, s, conn)
                assert len(t) == n
                # same partition: the pairs (ours, scipy's) are a bijection
                pairs = np.unique(np.stack([l[l >= 0].astype(np.int64), want[l >= 0].astype(np.int64)], 1), axis=0)
                assert len(pairs) == n and len(np.unique(pairs[:, 0])) == n and len(np.unique(pairs[:, 1])) == n
                assert ((want == 0) == (l < 0)).all()


def test_reference_labels_calgary_quickly(scenes):
    import time
    g = _named_grid("calgary", scenes)
    t0 = time.perf_counter()
    l, t = cr.label(g, cr.SET_SOLID, cr.CONN_FULL)
    dt = time.perf_counter() - t0
    assert int(t["voxels"].sum()) == int(g.sum()) and (l >= 0).sum() == g.sum()
    assert dt < 10.0, dt


def test_component_abi_layout_and_exports():
    """sizeof(rto_component) == 48 with the fields where COMPONENT_DTYPE puts them; the constants; the new symbols are exported."""
    hip = _hip()
    assert hip.COMPONENT_DTYPE.itemsize == 48 and cr.COMPONENT_DTYPE == hip.COMPONENT_DTYPE
    fields = ("root", "voxels", "lo", "hi", "touches", "reserved")
    assert [hip.COMPONENT_DTYPE.fields[f][1] for f in fields] == [0, 8, 16, 28, 40, 44]
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.fail("no C compiler: the header's layout cannot be checked")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "abi.c")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "rto_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu '
                    '%d %d %d %d %d %d %d %d %d %d\\n", sizeof(rto_component), offsetof(rto_component, root), offsetof(rto_component, voxels), '
                    'offsetof(rto_component, lo), offsetof(rto_component, hi), offsetof(rto_component, touches), '
                    'offsetof(rto_component, reserved), RTO_SET_EMPTY, RTO_SET_SOLID, RTO_CONN_FACE, RTO_CONN_FULL, '
                    'RTO_SELECT_SMALLER_THAN, RTO_SELECT_ALL_BUT_LARGEST, RTO_SELECT_ENCLOSED, RTO_SELECT_CONTAINING, '
                    'RTO_SELECT_NOT_CONTAINING, RTO_E_INTERNAL); return 0; }\n')
        exe = os.path.join(tmp, "abi")
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert out == [str(v) for v in (48, 0, 8, 16, 28, 40, 44, hip.SET_EMPTY, hip.SET_SOLID, hip.CONN_FACE, hip.CONN_FULL,
                                    hip.SELECT_SMALLER_THAN, hip.SELECT_ALL_BUT_LARGEST, hip.SELECT_ENCLOSED, hip.SELECT_CONTAINING,
                                    hip.SELECT_NOT_CONTAINING, hip.RTO_E_INTERNAL)]
    assert (cr.SET_EMPTY, cr.SET_SOLID, cr.CONN_FACE, cr.CONN_FULL) == (hip.SET_EMPTY, hip.SET_SOLID, hip.CONN_FACE, hip.CONN_FULL)
    L = hip.load()
    header = open(os.path.join(ROOT, "include", "rto_hip.h")).read()
    for s in SYMS:
        assert s in hip.SYMBOLS and hasattr(L, s), s
        assert s + "(" in header, s


def test_component_kernels_keep_their_budgets():
    """The built assembly (the product's flags): every k_cc_* kernel and the components' k_scan_counts without scratch, spills or v_mfma, at the VGPR counts DESIGN.md
    section 18 states; the 16-byte forms of k_cc_local and k_cc_flip move rows with dwordx4 accesses."""
    import test_isa_contract as isa
    asm = isa.built_asm()
    if asm is None:
        pytest.fail("no hipcc: the budget cannot be checked")
    meta = isa.kernel_meta(asm)
    names = [k for k in meta if "k_cc_" in k or "k_scan_countsILi256Ejj" in k]     # the scan of the chunk counts: the shared kernel's kBlock, unsigned form
    assert len(names) == 16, names              # local x4, merge x2, flip x2, eight others
    seen = set()
    for k in names:
        m = meta[k]
        base = next(b for b in CC_VGPR if b in k)
        seen.add(base)
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (k, m)
        assert m["vgpr"] <= CC_VGPR[base], (k, m)
        ins = isa.body(asm, k[len("_ZN3rto"):])
        assert not any(t.startswith(("scratch_", "buffer_load", "buffer_store")) or "v_mfma" in t for t in ins), k
        if "k_cc_local" in k and "ILb1E" in k:
            assert any(t.startswith("global_load_dwordx4") for t in ins), k
        if "k_cc_flip" in k and "ILb1E" in k:
            assert any(t.startswith("global_load_dwordx4") for t in ins) and any(t.startswith("global_store_dwordx4") for t in ins), k
    assert seen == set(CC_VGPR)


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


def _build(ctx, grid):
    ctx.set_kernel(_hip().KERNEL_AUTO)
    ctx.build_octree(grid, GMIN, VOX)


def _gpu_labelling(ctx, s, conn):
    table = ctx.label_components(s, conn)
    return ctx.component_labels(), table


LABEL_GRIDS = ["one_filled", "one_empty", "3x2x5", "tile_plus_1", "tile_minus_1", "odd37", *sorted(RANDOM_GRIDS), "checkerboard33",
               "serpentine48", "corner_slabs", "full", "empty", "sphere64", "sphere256", "calgary"]


@gpu
@pytest.mark.parametrize("name", LABEL_GRIDS)
def test_gpu_labels_and_table_equal_the_rule(ctx, scenes, name):
    g = _named_grid(name, scenes)
    _build(ctx, g)
    for s in SETS:
        for conn in CONNS:
            what = f"{name} set {s} conn {conn}"
            _same(_gpu_labelling(ctx, s, conn), _ref(name, g, s, conn), what)
            passes = ctx.components_passes()
            assert 2 <= passes < 32, (what, passes)
            ms = ctx.last_components_ms()
            assert all(m >= 0 for m in ms), (what, ms)
            _same((ctx.component_labels(), ctx.components()), _ref(name, g, s, conn), what + " (read again)")


@gpu
def test_gpu_shapes_of_the_stress_grids(ctx):
    """What the stress grids are there for: the checkerboard is one component per voxel under FACE and one in all under FULL; the
    serpentine is one component that crosses tile faces hundreds of times and still merges within the cap; the slabs join only
    across the tile corner."""
    g = _checkerboard(33)
    _build(ctx, g)
    assert len(ctx.label_components(cr.SET_SOLID, cr.CONN_FACE)) == int(g.sum())
    assert len(ctx.label_components(cr.SET_SOLID, cr.CONN_FULL)) == 1
    g = _serpentine(48)
    _build(ctx, g)
    for conn in CONNS:
        t = ctx.label_components(cr.SET_SOLID, conn)
        assert len(t) == 1 and t["voxels"][0] == g.sum() and t["root"][0] == 0
        assert ctx.components_passes() < 32
    g = _corner_slabs()
    _build(ctx, g)
    assert len(ctx.label_components(cr.SET_SOLID, cr.CONN_FACE)) == 2 and len(ctx.label_components(cr.SET_SOLID, cr.CONN_FULL)) == 1


def _d2h(ptr, nbytes):
    L = _hip().load()
    out = np.zeros(nbytes, np.uint8)
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert L.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), nbytes, 2) == 0          # hipMemcpyDeviceToHost
    return out


@gpu
def test_gpu_labels_device_pointers(ctx):
    name = "random_33x33x33_31"
    g = _named_grid(name)
    _build(ctx, g)
    table = ctx.label_components(cr.SET_SOLID, cr.CONN_FACE)
    d_labels, d_table, n = ctx.component_labels_device()
    assert d_labels and d_table and n == len(table) > 0
    want = _ref(name, g, cr.SET_SOLID, cr.CONN_FACE)
    assert _d2h(d_labels, 4 * g.size).tobytes() == want[0].tobytes()
    assert _d2h(d_table, 48 * n).tobytes() == table.tobytes() == want[1].tobytes()


def _same_struct(a, b):
    return bytes(a) == bytes(b)


def _check_rebuilt(ctx, ctx2, orc, gmin, vox, edited, what):
    """ctx (edited) holds what a fresh rto_build_octree of `edited` leaves: voxels, nodes (== the oracle's), info, scene bounds."""
    assert np.array_equal(ctx.download_voxels(), edited), f"{what}: voxels"
    dims = edited.shape[::-1]
    og = orc.Grid(dims, gmin, vox, edited)
    want = orc.build_flat_octree(og)
    got = ctx.download_nodes()
    assert got.tobytes() == want.tobytes(), f"{what}: nodes ({len(got)} vs {len(want)})"
    ctx2.build_octree(edited, gmin, vox)
    assert ctx2.download_nodes().tobytes() == want.tobytes(), what
    assert _same_struct(ctx.info(), ctx2.info()), f"{what}: info"
    assert _same_struct(ctx.scene_bounds(), ctx2.scene_bounds()), f"{what}: scene bounds"
    return og, want


def _check_render(ctx, orc, og, nodes, view, pos, what):
    from conftest import assert_bit_exact
    f = _hip().make_frame(view, pos, W / H, FOV, W, H)
    want, _ = orc.render(nodes, og.min, og.voxel_size, view, pos, W / H, FOV, W, H, nthreads=min(16, orc.max_threads()))
    assert_bit_exact(ctx.render_host(f), want, f"{what}: render")


def _scene(orc, scenes, camera, name):
    """(data, gridMin, voxelSize, view, pos) of an edit scene."""
    from conftest import make_camera
    if name in ("odd37", "random"):
        data = _odd37() if name == "odd37" else _random((33, 33, 33), 0.31, 41)
        vox = np.float32(1.0 / 64)
        gmin = (-0.5 * np.asarray(data.shape[::-1], np.float32) * vox).astype(np.float32)
        return data, gmin, vox, *make_camera(orc, 0.5, 0.7, 1.8)
    g = scenes(name).grid
    view, pos = camera("calgary_oblique") if name == "calgary" else make_camera(orc, 0.5, 0.7, 1.8)
    return np.ascontiguousarray(g.data, np.uint8), g.min, g.voxel_size, view, pos


def _selections(cur):
    flat = cur.reshape(-1)
    solid = int(np.flatnonzero(flat == 1)[len(np.flatnonzero(flat == 1)) // 2])
    return [("smaller than 50", cr.SET_SOLID, cr.CONN_FACE, cr.SELECT_SMALLER_THAN, 50),
            ("enclosed empty", cr.SET_EMPTY, cr.CONN_FACE, cr.SELECT_ENCLOSED, 0),
            ("containing", cr.SET_SOLID, cr.CONN_FULL, cr.SELECT_CONTAINING, solid),
            ("not containing voxel 0", cr.SET_EMPTY, cr.CONN_FACE, cr.SELECT_NOT_CONTAINING, 0),
            ("all but largest", cr.SET_SOLID, cr.CONN_FACE, cr.SELECT_ALL_BUT_LARGEST, 0)]


@gpu
@pytest.mark.parametrize("name", ["odd37", "sphere64", "random", "calgary"])
def test_gpu_component_edits_equal_the_rule_and_a_fresh_build(ctx, ctx2, orc, scenes, camera, name, path):
    """Every selection, each on the grid the one before left: the grid and changed are the rule's, the context equals a fresh
    build of that grid (nodes == the oracle's, info, scene bounds), and the frame is the oracle's."""
    data, gmin, vox, view, pos = _scene(orc, scenes, camera, name)
    ctx.set_kernel(_hip().KERNEL_AUTO)
    ctx.build_octree(data, gmin, vox)
    cur = data
    # a brush through the middle first, so that "containing" and "all but largest" have pieces to choose from
    mid = cur.shape[0] // 2
    hip = _hip()
    centre = (np.asarray(gmin, np.float64) + (np.asarray(cur.shape[::-1], np.float64) / 2) * float(vox)).astype(np.float32)
    half = np.asarray(cur.shape[::-1], np.float64) * float(vox)
    half[2] = 1.0 * float(vox)
    ctx.edit_voxels(hip.make_brushes([centre], [half.astype(np.float32)], hip.BRUSH_BOX, hip.EDIT_CARVE))
    cur = ctx.download_voxels()
    assert not cur[mid - 1:mid + 1].any() or not cur[mid].any()
    any_change = False
    for label, s, conn, sel, arg in _selections(cur):
        want, want_changed = cr.apply_selection(cur, s, conn, sel, arg)
        got_changed = ctx.edit_components(s, conn, sel, arg)
        what = f"{name} {path} {label}"
        assert got_changed == want_changed, f"{what}: changed {got_changed} vs {want_changed}"
        if want_changed == 0:
            assert np.array_equal(ctx.download_voxels(), cur), what
            continue
        any_change = True
        og, nodes = _check_rebuilt(ctx, ctx2, orc, gmin, vox, want, what)
        _check_render(ctx, orc, og, nodes, view, pos, what)
        assert ctx.info().culling_active == 0
        cur = want
    assert any_change


@gpu
@pytest.mark.parametrize("source", ["gpu", "upload"])
def test_gpu_component_edit_rebuilds_resident_triangles(ctx, ctx2, orc, scenes, source, path):
    """sphere64 is a shell: filling its cavity with triangles resident (built on the GPU, or uploaded) leaves the triangles of a
    fresh triangle build of the filled grid."""
    g = scenes("sphere64").grid
    ctx.set_kernel(_hip().KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    if source == "gpu":
        ctx.build_leaf_triangles(None)
    else:
        tris, off = orc.build_leaf_triangles(g, orc.build_flat_octree(g))
        ctx.upload_leaf_triangles(tris, off)
    want, changed = cr.apply_selection(g.data, cr.SET_EMPTY, cr.CONN_FACE, cr.SELECT_ENCLOSED)
    assert changed > 0
    assert ctx.edit_components(cr.SET_EMPTY, cr.CONN_FACE, cr.SELECT_ENCLOSED) == changed
    og, nodes = _check_rebuilt(ctx, ctx2, orc, g.min, g.voxel_size, want, f"sphere64 {source} {path}")
    ctx2.build_leaf_triangles(None)
    t1, o1 = ctx.download_leaf_triangles()
    t2, o2 = ctx2.download_leaf_triangles()
    assert t1.tobytes() == t2.tobytes() and o1.tobytes() == o2.tobytes()
    wt, wo = orc.build_leaf_triangles(og, nodes)
    assert t1.tobytes() == np.asarray(wt, np.float32).tobytes() and o1.tobytes() == np.asarray(wo, np.int32).tobytes()


@gpu
def test_gpu_carved_sphere_falls_in_two_and_keep_largest_leaves_one(ctx, ctx2, orc, scenes):
    from conftest import make_camera
    import ray_tracing_octrees_amd as rto
    hip = _hip()
    g = scenes("sphere64").grid
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    assert len(ctx.label_components(cr.SET_SOLID, cr.CONN_FACE)) == 1
    # a slab two voxels thick, off centre so that the two pieces differ in size
    centre = (np.asarray(g.min, np.float64) + np.array([32.0, 32.0, 24.0]) * float(g.voxel_size)).astype(np.float32)
    half = np.array([64.0, 64.0, 1.0]) * float(g.voxel_size)
    assert ctx.edit_voxels(hip.make_brushes([centre], [half.astype(np.float32)], hip.BRUSH_BOX, hip.EDIT_CARVE)) > 0
    with pytest.raises(hip.RtoError) as e:                               # the edit dropped the labels
        ctx.component_labels()
    assert e.value.code == hip.RTO_E_INVALID
    carved = ctx.download_voxels()
    table = ctx.label_components(cr.SET_SOLID, cr.CONN_FACE)
    assert len(table) == 2 and table["voxels"][0] != table["voxels"][1]
    want, changed = cr.apply_selection(carved, cr.SET_SOLID, cr.CONN_FACE, cr.SELECT_ALL_BUT_LARGEST)
    assert changed == int(table["voxels"].min())
    assert ctx.edit_components(cr.SET_SOLID, cr.CONN_FACE, cr.SELECT_ALL_BUT_LARGEST) == changed
    assert len(ctx.label_components(cr.SET_SOLID, cr.CONN_FACE)) == 1
    og, nodes = _check_rebuilt(ctx, ctx2, orc, g.min, g.voxel_size, want, "keep largest")
    _check_render(ctx, orc, og, nodes, *make_camera(orc, 0.5, 0.7, 1.8), "keep largest")
    # the host class, same scene: keepLargest after the same carve
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    rt.setOctreeFromGrid(rto.VoxelGrid.from_array(g.data, g.min, g.voxel_size))
    assert rt.editVoxels(hip.make_brushes([centre], [half.astype(np.float32)], hip.BRUSH_BOX, hip.EDIT_CARVE)) > 0
    t = rt.labelComponents(cr.SET_SOLID, cr.CONN_FACE)
    assert t is not None and t.tobytes() == table.tobytes()
    assert np.array_equal(rt.componentLabels(), cr.label(carved, cr.SET_SOLID, cr.CONN_FACE)[0])
    assert rt.keepLargest() == changed and np.array_equal(rt.grid(), want)
    assert rt.componentLabels() is None
    assert rt.removeDebris(10) == 0 and rt.flipComponentAt(0, 0, 0, cr.SET_SOLID) == 0


def _box_mesh(lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(hi if (i >> a) & 1 else lo)[a] for a in range(3)] for i in range(8)], np.float64)
    quads = [(0, 2, 6, 4), (1, 5, 7, 3), (0, 4, 5, 1), (2, 3, 7, 6), (0, 1, 3, 2), (4, 6, 7, 5)]
    tris = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.int32)
    return v, tris


@gpu
def test_gpu_fill_cavities_makes_a_voxelized_box_solid(ctx):
    """A closed box mesh voxelizes to a shell; filling the enclosed empty space flips exactly the inside, and the span through the
    centre turns from two walls with a gap into one solid interval."""
    hip = _hip()
    n = 40
    vox = np.float32(0.25)
    gmin = np.zeros(3, np.float32)
    v, tris = _box_mesh([2.6, 2.6, 2.6], [7.4, 7.4, 7.4])               # voxel centres 10.5 .. 29.5 lie inside: a 20^3 box
    ctx.voxelize_mesh(v, tris, vox, grid=((n, n, n), gmin, vox))
    shell = ctx.download_voxels()
    assert shell.any()
    z, y, x = np.nonzero(shell)
    box = (slice(z.min(), z.max() + 1), slice(y.min(), y.max() + 1), slice(x.min(), x.max() + 1))
    row = shell[n // 2, n // 2, x.min():x.max() + 1]
    t = int(np.argmin(row))                                             # wall thickness along the centre line
    assert 1 <= t <= 3 and row[:t].all() and row[-t:].all() and not row[t:-t].any()
    core = (slice(z.min() + t, z.max() + 1 - t), slice(y.min() + t, y.max() + 1 - t), slice(x.min() + t, x.max() + 1 - t))
    inside = int(shell[core].size)
    assert inside > 1000 and not shell[core].any() and shell[n // 2, n // 2, n // 2] == 0
    assert shell[box][0].any() and shell[box][-1].any()
    origin, d = np.array([-1.0, 5.0, 5.0], np.float32), np.array([1.0, 0.0, 0.0], np.float32)
    before = ctx.query_spans(origin, [d])[0]
    assert before["leaves"] >= 2 and before["length"] < 0.5 * (before["t_exit"] - before["t_enter"])      # two walls, a gap between
    want, changed = cr.apply_selection(shell, cr.SET_EMPTY, cr.CONN_FACE, cr.SELECT_ENCLOSED)
    assert changed == inside
    assert ctx.edit_components(cr.SET_EMPTY, cr.CONN_FACE, cr.SELECT_ENCLOSED) == inside
    filled = ctx.download_voxels()
    assert np.array_equal(filled, want) and filled[core].all() and filled.sum() == shell.sum() + inside
    after = ctx.query_spans(origin, [d])[0]
    width = (x.max() + 1 - x.min()) * float(vox)
    assert abs(float(after["length"]) - width) < 1e-4 and abs(float(after["t_exit"] - after["t_enter"]) - width) < 1e-4   # one interval
    assert abs(float(before["t_exit"] - before["t_enter"]) - width) < 1e-4


@gpu
def test_gpu_labels_are_dropped_when_the_grid_changes(ctx, orc, scenes):
    hip = _hip()
    g = scenes("sphere64").grid

    def gone():
        for read in (ctx.component_labels, ctx.components, ctx.component_labels_device):
            with pytest.raises(hip.RtoError) as e:
                read()
            assert e.value.code == hip.RTO_E_INVALID and "no labels are resident" in str(e.value)

    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    gone()                                                              # never labelled
    ctx.label_components(cr.SET_SOLID, cr.CONN_FACE)
    ctx.component_labels()
    ctx.build_octree(g.data, g.min, g.voxel_size)                       # build
    gone()
    ctx.label_components(cr.SET_EMPTY, cr.CONN_FULL)
    corner = hip.make_brushes([np.asarray(g.min, np.float32) + np.float32(0.5) * g.voxel_size], 0.5 * float(g.voxel_size),
                              hip.BRUSH_SPHERE, hip.EDIT_FILL)
    assert ctx.edit_voxels(corner) == 1                                 # an edit that changes a voxel
    gone()
    ctx.label_components(cr.SET_SOLID, cr.CONN_FACE)
    v, tris = _box_mesh([0.3, 0.3, 0.3], [0.7, 0.7, 0.7])
    ctx.voxelize_mesh(v, tris, np.float32(0.125), grid=((8, 8, 8), np.zeros(3, np.float32), np.float32(0.125)))     # voxelize
    gone()
    ctx.label_components(cr.SET_SOLID, cr.CONN_FACE)
    ctx.upload_octree(scenes("sphere64").nodes, g.min, g.voxel_size)    # upload: no grid either
    gone()
    for call in (lambda: ctx.label_components(cr.SET_SOLID, cr.CONN_FACE),
                 lambda: ctx.edit_components(cr.SET_SOLID, cr.CONN_FACE, cr.SELECT_ENCLOSED)):
        with pytest.raises(hip.RtoError) as e:
            call()
        assert e.value.code == hip.RTO_E_UNSUPPORTED
    fresh = hip.Context(0)
    try:
        with pytest.raises(hip.RtoError) as e:
            fresh.label_components(cr.SET_SOLID, cr.CONN_FACE)
        assert e.value.code == hip.RTO_E_NO_OCTREE
        with pytest.raises(hip.RtoError) as e:
            fresh.edit_components(cr.SET_SOLID, cr.CONN_FACE, cr.SELECT_ENCLOSED)
        assert e.value.code == hip.RTO_E_NO_OCTREE
    finally:
        fresh.close()


@gpu
def test_gpu_unchanged_component_edit_touches_nothing(ctx, orc, scenes, camera):
    from conftest import make_camera
    hip = _hip()
    g = scenes("sphere64").grid
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    ctx.build_leaf_triangles(None)
    view, _ = make_camera(orc, 0.5, 0.7, 1.8)
    ctx.update_frustum(view, FOV, W / H, True)
    table = ctx.label_components(cr.SET_EMPTY, cr.CONN_FACE)
    labels = ctx.component_labels()
    nodes, tris, info = ctx.download_nodes(), ctx.download_leaf_triangles(), bytes(ctx.info())
    assert ctx.info().culling_active == 1
    assert ctx.edit_components(cr.SET_SOLID, cr.CONN_FACE, cr.SELECT_SMALLER_THAN, 1) == 0       # nothing is smaller than 1
    assert ctx.edit_components(cr.SET_SOLID, cr.CONN_FACE, cr.SELECT_ALL_BUT_LARGEST) == 0       # one solid component
    assert ctx.edit_components(cr.SET_SOLID, cr.CONN_FACE, cr.SELECT_CONTAINING, 0) == 0         # voxel 0 is EMPTY
    assert bytes(ctx.info()) == info and ctx.info().culling_active == 1
    assert ctx.download_nodes().tobytes() == nodes.tobytes()
    t2 = ctx.download_leaf_triangles()
    assert t2[0].tobytes() == tris[0].tobytes() and t2[1].tobytes() == tris[1].tobytes()
    assert np.array_equal(ctx.component_labels(), labels) and ctx.components().tobytes() == table.tobytes()   # the EMPTY labelling stays
    assert np.array_equal(ctx.download_voxels(), g.data)


@gpu
def test_gpu_component_errors_leave_the_context_untouched(ctx, scenes):
    hip = _hip()
    g = scenes("sphere64").grid
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    table = ctx.label_components(cr.SET_SOLID, cr.CONN_FULL)
    labels, nodes, info = ctx.component_labels(), ctx.download_nodes(), bytes(ctx.info())
    nvox = g.data.size
    L, h = ctx._L, ctx._h
    n = C.c_int64(-5)
    buf = np.zeros(max(len(table), 1), hip.COMPONENT_DTYPE)
    small = np.zeros(nvox - 1, np.int32)
    cases = [
        ("unknown set", lambda: L.rto_label_components(h, 2, 6, C.byref(n))),
        ("unknown connectivity", lambda: L.rto_label_components(h, 1, 18, C.byref(n))),
        ("unknown set (edit)", lambda: L.rto_edit_components(h, -1, 6, 0, 0, C.byref(n))),
        ("unknown connectivity (edit)", lambda: L.rto_edit_components(h, 1, 0, 0, 0, C.byref(n))),
        ("unknown selection", lambda: L.rto_edit_components(h, 1, 6, 5, 0, C.byref(n))),
        ("negative selection", lambda: L.rto_edit_components(h, 1, 6, -1, 0, C.byref(n))),
        ("smaller than a negative", lambda: L.rto_edit_components(h, 1, 6, hip.SELECT_SMALLER_THAN, -1, C.byref(n))),
        ("containing a negative", lambda: L.rto_edit_components(h, 1, 6, hip.SELECT_CONTAINING, -1, C.byref(n))),
        ("not containing a negative", lambda: L.rto_edit_components(h, 1, 6, hip.SELECT_NOT_CONTAINING, -1, C.byref(n))),
        ("containing the voxel count", lambda: L.rto_edit_components(h, 1, 6, hip.SELECT_CONTAINING, nvox, C.byref(n))),
        ("not containing beyond", lambda: L.rto_edit_components(h, 1, 6, hip.SELECT_NOT_CONTAINING, nvox + 7, C.byref(n))),
        ("table capacity", lambda: L.rto_download_components(h, buf.ctypes.data, len(table) - 1, C.byref(n))),
        ("label capacity", lambda: L.rto_download_labels(h, small.ctypes.data, nvox - 1)),
    ]
    for what, call in cases:
        assert call() == hip.RTO_E_INVALID, what
        assert L.rto_last_error(h), what
        assert ctx.download_nodes().tobytes() == nodes.tobytes() and bytes(ctx.info()) == info, what
        assert np.array_equal(ctx.download_voxels(), g.data), what
        assert np.array_equal(ctx.component_labels(), labels) and ctx.components().tobytes() == table.tobytes(), what
    # a negative arg is no error where the selection takes none
    assert ctx.edit_components(cr.SET_SOLID, cr.CONN_FACE, cr.SELECT_ALL_BUT_LARGEST, -3) == 0
