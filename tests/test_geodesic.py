"""Geodesic distance fields, paths and flood edits (rto_geodesic_field, rto_download_geodesic, rto_geodesic_device,
rto_geodesic_paths, rto_edit_geodesic, Context.geodesic_field / geodesic_paths / edit_geodesic, RayTracerBVH::geodesicField /
pathsTo / floodFrom / farthestPoint).  CPU: the heap Dijkstra of tests/geodesic_ref.py against scipy's Dijkstra on the explicit
move graph and against the component rule, limits, paths, floods, the host layer's bucket queue, the ABI, the kernels' budgets, the
sanitizer script.  GPU: fields and summaries bit for bit against the rule on grids chosen around k_geo_relax's 32 x 8 x 8 tile and
its two load forms, the pass counts, paths, flood edits against the rule, a fresh build and the oracle's frame; state and errors."""
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
import geodesic_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("rto_geodesic_field", "rto_download_geodesic", "rto_geodesic_device", "rto_geodesic_paths", "rto_edit_geodesic",
        "rto_last_geodesic_ms", "rto_last_geodesic_edit_ms", "rto_debug_geodesic_passes", "rto_debug_set_geodesic_look")
MEDIA = (gr.SET_EMPTY, gr.SET_SOLID)
CONNS = (gr.CONN_FACE, gr.CONN_FULL)
TILE = (32, 8, 8)           # k_geo_relax's tile, x, y, z (rto_geodesic.inc)
# VGPRs and LDS bytes the build gives; a kernel that grows past its line here has changed
GEO_VGPR = {"k_geo_fill": 6, "k_geo_seeds": 13, "k_geo_relax": 38, "k_geo_paths": 20}
GEO_LDS = {"k_geo_fill": 0, "k_geo_seeds": 0, "k_geo_relax": 13864, "k_geo_paths": 0}


def _hip():
    from ray_tracing_octrees_amd import hip
    return hip


def _tc():
    import test_components as tc          # its scenes and its checks of a rebuilt context
    return tc


# ================================================================ grids
def _random(shape_xyz, fill, seed):
    x, y, z = shape_xyz
    return (np.random.default_rng(seed).random((z, y, x)) < fill).astype(np.uint8)


def _axis_grids():
    """Per axis: T - 1, T, T + 1 and 2 T + 1 voxels on that axis, 5 and 3 on the others."""
    out = {}
    for axis, t in enumerate(TILE):
        for n in (t - 1, t, t + 1, 2 * t + 1):
            dims = [5, 3, 3]
            if axis == 1:
                dims = [5, n, 3]
            elif axis == 2:
                dims = [5, 3, n]
            else:
                dims = [n, 5, 3]
            out[f"{'xyz'[axis]}{n}"] = (tuple(dims), 0.3, 500 + 10 * axis + n)
    return out


AXIS = _axis_grids()
LONG = {"long_x": ((200, 3, 3), 0.02, 301), "long_y": ((3, 200, 3), 0.02, 302), "long_z": ((3, 3, 200), 0.02, 303)}
OTHER = ["wide48", "one_filled", "one_empty", "all_medium", "no_medium", "pocket", "two_components", "thousand_seeds", "r33", "maze"]
GRIDS = [*sorted(AXIS), *sorted(LONG), *OTHER]


def _pocket():
    g = np.ones((5, 7, 9), np.uint8)
    g[2, 3, 4] = 0                                                      # one EMPTY voxel walled in on all 26 sides
    g[0, 0, :] = 0                                                      # and an EMPTY row elsewhere
    return g


def _two_components():
    g = np.zeros((9, 10, 40), np.uint8)
    g[:, :, 19:21] = 1                                                  # a wall two voxels thick splits the EMPTY space
    return g


def _named(name, scenes=None):
    """(grid, seeds) of a named case; the seeds are linear indices."""
    if name in AXIS or name in LONG:
        g = _random(*(AXIS.get(name) or LONG[name]))
        flat = g.reshape(-1)
        seeds = [0, g.size // 2, g.size - 1]
        for m in MEDIA:                                                 # the first and the last voxel of each medium, so that both have a seed
            at = np.flatnonzero(flat == m)
            if at.size:
                seeds += [int(at[0]), int(at[-1])]
        return g, np.asarray(seeds, np.int64)
    if name == "wide48":
        g = _random((48, 9, 9), 0.3, 77)
        return g, np.asarray([0, 1, g.size // 2, g.size - 1, g.size - 2], np.int64)
    if name == "one_filled":
        return np.ones((1, 1, 1), np.uint8), np.asarray([0], np.int64)
    if name == "one_empty":
        return np.zeros((1, 1, 1), np.uint8), np.asarray([0], np.int64)
    if name == "all_medium":
        return np.zeros((12, 20, 40), np.uint8), np.asarray([0], np.int64)
    if name == "no_medium":                                             # for the EMPTY medium; all of it for SOLID
        return np.ones((9, 9, 33), np.uint8), np.asarray([0, 100, 2672], np.int64)
    if name == "pocket":
        return _pocket(), np.asarray([4 + 9 * (3 + 7 * 2)], np.int64)
    if name == "two_components":
        return _two_components(), np.asarray([0, 39], np.int64)
    if name == "thousand_seeds":
        g = _random((40, 17, 9), 0.4, 91)
        s = np.random.default_rng(92).integers(0, g.size, 1000)
        s[500:] = s[:500]                                               # duplicates; about 40 % lie outside either medium
        return g, s.astype(np.int64)
    if name == "r33":
        g = _random((33, 33, 33), 0.6, 41)
        return g, np.asarray([0, 5, 17000, 35936], np.int64)
    if name == "maze":
        return gr.maze(), np.asarray([0], np.int64)
    if name == "odd37":
        g = _tc()._odd37()
        return g, np.asarray([0, g.size // 2], np.int64)
    g = np.ascontiguousarray(scenes(name).grid.data, np.uint8)
    return g, np.asarray([0, g.size // 2], np.int64)


_REF = {}


def _ref(name, grid, seeds, medium, conn):
    """The rule's unlimited field, computed once per (grid, medium, connectivity) and shared; the limited ones are thresholds of it."""
    key = (name, medium, conn)
    if key not in _REF:
        g = gr.field(grid, seeds, medium, conn)
        g.setflags(write=False)
        _REF[key] = g
    return _REF[key]


def _limits(full):
    m = int(gr.summary(full)["max_g"])
    return (None, 7, max(m - 1, 0))


# ================================================================ CPU: the rule
def test_rule_by_hand():
    g = np.zeros((1, 3, 5), np.uint8)
    g[0, :2, 2] = 1                                                     # a wall with a gap in the last row
    f = gr.field(g, [0], gr.SET_EMPTY, gr.CONN_FACE)
    assert f[0].tolist() == [[0, 1, gr.NONE, 7, 8], [1, 2, gr.NONE, 6, 7], [2, 3, 4, 5, 6]]
    c = gr.field(g, [0], gr.SET_EMPTY, gr.CONN_FULL)
    assert c[0].tolist() == [[0, 3, gr.NONE, 15, 16], [3, 4, gr.NONE, 12, 15], [6, 7, 8, 11, 14]]
    s = gr.field(g, [2, 0], gr.SET_SOLID, gr.CONN_FACE)                 # the seed at 0 is not in the medium: ignored
    assert s[0, 0, 2] == 0 and s[0, 1, 2] == 1 and int((s != gr.NONE).sum()) == 2
    sm = gr.summary(f)
    assert (sm["max_g"], sm["argmax"], sm["reached"], sm["reserved"]) == (8, 4, 13, 0)
    none = gr.summary(gr.field(g, [2], gr.SET_EMPTY, gr.CONN_FACE))
    assert (none["max_g"], none["argmax"], none["reached"]) == (-1, -1, 0)
    # a diagonal move between two medium voxels is allowed whatever the voxels beside it hold
    d = np.ones((1, 2, 2), np.uint8)
    d[0, 0, 0] = d[0, 1, 1] = 0
    assert gr.field(d, [0], gr.SET_EMPTY, gr.CONN_FULL)[0, 1, 1] == 4 and gr.field(d, [0], gr.SET_EMPTY, gr.CONN_FACE)[0, 1, 1] == gr.NONE
    for bad in ([], [-1], [15]):
        with pytest.raises(ValueError):
            gr.field(g, bad)
    with pytest.raises(ValueError):
        gr.field(g, [0], limit=-1)


WITNESS = {"r17": ((17, 9, 5), 0.3, 1), "r20": ((20, 12, 7), 0.45, 2), "r33": ((33, 33, 33), 0.6, 41)}


@pytest.mark.parametrize("name", sorted(WITNESS))
def test_rule_equals_scipy_dijkstra_and_the_component_rule(name):
    """The second witness (scipy's Dijkstra on the explicit move graph) and the third (the finite voxels are the components that
    hold a seed), for both media and both connectivities."""
    pytest.importorskip("scipy.sparse.csgraph")
    g = _random(*WITNESS[name])
    seeds = np.asarray([0, g.size // 3, g.size // 2, g.size - 1], np.int64)
    for m in MEDIA:
        for conn in CONNS:
            f = gr.field(g, seeds, m, conn)
            assert f.dtype == np.int32 and np.array_equal(f, gr.scipy_field(g, seeds, m, conn)), (name, m, conn)
            labels, _ = cr.label(g, m, conn)
            flat = labels.reshape(-1)
            held = {int(flat[s]) for s in seeds if flat[s] >= 0}
            assert np.array_equal(f != gr.NONE, np.isin(labels, sorted(held)) & (labels >= 0)), (name, m, conn)
            assert ((f == 0) == (np.isin(np.arange(g.size), seeds).reshape(g.shape) & (g == m))).all()


@pytest.mark.parametrize("name", ["x33", "maze", "r33", "two_components"])
def test_rule_limited_field_is_the_thresholded_one(name):
    g, seeds = _named(name)
    for m in MEDIA:
        for conn in CONNS:
            full = _ref(name, g, seeds, m, conn)
            for limit in (0, 1, 7, max(int(gr.summary(full)["max_g"]) - 1, 0)):
                assert np.array_equal(gr.field(g, seeds, m, conn, limit), gr.threshold(full, limit)), (name, m, conn, limit)
            assert np.array_equal(gr.field(g, seeds, m, conn, gr.NO_LIMIT), full)


def test_the_maze_is_a_maze():
    """The condition the GPU tests rely on: every EMPTY voxel is reached and the longest way is at least 10 times the largest
    dimension, so a shortest path re-enters the same tile many times."""
    g, seeds = _named("maze")
    assert g.shape == (5, 21, 37)
    sm = gr.summary(_ref("maze", g, seeds, gr.SET_EMPTY, gr.CONN_FACE))
    assert sm["reached"] == int((g == 0).sum()) and sm["max_g"] >= 10 * 37
    assert sm["max_g"] == sm["reached"] - 1                             # one corridor, walked end to end


def _check_paths(g, f, conn, targets, rows, lengths, medium):
    mv = {(mz, my, mx): w for mz, my, mx, w in gr.moves(conn)}
    dz, dy, dx = g.shape
    flat, gf = f.reshape(-1), g.reshape(-1)
    for t, row, n in zip(targets, rows, lengths):
        if flat[t] == gr.NONE:
            assert n == -1 and (row == -1).all()
            continue
        p = row[:n]
        assert p[0] == t and (row[n:] == -1).all() and flat[p[-1]] == 0 and (gf[p] == medium).all()
        total = 0
        for a, b in zip(p[:-1], p[1:]):
            d = (int(b // (dx * dy) - a // (dx * dy)), int((b // dx) % dy - (a // dx) % dy), int(b % dx - a % dx))
            assert d in mv, (t, a, b)                                   # consecutive voxels are neighbours under the connectivity
            assert flat[a] - flat[b] == mv[d]                           # g falls by exactly the move's weight
            total += mv[d]
        assert total == flat[t]


def test_rule_paths():
    g, seeds = _named("x33")
    for m in MEDIA:
        for conn in CONNS:
            f = _ref("x33", g, seeds, m, conn)
            targets = np.arange(g.size)
            longest = int(gr.paths(f, conn, targets, 0)[1].max())
            rows, lengths = gr.paths(f, conn, targets, longest)
            assert int((lengths > 0).sum()) == int((f != gr.NONE).sum()) > 0
            _check_paths(g, f, conn, targets, rows, lengths, m)
            cut, lengths2 = gr.paths(f, conn, targets, 2)
            assert np.array_equal(lengths2, lengths) and np.array_equal(cut, rows[:, :2])
    # the tie rule: (1, 1) is reached from (1, 0), index 1, and from (0, 1), index 3: the smaller index is the path's
    t = np.zeros((1, 3, 3), np.uint8)
    f = gr.field(t, [0], gr.SET_EMPTY, gr.CONN_FACE)
    assert f[0, 0, 1] == f[0, 1, 0] == 1 and f[0, 1, 1] == 2
    rows, lengths = gr.paths(f, gr.CONN_FACE, [4, 8], 6)
    assert rows.tolist() == [[4, 1, 0, -1, -1, -1], [8, 5, 2, 1, 0, -1]] and lengths.tolist() == [3, 5]
    # under the chamfer (1, 1) comes straight from 0 (4), and (2, 1), index 5, from 1 (3 + 4) rather than from 4 (4 + 3)
    fc = gr.field(t, [0], gr.SET_EMPTY, gr.CONN_FULL)
    assert gr.paths(fc, gr.CONN_FULL, [4, 5], 4)[0].tolist() == [[4, 0, -1, -1], [5, 1, 0, -1]]
    # a limited field still has a predecessor for every finite voxel
    lim = gr.threshold(f, 2)
    rows, lengths = gr.paths(lim, gr.CONN_FACE, [4, 8], 3)
    assert rows.tolist() == [[4, 1, 0], [-1, -1, -1]] and lengths.tolist() == [3, -1]


@pytest.mark.parametrize("name", ["x33", "r33", "two_components", "pocket"])
def test_rule_flood(name):
    g, seeds = _named(name)
    for m in MEDIA:
        for conn in CONNS:
            one = [int(seeds[0])]
            want, changed = cr.apply_selection(g, m, conn, cr.SELECT_CONTAINING, one[0])
            got, n = gr.flood(g, one, m, conn)
            assert n == changed and np.array_equal(got, want), (name, m, conn)
            full = _ref(name, g, seeds, m, conn)
            for limit in (0, 7):
                got, n = gr.flood(g, seeds, m, conn, limit)
                hit = full <= limit
                assert n == int(hit.sum()) and np.array_equal(got != g, hit), (name, m, conn, limit)


@pytest.mark.parametrize("name", GRIDS)
def test_reference_equals_the_host_layers_bucket_queue(name):
    """tests/geodesic_ref.py against geodesicFieldCPU / geodesicPathsCPU / floodGeodesicCPU (host/Geodesic.cpp), summary bytes
    included."""
    import ray_tracing_octrees_amd as rto
    g, seeds = _named(name)
    vg = rto.VoxelGrid.from_array(g, (0.0, 0.0, 0.0), 1.0)
    for m in MEDIA:
        for conn in CONNS:
            full = _ref(name, g, seeds, m, conn)
            for limit in _limits(full):
                want = gr.threshold(full, limit)
                rc, f, sm = vg.geodesicField(seeds, m, conn, gr.NO_LIMIT if limit is None else limit)
                assert rc == 0 and np.array_equal(f, want), (name, m, conn, limit)
                assert sm.tobytes() == gr.summary(want).tobytes(), (name, m, conn, limit, sm)
            targets = np.asarray([0, g.size // 2, g.size - 1, int(gr.summary(full)["argmax"]) if gr.summary(full)["reached"] else 0])
            wr, wl = gr.paths(full, conn, targets, 9)
            rc, rows, lengths = vg.geodesicPaths(full, targets, 9, conn)
            assert rc == 0 and np.array_equal(rows, wr) and np.array_equal(lengths, wl), (name, m, conn)
            edit = rto.VoxelGrid.from_array(g, (0.0, 0.0, 0.0), 1.0)
            want, changed = gr.flood(g, seeds, m, conn, 7)
            assert edit.floodGeodesic(seeds, m, conn, 7) == changed and np.array_equal(edit.data, want), (name, m, conn)


def test_host_layer_refusals():
    import ray_tracing_octrees_amd as rto
    hip = _hip()
    g, _ = _named("x33")
    vg = rto.VoxelGrid.from_array(g, (0.0, 0.0, 0.0), 1.0)
    f = gr.field(g, [0])
    for args in (([0], 2, 6), ([0], -1, 6), ([0], 0, 18), ([0], 0, 6, -1), ([], 0, 6), ([-1], 0, 6), ([g.size], 0, 6)):
        rc, out, _ = vg.geodesicField(*args)
        assert rc == hip.RTO_E_INVALID and out is None, args
        assert vg.floodGeodesic(*args) == hip.RTO_E_INVALID and np.array_equal(vg.data, g), args
    for args in ((f, [], 3), (f, [-1], 3), (f, [g.size], 3), (f, [0], -1), (f, [0], 3, 7)):
        assert vg.geodesicPaths(*args)[0] == hip.RTO_E_INVALID, args[1:]
    rc, rows, lengths = vg.geodesicPaths(f, [0, 1], 0)
    assert rc == 0 and rows.shape == (2, 0) and lengths.tolist() == gr.paths(f, gr.CONN_FACE, [0, 1], 0)[1].tolist()


def test_geodesic_abi_layout_and_exports():
    """sizeof(rto_geo_summary) == 32 with the fields where GEO_SUMMARY_DTYPE puts them; the new symbols are exported."""
    hip = _hip()
    assert hip.GEO_SUMMARY_DTYPE.itemsize == 32 and gr.SUMMARY_DTYPE == hip.GEO_SUMMARY_DTYPE
    fields = ("max_g", "argmax", "reached", "reserved")
    assert [hip.GEO_SUMMARY_DTYPE.fields[f][1] for f in fields] == [0, 8, 16, 24]
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.fail("no C compiler: the header's layout cannot be checked")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "abi.c")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "rto_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d %d %d\\n", '
                    'sizeof(rto_geo_summary), offsetof(rto_geo_summary, max_g), offsetof(rto_geo_summary, argmax), '
                    'offsetof(rto_geo_summary, reached), offsetof(rto_geo_summary, reserved), RTO_DIST_NONE, RTO_CONN_FACE, '
                    'RTO_CONN_FULL); return 0; }\n')
        exe = os.path.join(tmp, "abi")
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert out == [str(v) for v in (32, 0, 8, 16, 24, gr.NONE, gr.CONN_FACE, gr.CONN_FULL)]
    assert (gr.NONE, gr.NO_LIMIT) == (hip.DIST_NONE, hip.GEO_NO_LIMIT)
    L = hip.load()
    header = open(os.path.join(ROOT, "include", "rto_hip.h")).read()
    for s in SYMS:
        assert s in hip.SYMBOLS and hasattr(L, s), s
        assert s + "(" in header, s


def test_geodesic_kernels_keep_their_budgets():
    """The built assembly (the product's flags): every k_geo_* kernel without scratch, spills or v_mfma, within the VGPR and LDS
    figures DESIGN.md section 20 states; the wide form of k_geo_relax loads the grid with dwordx4 accesses."""
    import test_isa_contract as isa
    asm = isa.built_asm()
    if asm is None:
        pytest.fail("no hipcc: the budget cannot be checked")
    meta = isa.kernel_meta(asm)
    names = [k for k in meta if "k_geo_" in k]
    assert len(names) == 8, names               # fill, seeds, relax x4, paths x2
    seen = set()
    for k in names:
        m = meta[k]
        base = next(b for b in GEO_VGPR if b in k)
        seen.add(base)
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (k, m)
        assert m["vgpr"] <= GEO_VGPR[base], (k, m)
        entry = re.search(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\.group_segment_fixed_size).)*?\.name:\s+" + re.escape(k) + r"\n", asm, re.S)
        assert entry and int(entry.group(1)) <= GEO_LDS[base], (k, entry and entry.group(1))
        ins = isa.body(asm, k[len("_ZN3rto"):])
        assert not any(t.startswith(("scratch_", "buffer_load", "buffer_store")) or "v_mfma" in t for t in ins), k
        if "k_geo_relaxILb1E" in k:
            assert any(t.startswith("global_load_dwordx4") for t in ins), k
    assert seen == set(GEO_VGPR)


def test_sanitizer_script_reports_nothing():
    """tools/sanitize_geodesic.sh: host/Geodesic.cpp as a stand-alone program under AddressSanitizer and UBSan."""
    if not shutil.which("g++"):
        pytest.fail("no g++: the sanitizer build cannot be made")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize_geodesic.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "geodesic selftest ok" in r.stdout and "UBSan reports: 0" in r.stdout and "ASan reports: 0" in r.stdout, r.stdout


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


def _check_fields(ctx, name, g, seeds, expected):
    """Field, summary and pass count for both media, both connectivities, no limit and two limits; expected(m, conn) is the
    unlimited field."""
    cap = g.size + 2
    for m in MEDIA:
        for conn in CONNS:
            full = expected(m, conn)
            for limit in _limits(full):
                want = gr.threshold(full, limit)
                what = f"{name} medium {m} conn {conn} limit {limit}"
                got, gs = ctx.geodesic_field(seeds, m, conn, limit)
                assert got.dtype == np.int32 and got.shape == g.shape, what
                assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} voxels differ"
                assert gs.tobytes() == gr.summary(want).tobytes(), (what, gs)
                assert all(t >= 0 for t in ctx.last_geodesic_ms()), what
                passes, tiles = ctx.geodesic_passes(tiles=True)
                assert 2 <= passes <= cap and tiles >= 1, (what, passes, tiles)


@gpu
@pytest.mark.parametrize("name", GRIDS)
def test_gpu_field_and_summary_equal_the_rule(ctx, name, path):
    g, seeds = _named(name)
    _build(ctx, g)
    _check_fields(ctx, name, g, seeds, lambda m, conn: _ref(name, g, seeds, m, conn))


@gpu
@pytest.mark.parametrize("name", ["sphere64", "odd37"])
def test_gpu_field_of_the_suites_scenes_equals_the_host_layers(ctx, scenes, name):
    """The expected field is the host layer's bucket queue, which the CPU tests pin to the rule."""
    import ray_tracing_octrees_amd as rto
    g, seeds = _named(name, scenes)
    vg = rto.VoxelGrid.from_array(g, (0.0, 0.0, 0.0), 1.0)
    _build(ctx, g)

    def expected(m, conn):
        rc, f, _ = vg.geodesicField(seeds, m, conn)
        assert rc == 0
        return f
    _check_fields(ctx, name, g, seeds, expected)


@gpu
def test_gpu_geodesic_device_pointer_holds_the_download(ctx):
    g, seeds = _named("r33")
    _build(ctx, g)
    got, _ = ctx.geodesic_field(seeds, gr.SET_SOLID, gr.CONN_FULL)
    p = ctx.geodesic_device()
    assert p and _tc()._d2h(p, 4 * g.size).tobytes() == got.tobytes() == _ref("r33", g, seeds, gr.SET_SOLID, gr.CONN_FULL).tobytes()
    assert ctx.geodesic().tobytes() == got.tobytes()


@gpu
def test_gpu_passes_and_looks(ctx):
    """The maze needs more launches than the open grid; the field is the same bit for bit whether the host looks at the device
    after every launch or after every 8 (and 64).  The figures are printed for DESIGN.md, not asserted beyond that."""
    counts = {}
    try:
        for name in ("all_medium", "maze"):
            g, seeds = _named(name)
            _build(ctx, g)
            fields = []
            for look in (1, 8, 64):
                ctx.debug_set_geodesic_look(look)
                for conn in CONNS:
                    f, sm = ctx.geodesic_field(seeds, gr.SET_EMPTY, conn)
                    fields.append((conn, f.tobytes(), sm.tobytes()))
                    assert f.tobytes() == _ref(name, g, seeds, gr.SET_EMPTY, conn).tobytes(), (name, look, conn)
                    counts[(name, look, conn)] = ctx.geodesic_passes(tiles=True)
                    assert 2 <= counts[(name, look, conn)][0] <= g.size + 2
            for conn, f, sm in fields:
                assert (f, sm) == next((a, b) for c, a, b in fields if c == conn)
        print("geodesic passes (launches, tiles run):", counts)
        for look in (1, 8, 64):
            for conn in CONNS:
                assert counts[("maze", look, conn)][0] > counts[("all_medium", look, conn)][0], (look, conn, counts)
        with pytest.raises(_hip().RtoError):
            ctx.debug_set_geodesic_look(0)
        with pytest.raises(_hip().RtoError):
            ctx.debug_set_geodesic_look(65)
    finally:
        ctx.debug_set_geodesic_look(8)


@gpu
def test_gpu_paths_equal_the_rule(ctx):
    hip = _hip()
    g, seeds = _named("x33")                                            # T + 1 along x
    _build(ctx, g)
    targets = np.arange(g.size)
    for m in MEDIA:
        for conn in CONNS:
            full = _ref("x33", g, seeds, m, conn)
            for limit in (None, 7):
                f = gr.threshold(full, limit)
                ctx.geodesic_field(seeds, m, conn, limit)
                longest = int(gr.paths(f, conn, targets, 0)[1].max())
                for max_len in (longest, 2, 0):                          # whole paths, shorter than most paths, lengths alone
                    wr, wl = gr.paths(f, conn, targets, max_len)
                    rows, lengths = ctx.geodesic_paths(targets, max_len)
                    assert rows.shape == (g.size, max_len) and np.array_equal(lengths, wl), (m, conn, limit, max_len)
                    assert np.array_equal(rows, wr), (m, conn, limit, max_len)
                assert (wl == -1).any() and (wl > 0).any()               # unreachable targets and reached ones
    # (i, j, k) targets; the far end of the maze
    g, seeds = _named("maze")
    _build(ctx, g)
    f, sm = ctx.geodesic_field(seeds, gr.SET_EMPTY, gr.CONN_FACE)
    far = int(sm["argmax"])
    ijk = np.asarray([[far % 37, (far // 37) % 21, far // (37 * 21)]])
    rows, lengths = ctx.geodesic_paths(ijk, 2000)
    wr, wl = gr.paths(f, gr.CONN_FACE, [far], 2000)
    assert lengths.tolist() == wl.tolist() == [int(sm["max_g"]) + 1] and np.array_equal(rows, wr) and rows[0, lengths[0] - 1] == 0
    # the connectivity is the field's own
    ctx.geodesic_field(seeds, gr.SET_EMPTY, gr.CONN_FULL)
    fc = _ref("maze", g, seeds, gr.SET_EMPTY, gr.CONN_FULL)
    rows, lengths = ctx.geodesic_paths([far], 2000)
    wr, wl = gr.paths(fc, gr.CONN_FULL, [far], 2000)
    assert np.array_equal(lengths, wl) and np.array_equal(rows, wr)
    assert hip.RTO_OK == 0


def _flood_cases(data):
    flat = data.reshape(-1)
    empty, solid = np.flatnonzero(flat == 0), np.flatnonzero(flat == 1)
    return [("empty face limit 12", gr.SET_EMPTY, gr.CONN_FACE, [int(empty[0]), int(empty[len(empty) // 2])], 12),
            ("solid full limit 20", gr.SET_SOLID, gr.CONN_FULL, [int(solid[len(solid) // 2]), int(solid[0]), int(empty[0])], 20),
            ("solid face no limit", gr.SET_SOLID, gr.CONN_FACE, [int(solid[len(solid) // 2])], None)]


@gpu
@pytest.mark.parametrize("triangles", [False, True])
@pytest.mark.parametrize("name", ["odd37", "sphere64"])
def test_gpu_flood_edits_equal_the_rule_and_a_fresh_build(ctx, ctx2, orc, scenes, camera, name, path, triangles):
    """With a limit the grid is the rule's; the nodes are a fresh build's on a second context; the frame is the oracle's; resident
    leaf triangles are rebuilt.  With no limit grid and nodes equal edit_components(CONTAINING) run on the second context."""
    tc = _tc()
    hip = _hip()
    data, gmin, vox, view, pos = tc._scene(orc, scenes, camera, name)
    ctx.set_kernel(hip.KERNEL_AUTO)
    for label, m, conn, seeds, limit in _flood_cases(data):
        what = f"{name} {path} {label} triangles {triangles}"
        ctx.build_octree(data, gmin, vox)
        if triangles:
            ctx.build_leaf_triangles(None)
        want, want_changed = gr.flood(data, seeds, m, conn, limit)
        assert want_changed > 0
        assert ctx.edit_geodesic(seeds, m, conn, limit) == want_changed, what
        ms = ctx.last_geodesic_edit_ms()
        assert ms[0] >= 0 and ms[1] >= 0 and (ms[2] >= 0) == triangles, (what, ms)
        og, nodes = tc._check_rebuilt(ctx, ctx2, orc, gmin, vox, want, what)
        if triangles:
            ctx2.build_leaf_triangles(None)
            t1, o1 = ctx.download_leaf_triangles()
            t2, o2 = ctx2.download_leaf_triangles()
            assert t1.tobytes() == t2.tobytes() and o1.tobytes() == o2.tobytes(), f"{what}: leaf triangles"
        tc._check_render(ctx, orc, og, nodes, view, pos, what)
        assert ctx.info().culling_active == 0
        if limit is None:
            ctx2.build_octree(data, gmin, vox)
            assert ctx2.edit_components(m, conn, hip.SELECT_CONTAINING, seeds[0]) == want_changed, what
            assert np.array_equal(ctx2.download_voxels(), ctx.download_voxels()), what
            assert ctx2.download_nodes().tobytes() == ctx.download_nodes().tobytes(), what


@gpu
def test_gpu_geodesic_field_is_dropped_when_the_grid_changes(ctx, scenes):
    hip = _hip()
    tc = _tc()
    g = scenes("sphere64").grid

    def gone():
        for read in (ctx.geodesic, ctx.geodesic_device, lambda: ctx.geodesic_paths([0], 4)):
            with pytest.raises(hip.RtoError) as e:
                read()
            assert e.value.code == hip.RTO_E_INVALID and "no geodesic field is resident" in str(e.value)

    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    gone()                                                              # never made
    ctx.geodesic_field([0])
    ctx.geodesic()
    ctx.build_octree(g.data, g.min, g.voxel_size)                       # build
    gone()
    # labels and the Euclidean field survive a geodesic_field call, and it survives theirs
    table = ctx.label_components(1, 6)
    labels = ctx.component_labels()
    dist, _ = ctx.distance_field(1)
    geo, _ = ctx.geodesic_field([0], gr.SET_EMPTY, gr.CONN_FULL, 200)
    assert np.array_equal(ctx.component_labels(), labels) and ctx.components().tobytes() == table.tobytes()
    assert np.array_equal(ctx.distance(), dist)
    ctx.label_components(0, 26)
    ctx.distance_field(0)
    assert np.array_equal(ctx.geodesic(), geo)
    corner = hip.make_brushes([np.asarray(g.min, np.float32) + np.float32(0.5) * g.voxel_size], 0.5 * float(g.voxel_size),
                              hip.BRUSH_SPHERE, hip.EDIT_FILL)
    assert ctx.edit_voxels(corner) == 1                                 # rto_edit_voxels
    gone()
    ctx.geodesic_field([1])
    assert ctx.edit_components(1, 6, hip.SELECT_SMALLER_THAN, 2) == 1   # rto_edit_components: the corner voxel is debris
    gone()
    ctx.geodesic_field([0])
    assert ctx.edit_morphology(hip.MORPH_DILATE, g.voxel_size) > 0      # rto_edit_morphology
    gone()
    ctx.geodesic_field([0])
    ctx.label_components(1, 6)
    ctx.distance_field(1)
    want_changed = gr.flood(ctx.download_voxels(), [0], gr.SET_EMPTY, gr.CONN_FACE, 3)[1]
    assert ctx.edit_geodesic([0], gr.SET_EMPTY, gr.CONN_FACE, 3) == want_changed > 0      # rto_edit_geodesic: drops all three
    gone()
    for read in (ctx.component_labels, ctx.distance):
        with pytest.raises(hip.RtoError) as e:
            read()
        assert e.value.code == hip.RTO_E_INVALID
    ctx.geodesic_field([0], gr.SET_SOLID)
    v, tris = tc._box_mesh([0.3, 0.3, 0.3], [0.7, 0.7, 0.7])
    ctx.voxelize_mesh(v, tris, np.float32(0.125), grid=((8, 8, 8), np.zeros(3, np.float32), np.float32(0.125)))     # voxelize
    gone()
    ctx.geodesic_field([0])
    ctx.upload_octree(scenes("sphere64").nodes, g.min, g.voxel_size)    # upload: no grid either
    gone()


@gpu
def test_gpu_unchanged_flood_touches_nothing(ctx, orc, scenes):
    from conftest import make_camera
    hip = _hip()
    g = scenes("sphere64").grid
    data = np.ascontiguousarray(g.data, np.uint8)
    flat = data.reshape(-1)
    solid, empty = int(np.flatnonzero(flat == 1)[0]), int(np.flatnonzero(flat == 0)[0])
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(data, g.min, g.voxel_size)
    ctx.build_leaf_triangles(None)
    view, _ = make_camera(orc, 0.5, 0.7, 1.8)
    ctx.update_frustum(view, FOV, W / H, True)
    assert ctx.info().culling_active == 1
    table = ctx.label_components(0, 6)
    labels = ctx.component_labels()
    dist, _ = ctx.distance_field(gr.SET_EMPTY, np.float32(3.0) * np.float32(g.voxel_size))
    geo, _ = ctx.geodesic_field([empty], gr.SET_EMPTY, gr.CONN_FACE, 30)
    nodes, info = ctx.download_nodes(), bytes(ctx.info())
    tris = ctx.download_leaf_triangles()
    # no seed in the medium: nothing is reached, nothing flipped
    for seeds, m, conn, limit in (([solid], gr.SET_EMPTY, gr.CONN_FACE, None), ([empty, empty], gr.SET_SOLID, gr.CONN_FULL, 0)):
        assert ctx.edit_geodesic(seeds, m, conn, limit) == 0
        assert bytes(ctx.info()) == info and ctx.info().culling_active == 1
        assert ctx.download_nodes().tobytes() == nodes.tobytes()
        t2 = ctx.download_leaf_triangles()
        assert t2[0].tobytes() == tris[0].tobytes() and t2[1].tobytes() == tris[1].tobytes()
        assert np.array_equal(ctx.component_labels(), labels) and ctx.components().tobytes() == table.tobytes()
        assert np.array_equal(ctx.distance(), dist) and np.array_equal(ctx.geodesic(), geo)
        assert np.array_equal(ctx.download_voxels(), data)
        ms = ctx.last_geodesic_edit_ms()
        assert ms[0] >= 0 and ms[1] == -1 and ms[2] == -1


@gpu
def test_gpu_geodesic_errors_leave_the_context_untouched(ctx, orc, scenes):
    from conftest import assert_bit_exact, make_camera
    import ray_tracing_octrees_amd as rto
    hip = _hip()
    g = scenes("sphere64").grid
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    field, _ = ctx.geodesic_field([0], gr.SET_EMPTY, gr.CONN_FACE, 50)
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
    rows, lens = np.zeros((2, 4), np.int64), np.zeros(2, np.int64)
    NL = hip.GEO_NO_LIMIT
    cases = [
        ("unknown medium", lambda: L.rto_geodesic_field(h, 2, 6, ok.ctypes.data, 2, NL, None)),
        ("negative medium", lambda: L.rto_geodesic_field(h, -1, 6, ok.ctypes.data, 2, NL, None)),
        ("unknown connectivity", lambda: L.rto_geodesic_field(h, 0, 18, ok.ctypes.data, 2, NL, None)),
        ("n = 0", lambda: L.rto_geodesic_field(h, 0, 6, ok.ctypes.data, 0, NL, None)),
        ("NULL seeds", lambda: L.rto_geodesic_field(h, 0, 6, None, 2, NL, None)),
        ("negative seed", lambda: L.rto_geodesic_field(h, 0, 6, low.ctypes.data, 2, NL, None)),
        ("seed == voxels", lambda: L.rto_geodesic_field(h, 0, 6, high.ctypes.data, 2, NL, None)),
        ("negative limit", lambda: L.rto_geodesic_field(h, 0, 6, ok.ctypes.data, 2, -1, None)),
        ("edit: unknown medium", lambda: L.rto_edit_geodesic(h, 2, 6, ok.ctypes.data, 2, NL, C.byref(n))),
        ("edit: unknown connectivity", lambda: L.rto_edit_geodesic(h, 0, 7, ok.ctypes.data, 2, NL, C.byref(n))),
        ("edit: n = 0", lambda: L.rto_edit_geodesic(h, 0, 6, ok.ctypes.data, 0, NL, C.byref(n))),
        ("edit: NULL seeds", lambda: L.rto_edit_geodesic(h, 0, 6, None, 1, NL, C.byref(n))),
        ("edit: seed out of range", lambda: L.rto_edit_geodesic(h, 0, 6, high.ctypes.data, 2, NL, C.byref(n))),
        ("edit: negative limit", lambda: L.rto_edit_geodesic(h, 0, 6, ok.ctypes.data, 2, -7, C.byref(n))),
        ("paths: n = 0", lambda: L.rto_geodesic_paths(h, ok.ctypes.data, 0, 4, rows.ctypes.data, lens.ctypes.data)),
        ("paths: NULL targets", lambda: L.rto_geodesic_paths(h, None, 2, 4, rows.ctypes.data, lens.ctypes.data)),
        ("paths: negative target", lambda: L.rto_geodesic_paths(h, low.ctypes.data, 2, 4, rows.ctypes.data, lens.ctypes.data)),
        ("paths: target == voxels", lambda: L.rto_geodesic_paths(h, high.ctypes.data, 2, 4, rows.ctypes.data, lens.ctypes.data)),
        ("paths: negative max_len", lambda: L.rto_geodesic_paths(h, ok.ctypes.data, 2, -1, rows.ctypes.data, lens.ctypes.data)),
        ("paths: NULL rows", lambda: L.rto_geodesic_paths(h, ok.ctypes.data, 2, 4, None, lens.ctypes.data)),
        ("field capacity", lambda: L.rto_download_geodesic(h, small.ctypes.data, nvox - 1)),
    ]
    for what, call in cases:
        assert call() == hip.RTO_E_INVALID, what
        assert L.rto_last_error(h), what
        assert ctx.download_nodes().tobytes() == nodes.tobytes() and bytes(ctx.info()) == info, what
        assert np.array_equal(ctx.download_voxels(), g.data), what
        assert np.array_equal(ctx.geodesic(), field), what
    assert_bit_exact(ctx.render_host(frame), before, "the frame after the refusals")
    # through the host class: the same codes
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    assert rt.geodesicField([0])[0] == hip.RTO_E_NO_OCTREE and rt.floodFrom([0]) == hip.RTO_E_NO_OCTREE
    rt.setOctreeFromGrid(rto.VoxelGrid.from_array(g.data, g.min, g.voxel_size))
    assert rt.pathsTo([0], 4)[0] == hip.RTO_E_INVALID                    # no field made yet
    assert rt.geodesicField([0], 2)[0] == hip.RTO_E_INVALID and rt.geodesicField([nvox])[0] == hip.RTO_E_INVALID
    assert rt.geodesicField([])[0] == hip.RTO_E_INVALID and rt.floodFrom([0], 0, 6, -1) == hip.RTO_E_INVALID
    assert rt.floodFrom([-1]) == hip.RTO_E_INVALID
    assert np.array_equal(rt.grid(), g.data)
    # no resident grid, no octree
    ctx.upload_octree(scenes("sphere64").nodes, g.min, g.voxel_size)
    uploaded = ctx.render_host(frame)
    for call in (lambda: ctx.geodesic_field([0]), lambda: ctx.edit_geodesic([0])):
        with pytest.raises(hip.RtoError) as e:
            call()
        assert e.value.code == hip.RTO_E_UNSUPPORTED
    assert L.rto_geodesic_field(h, 2, 6, ok.ctypes.data, 2, NL, None) == hip.RTO_E_INVALID   # an unknown medium is reported before the missing grid
    assert_bit_exact(ctx.render_host(frame), uploaded, "the frame after the refusals (uploaded octree)")
    fresh = hip.Context(0)
    try:
        for call in (lambda: fresh.geodesic_field([0]), lambda: fresh.edit_geodesic([0])):
            with pytest.raises(hip.RtoError) as e:
                call()
            assert e.value.code == hip.RTO_E_NO_OCTREE
        assert fresh._L.rto_edit_geodesic(fresh._h, 7, 6, ok.ctypes.data, 2, NL, None) == hip.RTO_E_INVALID
    finally:
        fresh.close()


@gpu
def test_gpu_host_class_geodesic(scenes):
    import ray_tracing_octrees_amd as rto
    g = scenes("sphere64").grid
    data = np.ascontiguousarray(g.data, np.uint8)
    vg = rto.VoxelGrid.from_array(data, g.min, g.voxel_size)
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    rt.setOctreeFromGrid(rto.VoxelGrid.from_array(data, g.min, g.voxel_size))
    solid = int(np.flatnonzero(data.reshape(-1) == 1)[0])
    for seeds, m, conn, limit in (([0], gr.SET_EMPTY, gr.CONN_FACE, gr.NO_LIMIT), ([solid, 0], gr.SET_SOLID, gr.CONN_FULL, 90)):
        rc, f, sm = rt.geodesicField(seeds, m, conn, limit)
        wrc, want, wsm = vg.geodesicField(seeds, m, conn, limit)
        assert rc == wrc == 0 and np.array_equal(f, want) and sm.tobytes() == wsm.tobytes() and sm["reached"] > 1
        targets = [int(sm["argmax"]), 0, solid]
        rc, rows, lengths = rt.pathsTo(targets, 300)
        wr, wl = gr.paths(want, conn, targets, 300)
        assert rc == 0 and np.array_equal(rows, wr) and np.array_equal(lengths, wl)
    rc, far = rt.farthestPoint([0], gr.SET_EMPTY, gr.CONN_FACE)
    _, want, wsm = vg.geodesicField([0], gr.SET_EMPTY, gr.CONN_FACE)
    assert rc == 0 and far is not None
    (i, j, k), voxel, gmax, reached = far
    assert voxel == wsm["argmax"] == i + 64 * (j + 64 * k) and gmax == wsm["max_g"] and reached == wsm["reached"]
    assert rt.farthestPoint([solid], gr.SET_EMPTY, gr.CONN_FACE) == (0, None)
    want, changed = gr.flood(data, [solid], gr.SET_SOLID, gr.CONN_FULL, 30)
    assert rt.floodFrom([solid], gr.SET_SOLID, gr.CONN_FULL, 30) == changed > 0
    assert np.array_equal(rt.grid(), want)
    assert rt.floodFrom([solid], gr.SET_SOLID) == 0                     # that voxel is EMPTY now
    assert np.array_equal(rt.grid(), want)
