"""Part segmentation (rto_segment_parts, rto_download_part_labels / _parts / _necks, rto_parts_device, rto_edit_parts,
Context.segment_parts / edit_parts, RayTracerBVH::segmentParts / splitAtNecks, host/Parts.cpp).  CPU: the numpy rule
(tests/parts_ref.py) stated twice, against each other, against the host layer's plain loops, against the component rule at ratio 0
and, where scipy is present, against scipy.ndimage.label; the invariants of parts, necks and the cut; the ABI; the kernels' budgets.
GPU: labels, both tables, the summary and the number of basin edges downloaded, bit for bit against the rule, on grids chosen
around the 32 x 8 x 8 tile, the 16-byte path of the transform, a long ascent chain and a growing edge table; the edit against the
rule, a fresh build and the oracle's frame; state and errors."""
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
import parts_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("rto_segment_parts", "rto_download_part_labels", "rto_download_parts", "rto_download_necks", "rto_parts_device", "rto_edit_parts",
        "rto_last_parts_ms", "rto_debug_parts", "rto_debug_parts_capacity")
SETS = (pr.SET_SOLID, pr.SET_EMPTY)
CONNS = (pr.CONN_FACE, pr.CONN_FULL)
RATIOS = (0, 600, 800, 1000, 1001)
# VGPRs and LDS bytes the build gives, per instantiation: a kernel that grows past its line here has changed.
# ILb0E / ILb1E: the FACE / FULL form.  LDS: k_part_basin_min's block_reduce partials (4 waves x 12 bytes), k_part_cut's
# block_add_count partials.
PART_VGPR = {"k_part_ascendILb0E": 16, "k_part_ascendILb1E": 20, "k_part_flatten": 8, "k_part_basin_min": 23, "k_part_edgesILb0E": 19,
             "k_part_edgesILb1E": 22, "k_part_compact": 10, "k_part_relabel": 7, "k_part_cutILb0E": 18, "k_part_cutILb1E": 20}
PART_LDS = {"k_part_basin_min": 48, "k_part_cutILb0E": 16, "k_part_cutILb1E": 16}

def _hip():
    from ray_tracing_octrees_amd import hip
    return hip


# ================================================================ grids and their references (computed once, left unchanged)
def _bar():
    g = np.zeros((5, 5, 2102), np.uint8)
    g[1:4, 1:4, 1:2101] = 1
    return g


GRIDS = {
    "balls40": lambda: pr.two_balls(40, 24, 24),
    "balls48": lambda: pr.two_balls(48, 24, 24),
    "noise33": lambda: pr.opened_noise(33, 9, 10, 1),
    "noise37": lambda: pr.opened_noise(37, 22, 20, 2),
    "line_z": lambda: np.ones((70, 1, 1), np.uint8),
    "line_y": lambda: np.ones((1, 70, 1), np.uint8),
    "line_x": lambda: np.ones((1, 1, 70), np.uint8),
    "bar": _bar,
    "one_ball": lambda: pr.two_balls(24, 24, 24, 8, 0),
    "full": lambda: np.ones((9, 10, 33), np.uint8),
}
_GRID, _REF = {}, {}


def _grid(name):
    if name not in _GRID:
        _GRID[name] = GRIDS[name]()
        _GRID[name].setflags(write=False)
    return _GRID[name]


def _ref(name, s, conn, ratio):
    key = (name, s, conn, ratio)
    if key not in _REF:
        _REF[key] = pr.segment(_grid(name), s, conn, ratio)
    return _REF[key]


def _same(got, want, what):
    """got: (labels, parts, necks, summary); want: a parts_ref.Result."""
    labels, parts, necks, summary = got
    assert labels.shape == want.labels.shape and labels.dtype == np.int32, what
    assert np.array_equal(labels, want.labels), f"{what}: labels differ at {int((labels != want.labels).sum())} voxels"
    assert len(parts) == len(want.parts), f"{what}: {len(parts)} parts vs {len(want.parts)}"
    for f in pr.PART_DTYPE.names:
        assert np.array_equal(parts[f], want.parts[f]), f"{what}: part field {f}"
    assert len(necks) == len(want.necks), f"{what}: {len(necks)} necks vs {len(want.necks)}"
    for f in pr.NECK_DTYPE.names:
        assert np.array_equal(necks[f], want.necks[f]), f"{what}: neck field {f}"
    assert np.asarray(summary).tobytes() == want.summary.tobytes(), f"{what}: summary {summary} vs {want.summary}"


def _adjacent_pairs(labels, conn):
    """(a, b): the labels of every pair of adjacent voxels, both >= 0, each unordered pair once."""
    lab = labels.astype(np.int64)
    out = []
    for off in pr.offsets(conn):
        if (off[2], off[1], off[0]) < (0, 0, 0):
            continue
        nb = pr._shift(lab, off, np.int64(-1))
        m = (lab >= 0) & (nb >= 0)
        out.append(np.stack([lab[m], nb[m]], 1))
    return np.concatenate(out)


# ================================================================ CPU: the rule
NAMED = ["balls40", "balls48", "noise33", "noise37", "line_x", "line_y", "line_z", "bar", "one_ball", "full"]


@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("s", SETS)
@pytest.mark.parametrize("name", NAMED)
def test_the_two_statements_of_the_rule_agree(name, s, conn):
    """The per-voxel loop against the array form on every grid the GPU is checked on, both sets, both connectivities, every ratio.
    Rules 1 to 4 do not depend on the ratio, so the loop walks the voxels once per case and merges five times."""
    basins = pr.loops_basins(_grid(name), s, conn)
    for ratio in RATIOS:
        a, b = pr.loops(_grid(name), s, conn, ratio, basins), _ref(name, s, conn, ratio)
        what = f"{name} set {s} conn {conn} ratio {ratio}"
        _same((a.labels, a.parts, a.necks, a.summary), b, what)
        assert np.array_equal(a.basin_of, b.basin_of) and np.array_equal(a.edges, b.edges), what


@pytest.mark.parametrize("name", NAMED)
def test_host_cpu_form_equals_the_rule(name):
    import ray_tracing_octrees_amd as rto
    g = _grid(name)
    vg = rto.VoxelGrid.from_array(g, [0.0, 0.0, 0.0], 1.0)
    for s in SETS:
        for conn in CONNS:
            for ratio in RATIOS:
                _same(vg.segmentParts(s, conn, ratio), _ref(name, s, conn, ratio), f"{name} set {s} conn {conn} ratio {ratio}")


@pytest.mark.parametrize("name", ["balls40", "noise33", "noise37", "bar", "full"])
def test_ratio_0_is_the_component_labelling_and_ratio_1001_the_basins(name):
    g = _grid(name)
    for s in SETS:
        for conn in CONNS:
            labels, table = cr.label(g, s, conn)
            r0 = _ref(name, s, conn, 0)
            assert np.array_equal(r0.labels, labels), (name, s, conn)
            for f in ("root", "voxels", "lo", "hi", "touches"):
                assert np.array_equal(r0.parts[f], table[f]), (name, s, conn, f)
            assert len(r0.necks) == 0 and r0.summary["parts"] == len(table)
            r1 = _ref(name, s, conn, pr.RATIO_MAX)
            peaks = pr.peak_count(g, s, conn)
            assert r1.summary["parts"] == r1.summary["basins"] == peaks == len(r1.parts), (name, s, conn)
            # the same partition under two numberings: parts by their smallest voxel, basins by their peak
            both = np.unique(np.stack([r1.labels.reshape(-1), r1.basin_of.reshape(-1)], 1), axis=0)
            both = both[both[:, 0] >= 0]
            assert (r1.parts["basins"] == 1).all() and len(both) == peaks and len(np.unique(both[:, 1])) == peaks and (both[:, 1] >= 0).all()


def test_ratio_0_partition_equals_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for name in ("noise33", "noise37", "balls40"):
        for s in SETS:
            for conn in CONNS:
                want, n = ndi.label(_grid(name) == s, structure=ndi.generate_binary_structure(3, 1 if conn == pr.CONN_FACE else 3))
                l = _ref(name, s, conn, 0).labels
                pairs = np.unique(np.stack([l[l >= 0].astype(np.int64), want[l >= 0].astype(np.int64)], 1), axis=0)
                assert len(pairs) == n and len(np.unique(pairs[:, 0])) == n and len(np.unique(pairs[:, 1])) == n
                assert ((want == 0) == (l < 0)).all()


@pytest.mark.parametrize("name", ["balls40", "noise33", "noise37"])
def test_every_part_is_one_component_and_the_tables_describe_the_labels(name):
    g = _grid(name)
    dz, dy, dx = g.shape
    for s in SETS:
        for conn in CONNS:
            for ratio in RATIOS:
                r = _ref(name, s, conn, ratio)
                what = (name, s, conn, ratio)
                flat = r.labels.reshape(-1)
                assert ((flat >= 0) == (g.reshape(-1) == s)).all(), what
                # one component each: uniting the adjacent voxels of equal part number leaves one class per part
                idx = np.arange(g.size, dtype=np.int64).reshape(g.shape)
                ea, eb = [], []
                for off in pr.offsets(conn):
                    if (off[2], off[1], off[0]) < (0, 0, 0):
                        continue
                    nb, ni = pr._shift(r.labels, off, np.int32(-1)), pr._shift(idx, off, np.int64(-1))
                    m = (r.labels >= 0) & (nb == r.labels)
                    ea.append(idx[m]); eb.append(ni[m])
                parent = cr._union(g.size, np.concatenate(ea), np.concatenate(eb))
                classes = np.unique(parent[flat >= 0])
                assert len(classes) == len(r.parts), what
                # the part table
                assert np.array_equal(r.parts["voxels"], np.bincount(flat[flat >= 0], minlength=len(r.parts))), what
                assert np.array_equal(r.parts["root"], classes), what       # _union's root is the smallest member; ascending = the numbering
                assert r.parts["basins"].sum() == r.summary["basins"] and (r.parts["reserved"] == 0).all()
                h = r.heights.reshape(-1)
                for i, p in enumerate(r.parts):
                    mine = flat == i
                    assert flat[p["peak"]] == i and h[p["peak"]] == p["peak_h"] == h[mine].max(), what
                    assert p["peak"] == np.flatnonzero(mine & (h == p["peak_h"]))[0], what
                # the neck table: sorted, one per adjacent pair of parts, at is a voxel of S beside the other part at height h
                pairs = _adjacent_pairs(r.labels, conn)
                cross = pairs[pairs[:, 0] != pairs[:, 1]]
                keys = np.unique(np.sort(cross, 1), axis=0) if len(cross) else np.zeros((0, 2), np.int64)
                assert np.array_equal(np.stack([r.necks["part_lo"], r.necks["part_hi"]], 1).astype(np.int64).reshape(-1, 2), keys), what
                assert r.necks["pairs"].sum() == len(cross) == r.summary["pairs"], what
                for k in r.necks:
                    at = int(k["at"])
                    assert flat[at] in (k["part_lo"], k["part_hi"]), what
                    other = k["part_hi"] if flat[at] == k["part_lo"] else k["part_lo"]
                    x, y, z = at % dx, (at // dx) % dy, at // (dx * dy)
                    best = -1
                    for ox, oy, oz in pr.offsets(conn):
                        a, b, c = x + ox, y + oy, z + oz
                        if 0 <= a < dx and 0 <= b < dy and 0 <= c < dz and r.labels[c, b, a] == other:
                            best = max(best, min(int(h[at]), int(r.heights[c, b, a])))
                    assert best == k["h"], what


def test_two_balls_are_one_part_at_600_and_two_at_800():
    for name in ("balls40", "balls48"):
        r = _ref(name, pr.SET_SOLID, pr.CONN_FACE, 600)
        assert r.summary["parts"] == 1 and r.summary["basins"] == 2 and r.parts["voxels"][0] == 4126 and len(r.necks) == 0
        r = _ref(name, pr.SET_SOLID, pr.CONN_FACE, 800)
        assert r.summary["parts"] == 2 and list(r.parts["voxels"]) == [2063, 2063] and len(r.necks) == 1
        assert r.necks["h"][0] == 29 and r.necks["pairs"][0] == 89          # the lens between the balls: radius sqrt(29) voxels
    one = _ref("one_ball", pr.SET_SOLID, pr.CONN_FACE, pr.RATIO_MAX)
    assert one.summary["basins"] == 1 and one.summary["parts"] == 1


def test_full_grid_is_one_part_and_an_empty_set_gives_nothing():
    for conn in CONNS:
        for ratio in RATIOS:
            r = _ref("full", pr.SET_SOLID, conn, ratio)
            assert len(r.parts) == 1 and r.parts["peak_h"][0] == pr.NONE and r.parts["peak"][0] == 0 and r.parts["basins"][0] == 1
            assert (r.labels == 0).all() and len(r.necks) == 0
            e = _ref("full", pr.SET_EMPTY, conn, ratio)
            assert len(e.parts) == 0 and len(e.necks) == 0 and (e.labels == -1).all() and e.summary.tobytes() == bytes(32)


@pytest.mark.parametrize("name", ["balls40", "noise33", "noise37"])
def test_the_cut_separates_the_parts_on_the_host_layer_and_in_the_rule(name):
    import ray_tracing_octrees_amd as rto
    g = _grid(name)
    for s in SETS:
        for conn in CONNS:
            for ratio in (600, 800, 1001):
                r = _ref(name, s, conn, ratio)
                want, changed = pr.cut(g, s, conn, ratio, r.labels)
                vg = rto.VoxelGrid.from_array(g, [0.0, 0.0, 0.0], 1.0)
                assert vg.splitAtNecks(s, conn, ratio) == changed == int((want != g).sum()), (name, s, conn, ratio)
                assert np.array_equal(vg.data, want)
                assert (changed == 0) == (len(r.necks) == 0)
                # no two voxels of different former parts are adjacent any more
                kept = np.where(want == s, r.labels, -1)
                pairs = _adjacent_pairs(kept, conn)
                assert (pairs[:, 0] == pairs[:, 1]).all(), (name, s, conn, ratio)
                # Pieces against parts.  A part all of whose voxels touch a part of a larger number is flipped whole (rule 10 asks
                # for that), so "as many pieces as parts" can only be asked where every part keeps a voxel; what holds always is
                # that the parts that keep one are separated from each other.  The one case here where the count falls short:
                # noise33, EMPTY, FULL, ratio 1001: 49 parts, 46 keep a voxel, 47 pieces.
                survivors = len(np.unique(kept[kept >= 0]))
                pieces = len(cr.label(want, s, conn)[1])
                assert pieces >= survivors, (name, s, conn, ratio)


def test_host_cpu_form_refuses_what_the_call_refuses():
    import ray_tracing_octrees_amd as rto
    g = _grid("noise33")
    vg = rto.VoxelGrid.from_array(g, [0.0, 0.0, 0.0], 1.0)
    for s, conn, ratio in ((2, 6, 800), (1, 18, 800), (1, 6, -1), (1, 6, 1002)):
        with pytest.raises(ValueError):
            vg.segmentParts(s, conn, ratio)
        assert vg.splitAtNecks(s, conn, ratio) == -1
    assert np.array_equal(vg.data, g)


# ================================================================ CPU: the ABI and the build
def test_parts_abi_layout_and_exports():
    hip = _hip()
    assert hip.PART_DTYPE == pr.PART_DTYPE and hip.NECK_DTYPE == pr.NECK_DTYPE and hip.PARTS_SUMMARY_DTYPE == pr.SUMMARY_DTYPE
    assert [hip.PART_DTYPE.fields[f][1] for f in pr.PART_DTYPE.names] == [0, 8, 16, 28, 40, 44, 48, 56, 60]
    assert [hip.PART_DTYPE.fields[f][1] for f in ("root", "voxels", "lo", "hi", "touches")] == \
        [hip.COMPONENT_DTYPE.fields[f][1] for f in ("root", "voxels", "lo", "hi", "touches")]
    assert hip.PART_DTYPE.fields["basins"][1] == hip.COMPONENT_DTYPE.fields["reserved"][1]
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.fail("no C compiler: the header's layout cannot be checked")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "abi.c")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "rto_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu '
                    '%zu %zu %zu %d\\n", sizeof(rto_part), offsetof(rto_part, basins), offsetof(rto_part, peak), offsetof(rto_part, peak_h), '
                    'offsetof(rto_part, reserved), sizeof(rto_neck), offsetof(rto_neck, part_hi), offsetof(rto_neck, h), offsetof(rto_neck, at), '
                    'offsetof(rto_neck, pairs), sizeof(rto_parts_summary), offsetof(rto_parts_summary, basins), offsetof(rto_parts_summary, necks), '
                    'offsetof(rto_parts_summary, pairs), RTO_PARTS_RATIO_MAX); return 0; }\n')
        exe = os.path.join(tmp, "abi")
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert out == [str(v) for v in (64, 44, 48, 56, 60, 32, 4, 8, 16, 24, 32, 8, 16, 24, hip.PARTS_RATIO_MAX)]
    assert hip.PARTS_RATIO_MAX == pr.RATIO_MAX == 1001
    L = hip.load()
    header = open(os.path.join(ROOT, "include", "rto_hip.h")).read()
    for s in SYMS:
        assert s in hip.SYMBOLS and hasattr(L, s), s
        assert s + "(" in header, s


def test_part_kernels_keep_their_budgets():
    """The built assembly (the product's flags): every k_part_* kernel without scratch, spills or v_mfma, at the VGPR counts DESIGN.md
    section 26 states."""
    import test_isa_contract as isa
    asm = isa.built_asm()
    if asm is None:
        pytest.fail("no hipcc: the budget cannot be checked")
    meta = isa.kernel_meta(asm)
    md = asm[asm.index(".amdgpu_metadata"):]
    names = [k for k in meta if "k_part_" in k]
    assert len(names) == len(PART_VGPR) == 10, names      # ascend x2, edges x2, cut x2, four others
    seen = set()
    for k in names:
        m = meta[k]
        base = next(b for b in PART_VGPR if b in k)
        seen.add(base)
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (k, m)
        assert m["vgpr"] <= PART_VGPR[base], (k, m)
        lds = re.search(r"\.group_segment_fixed_size: (\d+)\n(?:(?!\.group_segment_fixed_size).)*?\.name:\s+" + re.escape(k) + r"\n", md, re.S)
        assert lds and int(lds.group(1)) == PART_LDS.get(base, 0), (k, lds and lds.group(1))
        ins = isa.body(asm, k[len("_ZN3rto"):])
        assert not any(t.startswith(("scratch_", "buffer_load", "buffer_store")) or "v_mfma" in t for t in ins), k
    assert seen == set(PART_VGPR)


# ================================================================ GPU
gpu = pytest.mark.gpu
GMIN, VOX = np.array([-0.5, -0.5, -0.5], np.float32), np.float32(1.0 / 64)


@pytest.fixture(scope="module")
def ctx2():
    """A second context: the fresh build of the edited grid that the edited context must equal."""
    c = _hip().Context(0)
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
    ctx.build_octree(np.ascontiguousarray(grid), GMIN, VOX)


def _gpu_result(ctx, s, conn, ratio):
    summary = ctx.segment_parts(s, conn, ratio)
    return ctx.part_labels(), ctx.parts(), ctx.necks(), summary


def _check_gpu(ctx, name, s, conn, ratio):
    want = _ref(name, s, conn, ratio)
    what = f"{name} set {s} conn {conn} ratio {ratio}"
    _same(_gpu_result(ctx, s, conn, ratio), want, what)
    basins, edges, rounds, cap = ctx.debug_parts()
    assert basins == want.summary["basins"], what
    assert edges == len(want.edges), f"{what}: {edges} basin edges came down, the rule has {len(want.edges)}"
    assert 1 <= rounds <= 32 and (cap == 0 if basins < 2 else cap >= max(edges, 1) and cap & (cap - 1) == 0), (what, rounds, cap)
    assert all(m >= 0 for m in ctx.last_parts_ms()), (what, ctx.last_parts_ms())
    return rounds, cap


@gpu
@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("s", SETS)
@pytest.mark.parametrize("name", ["balls40", "balls48", "noise33", "noise37", "line_x", "line_y", "line_z", "one_ball", "full"])
def test_gpu_parts_equal_the_rule(ctx, name, s, conn):
    _build(ctx, _grid(name))
    for ratio in RATIOS:
        _check_gpu(ctx, name, s, conn, ratio)
    # read again: the tables are resident
    want = _ref(name, s, conn, RATIOS[-1])
    _same((ctx.part_labels(), ctx.parts(), ctx.necks(), want.summary), want, f"{name} (read again)")


@gpu
def test_gpu_long_ridge_needs_more_than_one_flatten_round(ctx):
    """The 2,100 x 3 x 3 bar: its centre line is one flat ridge, every voxel of it steps to its -x neighbour, and the chain to the
    peak is about 2,100 long."""
    _build(ctx, _grid("bar"))
    for conn in CONNS:
        for ratio in (0, 800, 1001):
            rounds, _ = _check_gpu(ctx, "bar", pr.SET_SOLID, conn, ratio)
            assert 1 < rounds <= 32, rounds
    _check_gpu(ctx, "bar", pr.SET_EMPTY, pr.CONN_FACE, 800)


@gpu
@pytest.mark.parametrize("s,conn", [(pr.SET_EMPTY, pr.CONN_FACE), (pr.SET_SOLID, pr.CONN_FULL)])
def test_gpu_edge_table_grows_and_the_answer_stays(ctx, s, conn):
    _build(ctx, _grid("noise37"))
    ctx.debug_parts_capacity(16)
    try:
        _, cap = _check_gpu(ctx, "noise37", s, conn, pr.RATIO_MAX)
        edges = len(_ref("noise37", s, conn, pr.RATIO_MAX).edges)
        assert edges > 16 and cap > 16 and cap >= edges, (cap, edges)
        grown = cap
    finally:
        ctx.debug_parts_capacity(0)
    _, cap = _check_gpu(ctx, "noise37", s, conn, pr.RATIO_MAX)
    assert cap >= 1024 and grown >= 16                                      # the default table again: sized from the basin count


def _d2h(ptr, nbytes):
    L = _hip().load()
    out = np.zeros(nbytes, np.uint8)
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert L.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), nbytes, 2) == 0          # hipMemcpyDeviceToHost
    return out


@gpu
def test_gpu_parts_device_pointers(ctx):
    g = _grid("noise37")
    _build(ctx, g)
    want = _ref("noise37", pr.SET_EMPTY, pr.CONN_FACE, 800)
    ctx.segment_parts(pr.SET_EMPTY, pr.CONN_FACE, 800)
    d_labels, d_parts, n, d_necks, m = ctx.parts_device()
    assert d_labels and d_parts and d_necks and n == len(want.parts) > 0 and m == len(want.necks) > 0
    assert _d2h(d_labels, 4 * g.size).tobytes() == want.labels.tobytes()
    assert _d2h(d_parts, 64 * n).tobytes() == want.parts.tobytes()
    assert _d2h(d_necks, 32 * m).tobytes() == want.necks.tobytes()


@gpu
@pytest.mark.parametrize("name,s,conn,ratio", [("balls40", pr.SET_SOLID, pr.CONN_FACE, 800), ("noise37", pr.SET_SOLID, pr.CONN_FULL, 800),
                                               ("noise37", pr.SET_EMPTY, pr.CONN_FACE, 1001)])
def test_gpu_edit_parts_equals_the_rule_and_a_fresh_build(ctx, ctx2, orc, name, s, conn, ratio, path):
    """The cut: the grid and changed are the rule's, the context equals a fresh build of that grid (nodes == the oracle's, info,
    scene bounds), the frame is the oracle's, and the parts are now pieces."""
    import test_components as tc
    from conftest import make_camera
    g = np.array(_grid(name))
    _build(ctx, g)
    r = _ref(name, s, conn, ratio)
    want, changed = pr.cut(g, s, conn, ratio, r.labels)
    assert changed > 0
    what = f"{name} {path} set {s} conn {conn} ratio {ratio}"
    assert ctx.edit_parts(s, conn, ratio) == changed, what
    og, nodes = tc._check_rebuilt(ctx, ctx2, orc, GMIN, VOX, want, what)
    tc._check_render(ctx, orc, og, nodes, *make_camera(orc, 0.5, 0.7, 1.8), what)
    assert ctx.info().culling_active == 0
    assert len(ctx.label_components(s, conn)) >= len(r.parts)
    # cut again: the pieces may split further, but the answer is the rule's again
    want2, changed2 = pr.cut(want, s, conn, ratio)
    assert ctx.edit_parts(s, conn, ratio) == changed2
    assert np.array_equal(ctx.download_voxels(), want2)


@gpu
def test_gpu_edit_parts_rebuilds_resident_triangles(ctx, ctx2, orc, path):
    import test_components as tc
    g = np.array(_grid("balls40"))
    _build(ctx, g)
    ctx.build_leaf_triangles(None)
    want, changed = pr.cut(g, pr.SET_SOLID, pr.CONN_FACE, 800)
    assert ctx.edit_parts(pr.SET_SOLID, pr.CONN_FACE, 800) == changed > 0
    og, nodes = tc._check_rebuilt(ctx, ctx2, orc, GMIN, VOX, want, f"balls40 triangles {path}")
    ctx2.build_leaf_triangles(None)
    t1, o1 = ctx.download_leaf_triangles()
    t2, o2 = ctx2.download_leaf_triangles()
    assert t1.tobytes() == t2.tobytes() and o1.tobytes() == o2.tobytes()


def _readers(ctx):
    return {"part_labels": ctx.part_labels, "parts": ctx.parts, "necks": ctx.necks, "parts_device": ctx.parts_device}


def _all_gone(ctx):
    hip = _hip()
    for name, read in _readers(ctx).items():
        with pytest.raises(hip.RtoError) as e:
            read()
        assert e.value.code == hip.RTO_E_INVALID and "the grid has changed since" in str(e.value), (name, str(e.value))


def _snapshot(ctx):
    return ctx.part_labels().tobytes(), ctx.parts().tobytes(), ctx.necks().tobytes(), ctx.parts_device()


@gpu
def test_gpu_parts_lifecycle(ctx):
    """The results describe one state of the grid: every call that changes or replaces it drops them, a call that changes nothing
    keeps them, and the component labels and the other fields live beside them."""
    hip = _hip()
    g = np.array(_grid("balls40"))
    _build(ctx, g)
    _all_gone(ctx)                                                         # nothing made yet
    ctx.segment_parts(pr.SET_SOLID, pr.CONN_FACE, 800)
    before = _snapshot(ctx)
    # calls that change nothing: a cut with nothing to cut, a component edit that selects nothing, other products
    assert ctx.edit_parts(pr.SET_SOLID, pr.CONN_FACE, 600) == 0
    assert ctx.edit_components(hip.SET_SOLID, hip.CONN_FACE, hip.SELECT_SMALLER_THAN, 1) == 0
    ctx.label_components(hip.SET_SOLID, hip.CONN_FACE)
    ctx.distance_field(hip.SET_SOLID)
    assert _snapshot(ctx) == before
    assert len(ctx.components()) == 1 and ctx.distance().shape == g.shape
    # a second segmentation replaces the first
    ctx.segment_parts(pr.SET_SOLID, pr.CONN_FACE, 600)
    assert len(ctx.parts()) == 1 and len(ctx.necks()) == 0
    ctx.segment_parts(pr.SET_SOLID, pr.CONN_FACE, 800)
    assert _snapshot(ctx)[:3] == before[:3]
    # calls that change the grid
    assert ctx.edit_parts(pr.SET_SOLID, pr.CONN_FACE, 800) > 0
    _all_gone(ctx)
    ctx.segment_parts(pr.SET_SOLID, pr.CONN_FACE, 800)
    assert len(ctx.necks()) == 0 and len(ctx.parts()) == 2                 # the parts are pieces now
    centre = (GMIN.astype(np.float64) + np.array([10.0, 12.0, 12.0]) * float(VOX)).astype(np.float32)
    assert ctx.edit_voxels(hip.make_brushes([centre], [np.full(3, 2 * float(VOX), np.float32)], hip.BRUSH_BOX, hip.EDIT_CARVE)) > 0
    _all_gone(ctx)
    ctx.segment_parts(pr.SET_SOLID, pr.CONN_FACE, 800)
    _build(ctx, g)                                                         # a rebuild
    _all_gone(ctx)
    ctx.segment_parts(pr.SET_SOLID, pr.CONN_FACE, 800)
    assert _snapshot(ctx)[:3] == before[:3]


@gpu
@pytest.mark.parametrize("k", [1, 2, 3])
def test_gpu_a_failed_allocation_keeps_the_old_result(ctx, k):
    """rto_debug_fault_alloc(k): the allocation of the new label volume (1), part table (2) or neck table (3) fails (a simulated
    host-side failure; nothing faults on the device).  The call answers RTO_E_HIP, the old result reads back byte for byte under
    the same pointers, and the same call succeeds once the hook is disarmed."""
    hip = _hip()
    L = hip.load()
    _build(ctx, _grid("balls40"))
    ctx.segment_parts(pr.SET_SOLID, pr.CONN_FACE, 800)
    before = _snapshot(ctx)
    try:
        assert L.rto_debug_fault_alloc(k) == 0
        with pytest.raises(hip.RtoError) as e:
            ctx.segment_parts(pr.SET_SOLID, pr.CONN_FACE, 1001)
    finally:
        assert L.rto_debug_fault_alloc(0) == 0
    assert e.value.code == hip.RTO_E_HIP, str(e.value)
    assert _snapshot(ctx) == before
    _check_gpu(ctx, "balls40", pr.SET_SOLID, pr.CONN_FACE, 1001)


@gpu
def test_gpu_parts_refusals_leave_the_context_untouched(ctx):
    hip = _hip()
    g = _grid("noise33")
    _build(ctx, g)
    ctx.segment_parts(pr.SET_EMPTY, pr.CONN_FULL, 800)
    before = _snapshot(ctx)
    nodes = ctx.download_nodes().tobytes()
    for call in (ctx.segment_parts, ctx.edit_parts):
        for s, conn, ratio in ((2, 6, 800), (-1, 6, 800), (1, 18, 800), (1, 0, 800), (1, 6, -1), (1, 6, 1002)):
            with pytest.raises(hip.RtoError) as e:
                call(s, conn, ratio)
            assert e.value.code == hip.RTO_E_INVALID, (s, conn, ratio)
    L = hip.load()
    n = C.c_int64()
    small = np.zeros(1, pr.PART_DTYPE)
    assert L.rto_download_parts(ctx._h, small.ctypes.data, 0, C.byref(n)) == hip.RTO_E_INVALID and n.value == len(_ref("noise33", 0, 26, 800).parts)
    assert L.rto_download_necks(ctx._h, small.ctypes.data, 0, C.byref(n)) == hip.RTO_E_INVALID
    assert L.rto_download_part_labels(ctx._h, small.ctypes.data, g.size - 1) == hip.RTO_E_INVALID
    with pytest.raises(hip.RtoError):
        ctx.debug_parts_capacity(-1)
    assert _snapshot(ctx) == before and ctx.download_nodes().tobytes() == nodes and np.array_equal(ctx.download_voxels(), g)
    # no resident grid: an uploaded octree
    up = hip.Context(0)
    try:
        with pytest.raises(hip.RtoError) as e:
            up.segment_parts()
        assert e.value.code == hip.RTO_E_NO_OCTREE
        up.upload_octree(ctx.download_nodes(), GMIN, VOX)
        for call in (up.segment_parts, up.edit_parts):
            with pytest.raises(hip.RtoError) as e:
                call()
            assert e.value.code == hip.RTO_E_UNSUPPORTED
    finally:
        up.close()


@gpu
def test_gpu_host_class_segments_and_splits(ctx):
    import ray_tracing_octrees_amd as rto
    hip = _hip()
    g = np.array(_grid("balls40"))
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    rt.setOctreeFromGrid(rto.VoxelGrid.from_array(g, GMIN, VOX))
    assert rt.parts()[0] == hip.RTO_E_INVALID and rt.partLabels()[0] == hip.RTO_E_INVALID
    want = _ref("balls40", pr.SET_SOLID, pr.CONN_FACE, 800)
    rc, labels, summary = rt.segmentParts(pr.SET_SOLID, pr.CONN_FACE, 800)
    assert rc == 0
    _same((labels, rt.parts()[1], rt.necks()[1], summary), want, "RayTracerBVH")
    assert np.array_equal(rt.partLabels()[1], want.labels)
    assert rt.segmentParts(pr.SET_SOLID, pr.CONN_FACE, 1002)[0] == hip.RTO_E_INVALID
    cut, changed = pr.cut(g, pr.SET_SOLID, pr.CONN_FACE, 800, want.labels)
    assert rt.splitAtNecks(pr.SET_SOLID, pr.CONN_FACE, 800) == changed and np.array_equal(rt.grid(), cut)
    assert rt.parts()[0] == hip.RTO_E_INVALID
    assert rt.splitAtNecks(pr.SET_SOLID, pr.CONN_FACE, 800) == 0
    t = rt.labelComponents(pr.SET_SOLID, pr.CONN_FACE)
    assert t is not None and len(t) == 2
