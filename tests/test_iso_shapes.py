"""The isosurface kernels at their tile, run and box edges ("Checks"; tests/iso_shapes.py is the launch
geometry as code and holds the inputs).  CPU: the calls below take every row of the table, the model agrees with iso_ref, the host
form equals iso_ref on every call, and a box that starts in a later tile cannot be told from the same box one tile earlier only
where the lists really differ.  GPU: every call bit for bit against iso_ref, with the brick table on and off."""
from __future__ import annotations

import os
import re
from collections import Counter

import numpy as np
import pytest

import distance_ref as dr
import iso_ref as ir
import iso_shapes as sh
from ray_tracing_octrees_amd import hip
from test_isosurface import _from18, _same_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AT_LEAST = 4                  # calls with a triangle that must take a row; a row that falls short wants other inputs, not another figure
BUFFER_CALLS = 40             # the calls a fresh context makes in test_gpu_the_output_buffer_grows_and_is_kept
NO_TRIANGLE = {"iso:box-without-a-cell", "iso_emit:no-triangle"}
GROUPS = {"shelf-pad": lambda: sh.shelf_calls(True), "shelf-nopad": lambda: sh.shelf_calls(False), "window": sh.window_calls,
          "row": sh.row_calls, "even": sh.even_calls}

# clip boxes of the shelf for the resident distance field: t0 >= 1 along x, along y, along z, along all three
RESIDENT_BOXES = [((32, 0, 0), (100, 28, 27)), ((65, 0, 0), (96, 28, 27)), ((95, 0, 0), (100, 28, 27)),
                  ((0, 8, 0), (100, 16, 27)), ((0, 9, 0), (100, 17, 27)), ((0, 16, 0), (100, 28, 27)),
                  ((0, 0, 8), (100, 28, 16)), ((0, 0, 9), (100, 28, 15)), ((0, 0, 17), (100, 28, 27)),
                  ((33, 9, 9), (65, 17, 15)), ((64, 16, 17), (100, 28, 27)), ((31, 15, 7), (63, 24, 27))]


def _params(call, source=hip.FIELD_CALLER):
    return hip.make_iso_params(source, call.level, call.outside, call.valid, bool(call.pad), call.clip)


def _what(call, *more):
    return " ".join(str(w) for w in (call.grid, "pad" if call.pad else "nopad", call.clip, call.valid, *more))


def _later(call):
    g = sh.call_geometry(call)
    return g is not None and max(g["t0"]) >= 1


def _buffer_sequence():
    return sh.ordered(sh.shelf_calls(True))[:BUFFER_CALLS]


# ---------------------------------------------------------------- without a GPU
def test_every_row_is_taken_by_calls_that_hold_a_triangle():
    taken, any_list, unknown = Counter(), Counter(), set()
    pinned = Counter()                    # the three shapes at a box edge, in calls whose box begins past the first tile
    for call in sh.all_calls():
        rows = sh.call_classes(call)
        unknown |= rows - set(sh.TABLE)
        unknown |= sh.call_classes(call, table=False) - set(sh.TABLE)
        any_list.update(rows)
        if len(sh.ref(call)[1]):
            taken.update(rows)
            if _later(call):
                pinned.update(rows & {"iso_count:crossed-by-outside-alone", "iso_count:staged-without-a-triangle",
                                      "iso_count:skipped:rows-outside-the-cell-box"})
    cap = 0                               # the iso_out rows: by the order of the calls, from a context without a buffer
    for call in _buffer_sequence():
        if sh.call_geometry(call) is None:
            continue
        row, cap = sh.buffer_class(cap, len(sh.ref(call)[1]))
        any_list[row] += 1
        taken[row] += 1 if len(sh.ref(call)[1]) else 0
    assert not unknown, unknown
    short = {}
    for row in sh.TABLE:
        if row == "iso_scan:rounds>=2":   # 2,097,153 runs: one call of test_isosurface.py, checked below
            continue
        n = any_list[row] if row in NO_TRIANGLE else taken[row]
        if n < (1 if row in NO_TRIANGLE else AT_LEAST):
            short[row] = n
    assert not short, short
    assert len(pinned) == 3 and min(pinned.values()) >= AT_LEAST, pinned


def test_the_brick_table_off_stages_every_tile():
    for call in sh.window_calls()[:6]:
        rows = sh.call_classes(call, table=False)
        assert not any(r.startswith(("iso_bricks:", "iso_count:tile-skipped", "iso_count:skipped")) for r in rows), rows
        assert "iso_count:tile-staged" in rows


def test_the_scan_of_more_than_1024_block_sums_is_the_test_the_table_names():
    assert sh.SCAN_TEST in sh.TABLE["iso_scan:rounds>=2"][1]
    text = open(os.path.join(ROOT, "tests", "test_isosurface.py")).read()
    body = text[text.index(f"def {sh.SCAN_TEST}(ctx)"):]
    assert re.search(r"N = 2901\b", body) and "np.full((N, N, 2)" in body and "pad=False" in body
    rows = sh.launch_classes((2, 2901, 2901), False, None)
    assert "iso_scan:rounds>=2" in rows and sh.geometry((2, 2901, 2901), False, None)["runs"] == 2900 * 2900


def test_the_design_names_every_row():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("## 24. Launch shapes of the grid kernels"):text.index("## 25. ")]
    for row in [*sh.TABLE, *sh.BY_INSPECTION]:
        assert f"`{row}`" in section, row


def test_geometry_agrees_with_iso_ref_on_the_cells():
    for call in sh.all_calls():
        S, first = ir.samples(sh.grid(call.grid), call.level, call.outside, call.valid, call.pad, call.clip)
        g = sh.call_geometry(call)
        if g is None:
            assert min(S.shape) < 2 and len(sh.ref(call)[1]) == 0, _what(call)
            continue
        assert g["cells"] == tuple(n - 1 for n in S.shape[::-1]), _what(call)
        assert g["uLo"] == tuple(int(f) + 1 for f in first), _what(call)
        assert all(g["t0"][a] * sh.TILE[a] <= g["uLo"][a] < (g["t0"][a] + 1) * sh.TILE[a] for a in range(3))
        assert all((g["t0"][a] + g["tiles"][a] - 1) * sh.TILE[a] < g["uHi"][a] <= (g["t0"][a] + g["tiles"][a]) * sh.TILE[a] for a in range(3))


def test_the_tiles_hold_the_reference_s_triangles_and_skip_none():
    """tiles_of asserts that a skipped tile holds no triangle; here the tiles' counts add up to the list, on one call of each kind."""
    for call in (sh.shelf_calls(True)[0], sh.shelf_calls(False)[200], sh.window_calls()[7], sh.row_calls()[1], sh.even_calls()[3]):
        tiles = sh.tiles_of(sh.grid(call.grid), call.level, call.outside, call.valid, call.pad, call.clip, sh.ref(call))
        g = sh.call_geometry(call)
        assert len(tiles) == g["tiles"][0] * g["tiles"][1] * g["tiles"][2]
        assert sum(t.triangles for t in tiles) == len(sh.ref(call)[1]) > 0, _what(call)


def test_the_tiles_write_every_run_once_and_only_with_the_first_tile_and_the_guard():
    """k_iso_count's workgroups, by the model: every run of the cell box gets its count exactly once.  With u0y taken from tile 0
    where t0[1] >= 1, rows stay unwritten (and the scans would read what the scratch held); without the uLo / uHi test a
    tile writes outside the run array or onto another row's count.  Neither form was run on a GPU for that reason."""
    seen = Counter()
    for call in sh.all_calls():
        g = sh.call_geometry(call)
        if g is None or call.grid != "shelf" or call.valid != sh.VALID:
            continue
        hits, stray = sh.rows_written(g)
        assert stray == 0 and (hits == 1).all(), _what(call)
        if g["t0"][1] >= 1:
            hits, stray = sh.rows_written(g, t0=(g["t0"][0], 0, g["t0"][2]))
            assert (hits == 0).any(), _what(call)
            seen["t0y"] += 1
        if g["uLo"][1] % 8 or g["uHi"][1] % 8 or g["uLo"][2] % 8 or g["uHi"][2] % 8:
            hits, stray = sh.rows_written(g, guard=False)
            assert stray > 0 or (hits > 1).any(), _what(call)
            seen["guard"] += 1
    assert min(seen["t0y"], seen["guard"]) >= 100, seen


@pytest.mark.parametrize("group", list(GROUPS))
def test_the_host_form_equals_iso_ref_on_every_call(group):
    from ray_tracing_octrees_amd import host
    for call in GROUPS[group]():
        t18, cell, summary = host.isoSurfaceVolume(sh.grid(call.grid), sh.GMIN, sh.VS, _params(call))
        _same_list((_from18(t18), cell, summary), sh.ref(call), _what(call))


def _shifted(call, axis):
    """The same-sized box one tile earlier along `axis`, None where it leaves the grid."""
    lo, hi = list(call.clip[0]), list(call.clip[1])
    lo[axis] -= sh.TILE[axis]
    hi[axis] -= sh.TILE[axis]
    return None if lo[axis] < 0 else call._replace(clip=(tuple(lo), tuple(hi)))


def test_a_box_in_a_later_tile_differs_from_the_same_box_one_tile_earlier():
    """A kernel that ignored t0 and added the shift to tri_cell afterwards would give the list of the box one tile earlier, moved.
    Every box of the shelf that starts in a later tile and holds 32 voxels of noise or more (two such boxes agree on which lie
    below the level with probability 2^-32) has another triangle count, or other cells once the shift is taken out; boxes
    inside the uniform 7 do not, and are not counted."""
    vol = sh.grid("shelf")
    dims = vol.shape[::-1]
    stride = (1, dims[0] + 1, (dims[0] + 1) * (dims[1] + 1))
    noise = np.zeros(vol.shape, bool)
    noise[:, :, 40:] = True
    noise[9:27, 9:28, 66:100] = False
    told, held = Counter(), Counter()
    for call in [*sh.shelf_calls(True), *sh.shelf_calls(False)]:
        g = sh.call_geometry(call)
        if g is None or call.clip is None or len(sh.ref(call)[1]) == 0:
            continue
        (x0, y0, z0), (x1, y1, z1) = call.clip
        for a in range(3):
            other = _shifted(call, a) if g["t0"][a] >= 1 else None
            if other is None:
                continue
            cell, ocell = sh.ref(call)[1], sh.cell_list(other)
            assert np.array_equal(sh.cell_list(call), cell)
            differs = len(cell) != len(ocell) or not np.array_equal(cell, ocell + sh.TILE[a] * stride[a])
            if noise[z0:z1, y0:y1, x0:x1].sum() >= 32:
                assert differs, _what(call, "axis", a)
                held[(a, bool(call.pad))] += 1
            told[(a, bool(call.pad))] += differs
    assert len(held) == 6 and min(held.values()) >= 20, held
    assert all(told[k] >= held[k] for k in held), (told, held)


# ---------------------------------------------------------------- on the GPU
def _resident(ctx, name):
    """A resident grid of the volume's dims (its voxels do not enter a CALLER extraction)."""
    grid = (sh.grid(name) & 1).astype(np.uint8)
    ctx.build_octree(grid, sh.GMIN, sh.VS)
    return grid


def _run(ctx, call, volume, more=""):
    want = sh.ref(call)
    _same_list(ctx.extract_isosurface(_params(call), volume), want, _what(call, more))
    ms = tuple(ctx.last_isosurface_ms())
    if sh.call_geometry(call) is None:                # no cell: no kernel, and nothing to download
        assert ms == (-1.0, -1.0, -1.0), _what(call, ms)
        assert len(ctx.download_isosurface()[0]) == 0 and ctx.isosurface_device()[2] == 0
    else:
        assert len(ms) == 3 and all(m >= 0 for m in ms), _what(call, ms)


@pytest.mark.gpu
@pytest.mark.parametrize("table", [True, False], ids=["table", "notable"])
@pytest.mark.parametrize("pad", [True, False], ids=["pad", "nopad"])
def test_gpu_the_shelf_under_every_box(ctx, pad, table):
    import torch
    _resident(ctx, "shelf")
    d_vol = torch.from_numpy(np.array(sh.grid("shelf"))).cuda()                   # a writable copy
    calls = sh.ordered(sh.shelf_calls(pad))
    assert len(calls) == 505
    try:
        ctx.debug_set_projection_table(table)
        for call in calls:
            _run(ctx, call, d_vol, f"table {table}")
    finally:
        ctx.debug_set_projection_table(True)


@pytest.mark.gpu
@pytest.mark.parametrize("table", [True, False], ids=["table", "notable"])
def test_gpu_the_window_the_row_and_the_even_grids(ctx, table):
    import torch
    try:
        ctx.debug_set_projection_table(table)
        for calls in (sh.window_calls(), sh.row_calls(), sh.even_calls()):
            for name in dict.fromkeys(c.grid for c in calls):
                _resident(ctx, name)
                d_vol = torch.from_numpy(np.array(sh.grid(name))).cuda()
                for call in sh.ordered([c for c in calls if c.grid == name]):
                    _run(ctx, call, d_vol, f"table {table}")
    finally:
        ctx.debug_set_projection_table(True)


@pytest.mark.gpu
def test_gpu_the_host_volume_entry_point_in_later_tiles(ctx):
    """rto_extract_isosurface_host uploads the volume itself, on the call's stream."""
    _resident(ctx, "shelf")
    later = [c for c in [*sh.shelf_calls(True), *sh.shelf_calls(False)] if _later(c) and len(sh.ref(c)[1])]
    picked = later[::len(later) // 20]
    assert len(picked) >= 20 and all(any(sh.call_geometry(c)["t0"][a] >= 1 for c in picked) for a in range(3))
    for call in picked:
        _run(ctx, call, sh.grid("shelf"), "host volume")


@pytest.mark.gpu
@pytest.mark.parametrize("table", [True, False], ids=["table", "notable"])
def test_gpu_the_resident_distance_field_in_later_tiles(ctx, table):
    grid = _resident(ctx, "shelf")
    d2 = ctx.distance_field(hip.SET_EMPTY)[0]
    assert np.array_equal(d2, dr.field(grid, dr.SET_EMPTY))
    assert all(any(sh.geometry((100, 28, 27), True, box)["t0"][a] >= 1 for box in RESIDENT_BOXES) for a in range(3))
    try:
        ctx.debug_set_projection_table(table)
        for box in RESIDENT_BOXES:
            for pad in (True, False):
                want = ir.extract(d2, sh.GMIN, sh.VS, 0.5, 0.0, pad=pad, clip=box)
                assert len(want[0]) > 0, box
                got = ctx.extract_isosurface(hip.make_iso_params(hip.FIELD_DISTANCE, 0.5, 0.0, pad=pad, clip=box))
                _same_list(got, want, f"distance field {box} pad {pad} table {table}")
    finally:
        ctx.debug_set_projection_table(True)


@pytest.mark.gpu
def test_gpu_the_output_buffer_grows_and_is_kept():
    """A context of its own, so that the buffer's capacity is the model's: the device pointers change exactly where
    iso_shapes.buffer_class says the buffer grows, and every list is right in a buffer made for a longer one."""
    import ray_tracing_octrees_amd as rto
    ctx = rto.Context(0)
    try:
        _resident(ctx, "shelf")
        vol = sh.grid("shelf")
        cap, before, rows = 0, None, Counter()
        for call in _buffer_sequence():
            _run(ctx, call, vol, "own context")
            if sh.call_geometry(call) is None:
                continue
            row, cap = sh.buffer_class(cap, len(sh.ref(call)[1]))
            now = ctx.isosurface_device()[:2]
            assert (now != before) == (row == "iso_out:buffer-grows"), _what(call, row, before, now)
            before = now
            rows[row] += 1
        assert min(rows["iso_out:buffer-grows"], rows["iso_out:buffer-kept"]) >= AT_LEAST, rows
    finally:
        ctx.close()
