"""Dose fields (rto_dose_field): the two statements of the crossing rule in tests/dose_ref.py against each other
(the open-cube definition from both ends, and the template's periods), against the closed forms, against the host layer's CPU form
(host/Dose.cpp) and, on the GPU, against the library bit for bit: field, coverage table, summary and the device pointer's copy."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import dose_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("rto_dose_field", "rto_download_dose", "rto_dose_device", "rto_download_dose_coverage", "rto_last_dose_ms")
MODES = (dr.DOSE_ALL, dr.DOSE_SKIN)
FALLOFFS = (dr.FALLOFF_NONE, dr.FALLOFF_INVERSE_SQUARE)
REACHES = (1, 3, None)
SIGHT, HALVING, GAP = [65536], [65536, 32768, 16384], [65536, 0, 65536]
TABLES = (SIGHT, HALVING, GAP)
# VGPRs and LDS bytes the build gives; a kernel that grows past its line here has changed
DOSE_VGPR = {"k_dose_march": 28, "k_dose_summary": 21}
DOSE_LDS = {"k_dose_march": 256, "k_dose_summary": 96}


def _hip():
    from ray_tracing_octrees_amd import hip
    return hip


def _tc():
    import test_components as tc          # its checks of a context
    return tc


# ================================================================ grids and sources
def _seeded(x, y, z, fill):
    return (np.random.default_rng(1000 + x + fill).random((z, y, x)) < fill / 100).astype(np.uint8)


TILE_SIZED = ((31, 7, 7), (32, 8, 8), (33, 9, 9), (65, 17, 17))
SEEDED = {f"s{x}x{y}x{z}_{fill}": (x, y, z, fill) for (x, y, z) in (*TILE_SIZED, (5, 3, 2), (40, 1, 1)) for fill in (3, 10)}
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


def _cap_sources(g):
    """The four source voxels of the coverage cap: two opposite corners, the centre and the middle of an edge."""
    z, y, x = g.shape
    return [(0, 0, 0), (x - 1, y - 1, z - 1), (x // 2, y // 2, z // 2), (x - 1, 0, z // 2)]


def _weighted(positions):
    """Weights 1 + 1000 (index % 7), with one zero among them."""
    return [(*p, 0 if i == 3 else 1 + 1000 * (i % 7)) for i, p in enumerate(positions)]


def _sources(name, g):
    """The cap's four, the first SOLID voxel (a lamp on a wall), the centre again (a source given twice counts twice); for a wall,
    sources on both sides of it and one in the hole's place."""
    pos = _cap_sources(g)
    solid = np.argwhere(g == 1)
    if len(solid):
        pos.append(tuple(int(c) for c in solid[0][::-1]))
    pos.append(pos[2])
    if name in WALLS:
        axis, at, _ = WALLS[name]
        for off in (-1, 0, 1, 2):
            p = [30, 8, 8]
            p[axis] = at + off
            pos.append(tuple(p))
    return _weighted(pos)


_WALLS_OF = {}
_REF = {}


def _ref(name, g, sources, transmit, falloff, mode, reach, counts=None):
    """The rule's field, coverage and summary, made once per case and left unchanged; k(p, s) of a (grid, mode, reach, source voxel)
    is shared by every case that needs it."""
    r = dr.NO_LIMIT if reach is None else reach

    def walls(grid, P, s):
        key = (name, mode, min(r, dr.MAX_REACH), tuple(s))
        if key not in _WALLS_OF:
            _WALLS_OF[key] = dr.walls(grid, P, s)
            _WALLS_OF[key].setflags(write=False)
        assert len(_WALLS_OF[key]) == len(P)
        return _WALLS_OF[key]

    key = (name, tuple(tuple(int(c) for c in s) for s in sources), None if transmit is None else tuple(transmit), falloff, mode, r)
    if key not in _REF or counts is not None:
        e, cov, s = dr.dose(g, sources, transmit, falloff, mode, r, walls, counts)
        e.setflags(write=False)
        cov.setflags(write=False)
        _REF[key] = (e, cov, s)
    return _REF[key]


def _cases(name):
    """(transmit, falloff, mode, reach) of a named grid: both modes and falloffs, reach 1, 3 and none, the three short tables."""
    if name in SEEDED:
        return [(t, f, m, r) for m in MODES for f in FALLOFFS for r in REACHES for t in TABLES]
    return [(HALVING, f, m, r) for m in MODES for r in REACHES for f in (FALLOFFS if r is None else FALLOFFS[:1])]


# ---- the special grids of the GPU tests, which the host form is pinned on as well
def _row(x):
    return np.zeros((1, 1, x), np.uint8)


def _row_sources(x):
    return _weighted([(0, 0, 0), (x - 1, 0, 0), (x // 2, 0, 0)])


LONG_TABLE = [65536 - 1000 * k for k in range(64)]                      # 64 entries, the last one 2,536: not zero


def _run130(run):
    """130 x 1 x 1 with `run` SOLID voxels from x = 1 on, between p = 0 and the source at x = 129."""
    g = _row(130)
    g[0, 0, 1:1 + run] = 1
    return g


def _floor128():
    g = np.zeros((66, 128, 128), np.uint8)
    g[0] = 1
    g[40, 64, 64] = 1
    return g


FLOOR_SOURCE = [(64, 64, 38, 777)]


def _edge1024():
    """1,024 x 1,024 x 2, EMPTY but for 16 isolated SOLID voxels, three of them beside far corners: under SKIN the list is their
    face neighbours, among them the corners (1023, 1023, 1) and (0, 0, 1) and the voxel (1023, 1022, 0)."""
    g = np.zeros((2, 1024, 1024), np.uint8)
    rng = np.random.default_rng(1024)
    for i in range(13):                                                  # on a lattice of 4: no two are neighbours
        g[i % 2, 4 * int(rng.integers(2, 250)), 4 * int(rng.integers(2, 250))] = 1
    g[1, 1023, 1022] = 1                                                 # beside (1023, 1023, 1)
    g[0, 1021, 1023] = 1                                                 # beside (1023, 1022, 0)
    g[1, 0, 1] = 1                                                       # beside (0, 0, 1)
    assert int(g.sum()) == 16
    return g


EDGE_SOURCES = [(0, 0, 0, 2 ** 30), (1023, 0, 0, 2 ** 29), (0, 1023, 0, 2 ** 28), (1023, 1023, 0, 2 ** 27), (0, 0, 1, 12345)]


def _count_sources(g, n):
    """n sources that cycle over 67 voxels spread over the grid, SOLID ones among them."""
    z, y, x = g.shape
    out = []
    for i in range(n):
        v = (i % 67) * 39
        out.append((v % x, v // x % y, v // x // y, 1 + 1000 * (i % 7)))
    assert any(g[s[2], s[1], s[0]] == 1 for s in out[:67]) or n < 67
    return out


# ================================================================ CPU: the rule
@pytest.mark.parametrize("dims", [(7, 5, 4), (5, 3, 2)])
def test_the_definition_equals_the_template_periods(dims):
    """(a) == (b) == the vectorised walk for every EMPTY voxel against every voxel of the grid as the source; and voxel by voxel,
    not only as a count, for the sources at the corners."""
    x, y, z = dims
    g = (np.random.default_rng(x).random((z, y, x)) < 0.3).astype(np.uint8)
    P = np.argwhere(g == 0)[:, ::-1]
    for k in range(z):
        for j in range(y):
            for i in range(x):
                a = dr.walls_by_definition(g, P, (i, j, k))
                assert np.array_equal(a, dr.walls_by_template(g, P, (i, j, k))) and np.array_equal(a, dr.walls(g, P, (i, j, k))), (i, j, k)
    for s in ((0, 0, 0), (x - 1, y - 1, z - 1), (x - 1, 0, z - 1)):
        for p in P:
            mask = np.zeros(g.shape, bool)
            for i, j, k in dr.crossed_by_template(tuple(p), s):
                assert not mask[k, j, i]
                mask[k, j, i] = True
            assert np.array_equal(mask, dr.crossed_by_definition(g.shape, tuple(p), s)), (p, s)


def test_the_far_pairs_of_the_32_bit_edge():
    """|d| = (1023, 1023, 1) and (1023, 1022, 0): the vectorised walk equals the template's periods taken literally, and the
    segments are as long as the rule says: one voxel per distinct crossing time, less the arrival."""
    g = _edge1024()
    for p, s in (((1023, 1023, 1), (0, 0, 0)), ((1023, 1022, 0), (0, 0, 0)), ((0, 0, 1), (1023, 1023, 0)), ((1023, 1022, 0), (0, 1023, 0))):
        cells = dr.crossed_by_template(p, s)
        assert len(set(cells)) == len(cells)
        assert int(dr.walls(g, [p], s)[0]) == sum(int(g[k, j, i]) for i, j, k in cells)
    assert len(dr.crossed_by_template((1023, 1023, 1), (0, 0, 0))) == 1023 - 1             # 1023 joint x-y steps, the z step at t = 1 / 2 among them
    assert len(dr.crossed_by_template((1023, 1022, 0), (0, 0, 0))) == 1023 + 1022 - 1      # coprime: no two times are equal


def _closed_forms(run):
    """run(g, sources, transmit, falloff, mode, reach) -> (e, covered, summary).  The closed forms of DESIGN.md section 31."""
    A, S, N, Q = dr.DOSE_ALL, dr.DOSE_SKIN, dr.FALLOFF_NONE, dr.FALLOFF_INVERSE_SQUARE
    # corner cutting: the segment through the shared edge crosses neither voxel it touches
    g = np.zeros((2, 2, 2), np.uint8)
    g[0, 0, 1] = g[0, 1, 0] = 1
    e, cov, s = run(g, [(1, 1, 0, 1000)], HALVING, N, A, None)
    assert e[0, 0, 0] == 1000 and e[0, 1, 1] == 1000 and int(cov[0]) == int(s["evaluated"]) == 6 and (e[g == 1] == -1).all()
    # a line through a centre: d = (4, 2, 0) passes the centre of (2, 1, 0)
    g = np.zeros((1, 3, 5), np.uint8)
    g[0, 1, 2] = 1
    e, cov, s = run(g, [(4, 2, 0, 1000)], HALVING, N, A, None)
    assert e[0, 0, 0] == 500 and int(dr.walls_by_definition(g, [(0, 0, 0)], (4, 2, 0))[0]) == 1
    g = np.zeros((1, 3, 5), np.uint8)
    for i, j in ((1, 0), (1, 1), (3, 1), (3, 2)):
        g[0, j, i] = 1
    k = int(dr.walls_by_definition(g, [(0, 0, 0)], (4, 2, 0))[0])
    assert k == 4
    e, cov, s = run(g, [(4, 2, 0, 64000)], [65536 >> i for i in range(6)], N, A, None)
    assert e[0, 0, 0] == 64000 >> k
    # a source in a SOLID voxel does not count itself; p = s has D = 1 and k = 0
    g = np.zeros((1, 1, 5), np.uint8)
    g[0, 0, 4] = 1
    e, cov, s = run(g, [(4, 0, 0, 900), (1, 0, 0, 7)], SIGHT, Q, A, None)
    assert e[0, 0].tolist() == [900 // 16 + 7, 900 // 9 + 7, 900 // 4 + 7, 900 + 7 // 4, -1] and cov.tolist() == [4, 4]
    assert int(s["peak"]) == 901 and int(s["peak_voxel"]) == 3 and int(s["seen"]) == 4
    # one SOLID voxel at the centre of 21^3, one corner source: 70 voxels lie in its shadow (test_closed_forms counts them by form (a))
    g = np.zeros((21, 21, 21), np.uint8)
    g[10, 10, 10] = 1
    e, cov, s = run(g, [(0, 0, 0, 5)], SIGHT, N, A, None)
    assert int(s["dark"]) == 70 == int((e == 0).sum()) and e[10, 10, 10] == -1 and int(cov[0]) == 9260 - 70 == int(s["seen"])
    assert int(s["total"]) == 5 * (9260 - 70) and int(s["peak"]) == 5 and int(s["peak_voxel"]) == 0 and e[20, 20, 20] == 0 and e[11, 11, 10] == 0
    # an empty grid: e = the sum of floor(w / D); without falloff e == W wherever every source is in reach
    g = np.zeros((3, 4, 5), np.uint8)
    src = [(0, 0, 0, 1000), (4, 3, 2, 77), (2, 1, 1, 0), (2, 1, 1, 5)]
    e, cov, s = run(g, src, SIGHT, N, A, None)
    assert (e == 1082).all() and cov.tolist() == [60] * 4 and int(s["seen"]) == 60 and int(s["dark"]) == 0 and int(s["peak_voxel"]) == 0
    e, cov, s = run(g, src, SIGHT, Q, A, None)
    zz, yy, xx = np.mgrid[0:3, 0:4, 0:5]
    want = sum(w // np.maximum(1, (xx - i) ** 2 + (yy - j) ** 2 + (zz - k) ** 2) for i, j, k, w in src)
    assert np.array_equal(e, want) and int(s["total"]) == int(want.sum())
    e, cov, s = run(g, src, SIGHT, N, A, 2)
    near = [np.maximum(np.maximum(abs(xx - i), abs(yy - j)), abs(zz - k)) <= 2 for i, j, k, w in src]
    assert np.array_equal(e, sum(n * w for n, (_, _, _, w) in zip(near, src))) and cov.tolist() == [int(n.sum()) for n in near]
    e, cov, s = run(g, src, SIGHT, N, S, None)                           # no SOLID voxel: no skin
    assert (e == -1).all() and cov.tolist() == [0] * 4 and s.tolist() == (0, 0, 0, 0, -1, -1)
    # a full grid: nothing is evaluated
    g = np.ones((3, 4, 5), np.uint8)
    for mode in MODES:
        e, cov, s = run(g, src, HALVING, Q, mode, None)
        assert (e == -1).all() and cov.tolist() == [0] * 4 and s.tolist() == (0, 0, 0, 0, -1, -1)
    # the 64-bit product: w = 2^31 - 1 passes T[0] = 65536 whole
    g = np.zeros((1, 2, 3), np.uint8)
    e, cov, s = run(g, [(1, 1, 0, 2 ** 31 - 1)], SIGHT, N, A, None)
    assert (e == 2 ** 31 - 1).all() and int(s["total"]) == 6 * (2 ** 31 - 1) and int(s["peak"]) == 2 ** 31 - 1
    # a table that is not monotone: one wall is opaque, two walls are clear again; only trailing zeros end a pair early
    g = np.zeros((1, 1, 6), np.uint8)
    g[0, 0, 1] = g[0, 0, 3] = 1
    e, cov, s = run(g, [(5, 0, 0, 100)], GAP, N, A, None)
    assert e[0, 0].tolist() == [100, -1, 0, -1, 100, 100] and cov.tolist() == [2] and int(s["seen"]) == 2 and int(s["dark"]) == 1
    e, cov, s = run(g, [(5, 0, 0, 100)], [65536, 0, 65536, 0, 0], N, A, None)
    assert e[0, 0].tolist() == [100, -1, 0, -1, 100, 100]
    e, cov, s = run(g, [(5, 0, 0, 100)], [0, 0], N, A, None)             # all zero: nothing arrives, the coverage still counts
    assert e[0, 0].tolist() == [0, -1, 0, -1, 0, 0] and cov.tolist() == [2] and int(s["dark"]) == 4 and int(s["peak_voxel"]) == 0
    # k >= m transmits 0: SOLID runs of 63, 64 and 65 under a 64-entry table whose last entry is not zero
    for run_len, want in ((63, (100 * LONG_TABLE[63]) >> 16), (64, 0), (65, 0)):
        g = _run130(run_len)
        e, cov, s = run(g, [(129, 0, 0, 100)], LONG_TABLE, N, A, None)
        assert e[0, 0, 0] == want and (e[0, 0, 1 + run_len:] == 100).all() and int(cov[0]) == 129 - run_len, run_len


def _host_run(g, sources, transmit, falloff, mode, reach):
    import ray_tracing_octrees_amd as rto
    rc, e, cov, s = rto.VoxelGrid.from_array(g, (0.0, 0.0, 0.0), 1.0).doseField(sources, transmit, falloff, mode, dr.NO_LIMIT if reach is None else reach)
    assert rc == 0
    return e, cov, s


def _ref_run(walls):
    return lambda g, src, t, f, m, r: dr.dose(g, src, t, f, m, dr.NO_LIMIT if r is None else r, walls)


def test_closed_forms():
    g = np.zeros((21, 21, 21), np.uint8)                                 # the 70 of the 21^3 closed form, by form (a) over every voxel
    g[10, 10, 10] = 1
    assert int((dr.walls_by_definition(g, np.argwhere(g == 0)[:, ::-1], (0, 0, 0)) > 0).sum()) == 70
    _closed_forms(_ref_run(dr.walls))
    _closed_forms(lambda g, src, t, f, m, r: _ref_run(dr.walls_by_definition if g.size <= 130 else dr.walls)(g, src, t, f, m, r))
    _closed_forms(_host_run)


def _same(got, want, what):
    e, cov, s = got
    we, wcov, ws = want
    assert e.dtype == np.int32 and e.shape == we.shape, what
    assert np.array_equal(e, we), f"{what}: {int((e != we).sum())} voxels differ"
    assert np.array_equal(cov, wcov), (what, cov, wcov)
    assert s.tobytes() == ws.tobytes(), (what, s, ws)


@pytest.mark.parametrize("name", [*sorted(SEEDED), *sorted(WALLS)])
def test_reference_equals_the_host_layers_walk(name):
    """tests/dose_ref.py against doseFieldCPU (host/Dose.cpp): field, coverage and summary bytes, on the GPU tests' named grids."""
    g = _named(name)
    src = _sources(name, g)
    for t, f, m, r in _cases(name):
        _same(_host_run(g, src, t, f, m, r), _ref(name, g, src, t, f, m, r), (name, t, f, m, r))


def test_reference_equals_the_host_layers_walk_on_the_special_grids():
    for x in (1, 63, 64, 65, 255, 256, 257):
        for r in (1, None):
            _same(_host_run(_row(x), _row_sources(x), HALVING, 1, 0, r), _ref(f"row{x}", _row(x), _row_sources(x), HALVING, 1, 0, r), x)
    g = _named("s33x9x9_10")
    for n in (1, 64, 65, 1024):
        src = _count_sources(g, n)
        for m, r in ((dr.DOSE_ALL, None), (dr.DOSE_SKIN, 3)):
            _same(_host_run(g, src, HALVING, 1, m, r), _ref("s33x9x9_10", g, src, HALVING, 1, m, r), (n, m, r))
    g = _floor128()
    _same(_host_run(g, FLOOR_SOURCE, SIGHT, 0, 0, 4), _ref("floor128", g, FLOOR_SOURCE, SIGHT, 0, 0, 4), "floor128")
    g = _edge1024()
    _same(_host_run(g, EDGE_SOURCES, HALVING, 1, 1, None), _ref("edge1024", g, EDGE_SOURCES, HALVING, 1, 1, None), "edge1024")


@pytest.mark.parametrize("dims", TILE_SIZED)
@pytest.mark.parametrize("fill", [3, 10])
def test_the_seeded_grids_exercise_both_sides(dims, fill):
    """Under ALL with no reach and the cap's four sources, the share of pairs with k = 0 lies in [0.05, 0.8] and the share with
    k >= 2 is at least 0.05: the clear side and the counting side of the march are both exercised."""
    x, y, z = dims
    name = f"s{x}x{y}x{z}_{fill}"
    g = _named(name)
    counts = {}
    _ref(name, g, [(*p, 1) for p in _cap_sources(g)], SIGHT, 0, dr.DOSE_ALL, None, counts)
    clear, two = counts["clear"] / counts["pairs"], counts["two"] / counts["pairs"]
    print(f"{name}: k = 0 share {clear:.3f}, k >= 2 share {two:.3f}")
    assert counts["pairs"] == 4 * int((g == 0).sum()) and 0.05 <= clear <= 0.8 and two >= 0.05, (name, clear, two)


def test_host_layer_refusals():
    """The refusals of the host form, in rto_dose_field's order: of several faults the first in the list is the one reported."""
    import ray_tracing_octrees_amd as rto
    hip = _hip()
    g = _seeded(5, 3, 2, 10)
    vg = rto.VoxelGrid.from_array(g, (0.0, 0.0, 0.0), 1.0)
    ok = [(0, 0, 0, 1), (4, 2, 1, 2)]
    big = 2 ** 31 - 1
    out = [(5, 0, 0, 1)]
    bad = [(None,), ([(0, 0, 0, 1)] * 1025,), (np.zeros((0, 4), np.int32),), ([(0, 0, 0, -1)],), ([(0, 0, 0, big), (1, 0, 0, 1)],), (ok, []), (ok, [1] * 65),
           (ok, [65537]), (ok, None, 2), (ok, None, -1), (ok, None, 0, 2), (ok, None, 0, -1), (ok, None, 0, 0, 0), (ok, None, 0, 0, -3),
           (out,), ([(0, 0, 0, 1), (0, 3, 0, 1)],), ([(0, 0, 2, 1)],), ([(-1, 0, 0, 1)],)]
    for args in bad:
        rc, e, cov, _ = vg.doseField(*args)
        assert rc == hip.RTO_E_INVALID and e is None and cov is None, args
        if args[0] is not None and len(args[0]):
            with pytest.raises(ValueError):
                dr.dose(g, *args)
    assert vg.doseField([(0, 0, 0, 1), (0, 3, 0, 1)])[0] == hip.RTO_E_INVALID and vg.badSource == 1
    assert vg.doseField([(0, 0, 0, big - 1), (1, 0, 0, 1)])[0] == 0 and vg.doseField([(1, 1, 1, 1)] * 1024)[0] == 0
    assert vg.doseField(ok, [65536] * 64, 1, 1, 1)[0] == 0 and vg.doseField(ok, [0])[0] == 0
    # the order: every argument comes before a source's place; badSource is set by that last refusal alone
    for args in (([(9, 9, 9, -1)],), ([(9, 9, 9, 1)], [65537]), ([(9, 9, 9, 1)], None, 7), ([(9, 9, 9, 1)], None, 0, 7), ([(9, 9, 9, 1)], None, 0, 0, 0)):
        assert vg.doseField(*args)[0] == hip.RTO_E_INVALID and vg.badSource == -1, args
    assert vg.doseField([(9, 9, 9, 1)])[0] == hip.RTO_E_INVALID and vg.badSource == 0
    # a reach above RTO_DOSE_MAX_REACH stands for it
    assert np.array_equal(vg.doseField(ok, None, 0, 0, 5000)[1], vg.doseField(ok, None, 0, 0, dr.NO_LIMIT)[1])


def test_dose_abi_layout_and_exports():
    """sizeof(rto_dose_summary) == 48 with the fields where DOSE_SUMMARY_DTYPE puts them; the constants; the five symbols are
    exported and declared; no RTO_FIELD_* code stands for the dose field."""
    hip = _hip()
    assert hip.DOSE_SUMMARY_DTYPE.itemsize == 48 and dr.SUMMARY_DTYPE == hip.DOSE_SUMMARY_DTYPE
    fields = ("evaluated", "total", "dark", "seen", "peak", "peak_voxel")
    assert [hip.DOSE_SUMMARY_DTYPE.fields[f][1] for f in fields] == [0, 8, 16, 24, 32, 40]
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.fail("no C compiler: the header's layout cannot be checked")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "abi.c")
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "rto_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu '
                    '%d %d %d %d %d %d %d %d\\n", sizeof(rto_dose_summary), offsetof(rto_dose_summary, evaluated), '
                    'offsetof(rto_dose_summary, total), offsetof(rto_dose_summary, dark), offsetof(rto_dose_summary, seen), '
                    'offsetof(rto_dose_summary, peak), offsetof(rto_dose_summary, peak_voxel), RTO_DOSE_ALL, RTO_DOSE_SKIN, '
                    'RTO_DOSE_FALLOFF_NONE, RTO_DOSE_FALLOFF_INVERSE_SQUARE, RTO_DOSE_MAX_SOURCES, RTO_DOSE_MAX_REACH, RTO_DOSE_MAX_TABLE, '
                    'RTO_DOSE_NO_LIMIT); return 0; }\n')
        exe = os.path.join(tmp, "abi")
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    consts = (dr.DOSE_ALL, dr.DOSE_SKIN, dr.FALLOFF_NONE, dr.FALLOFF_INVERSE_SQUARE, dr.MAX_SOURCES, dr.MAX_REACH, dr.MAX_TABLE, dr.NO_LIMIT)
    assert out == [str(v) for v in (48, 0, 8, 16, 24, 32, 40, *consts)]
    assert consts == (0, 1, 0, 1, 1024, 1023, 64, 0x7fffffff)
    assert consts == (hip.DOSE_ALL, hip.DOSE_SKIN, hip.DOSE_FALLOFF_NONE, hip.DOSE_FALLOFF_INVERSE_SQUARE, hip.DOSE_MAX_SOURCES, hip.DOSE_MAX_REACH,
                      hip.DOSE_MAX_TABLE, hip.DOSE_NO_LIMIT)
    L = hip.load()
    header = open(os.path.join(ROOT, "include", "rto_hip.h")).read()
    for s in SYMS:
        assert s in hip.SYMBOLS and hasattr(L, s), s
        assert s + "(" in header, s
    assert "RTO_FIELD_DOSE" not in header and not hasattr(hip, "FIELD_DOSE") and hip.FIELD_CALLER == 7


def test_dose_kernels_keep_their_budgets():
    """The built assembly (the product's flags): exactly the two k_dose_* kernels, without scratch, spills or v_mfma, within the
    VGPR and LDS figures DESIGN.md section 31 states; the march reads the source record through a scalar load and writes LDS only
    to stage the table, before its first read."""
    import test_isa_contract as isa
    asm = isa.built_asm()
    if asm is None:
        pytest.fail("no hipcc: the budget cannot be checked")
    meta = isa.kernel_meta(asm)
    names = [k for k in meta if "k_dose_" in k]
    assert len(names) == 2 and sorted(next(b for b in DOSE_VGPR if b in k) for k in names) == sorted(DOSE_VGPR), names
    for k in names:
        m = meta[k]
        base = next(b for b in DOSE_VGPR if b in k)
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (k, m)
        assert m["vgpr"] <= DOSE_VGPR[base], (k, m)
        entry = re.search(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\.group_segment_fixed_size).)*?\.name:\s+" + re.escape(k) + r"\n", asm, re.S)
        assert entry and int(entry.group(1)) <= DOSE_LDS[base], (k, entry and entry.group(1))
        ins = isa.body(asm, k[len("_ZN3rto"):])
        assert not any(t.startswith("scratch_") or "v_mfma" in t for t in ins), k
        if base == "k_dose_march":
            barrier = next(i for i, t in enumerate(ins) if t.startswith("s_barrier"))
            assert any(t.startswith("s_load_dwordx4") for t in ins[barrier + 1:]), k      # in the source loop, not among the kernel arguments
            writes = [i for i, t in enumerate(ins) if t.startswith("ds_write") or t.startswith("ds_store")]
            reads = [i for i, t in enumerate(ins) if t.startswith("ds_read") or t.startswith("ds_load")]
            assert writes and reads and max(writes) < min(reads), (k, writes, reads)


def test_sanitizer_script_reports_nothing():
    """tools/sanitize_dose.sh: host/Dose.cpp as a stand-alone program under AddressSanitizer and UBSan."""
    if not shutil.which("g++"):
        pytest.fail("no g++: the sanitizer build cannot be made")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize_dose.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dose selftest ok" in r.stdout and "UBSan reports: 0" in r.stdout and "ASan reports: 0" in r.stdout, r.stdout


# ================================================================ GPU
gpu = pytest.mark.gpu
W, H, FOV = 128, 96, 45.0
GMIN, VOX = np.array([-0.5, -0.5, -0.5], np.float32), np.float32(1.0 / 64)


def _build(ctx, grid, gmin=GMIN, vox=VOX):
    ctx.set_kernel(_hip().KERNEL_AUTO)
    ctx.build_octree(grid, gmin, vox)


def _check(ctx, g, want, sources, transmit, falloff, mode, reach, what):
    e, s = ctx.dose_field(sources, transmit, falloff, mode, reach)
    _same((e, ctx.dose_coverage(), s), want, what)
    p = ctx.dose_device()
    assert p and _tc()._d2h(p, 4 * g.size).tobytes() == want[0].tobytes(), f"{what}: the device pointer's copy"
    ms = ctx.last_dose_ms()
    assert all(t >= 0 for t in ms), (what, ms)
    return e


def _check_field(ctx, name, g, sources, transmit, falloff, mode, reach):
    return _check(ctx, g, _ref(name, g, sources, transmit, falloff, mode, reach), sources, transmit, falloff, mode, reach,
                  f"{name} n {len(sources)} table {transmit} falloff {falloff} mode {mode} reach {reach}")


def _gpu_run(ctx):
    def run(g, sources, transmit, falloff, mode, reach):
        _build(ctx, g)
        e, s = ctx.dose_field(sources, transmit, falloff, mode, reach)
        return e, ctx.dose_coverage(), s
    return run


@gpu
@pytest.mark.parametrize("name", sorted(SEEDED))
def test_gpu_seeded_grids_equal_the_rule(ctx, name):
    """e, the coverage, the summary and the device copy bit for bit: both modes and falloffs, reach 1, 3 and none, the three short
    tables, weights 1 + 1000 (index % 7) with a zero among them, a source in a SOLID voxel and one given twice."""
    g = _named(name)
    _build(ctx, g)
    src = _sources(name, g)
    for t, f, m, r in _cases(name):
        _check_field(ctx, name, g, src, t, f, m, r)


@gpu
@pytest.mark.parametrize("name", sorted(WALLS))
def test_gpu_walls_at_word_and_tile_edges(ctx, name):
    """A one-voxel wall at x = 31, x = 32, y = 7, y = 8, z = 7, z = 8 of 65 x 17 x 17, whole and with a one-voxel hole, sources on
    both sides and in the wall: segments cross the word boundary and every tile face both ways."""
    g = _named(name)
    _build(ctx, g)
    src = _sources(name, g)
    for t, f, m, r in _cases(name):
        e = _check_field(ctx, name, g, src, t, f, m, r)
        assert (e[g == 1] == -1).all() and (e[g == 0] >= 0).any(), name


@gpu
@pytest.mark.parametrize("x", [1, 63, 64, 65, 255, 256, 257])
def test_gpu_list_sizes_around_a_wave_and_a_workgroup(ctx, x):
    """Mode ALL on an empty x * 1 * 1 row: the list is every voxel, one entry, a wave or a workgroup less one, whole, and one more."""
    g = _row(x)
    _build(ctx, g)
    src = _row_sources(x)
    for r in (1, None):
        _check_field(ctx, f"row{x}", g, src, HALVING, 1, dr.DOSE_ALL, r)
    e, s = ctx.dose_field(src)
    assert (e == sum(w for *_, w in src)).all() and ctx.dose_coverage().tolist() == [x] * len(src)
    e, s = ctx.dose_field(src, None, 0, dr.DOSE_SKIN)                    # nothing is listed: no march and no summary launch
    assert (e == -1).all() and s.tolist() == (0, 0, 0, 0, -1, -1) and ctx.dose_coverage().tolist() == [0] * len(src)
    assert ctx.last_dose_ms()[1] >= 0


@gpu
@pytest.mark.parametrize("n", [1, 64, 65, 1024])
def test_gpu_source_counts(ctx, n):
    """n sources cycling over the grid, SOLID voxels included; under SKIN with reach 3 most waves have no clear lane for most
    sources, so their atomic is skipped."""
    name = "s33x9x9_10"
    g = _named(name)
    _build(ctx, g)
    src = _count_sources(g, n)
    _check_field(ctx, name, g, src, HALVING, 1, dr.DOSE_ALL, None)
    e = _check_field(ctx, name, g, src, HALVING, 1, dr.DOSE_SKIN, 3)
    if n == 1024:
        waves = -(-int((e >= 0).sum()) // 64)
        cov = ctx.dose_coverage()
        assert waves == 18 and (cov > 0).all() and (cov < waves).any()    # fewer clear voxels than waves: some wave has none, and adds nothing


@gpu
def test_gpu_a_list_beyond_the_summarys_grid(ctx):
    """k_dose_summary runs at most 4,096 workgroups and strides: 128 x 128 x 66 with a SOLID floor and one SOLID voxel above it lists
    1,064,959 voxels.  One source, reach 4, line of sight: every voxel that sees it holds the peak, the smallest index wins."""
    g = _floor128()
    _build(ctx, g, np.array([-1.0, -1.0, -0.5], np.float32))
    e = _check_field(ctx, "floor128", g, FLOOR_SOURCE, SIGHT, 0, dr.DOSE_ALL, 4)
    s = ctx.dose_field(FLOOR_SOURCE, SIGHT, 0, dr.DOSE_ALL, 4)[1]
    assert int(s["evaluated"]) == 65 * 128 * 128 - 1 == 1064959 > 4096 * 256
    assert int(s["peak"]) == 777 and int(s["peak_voxel"]) == 60 + 128 * (60 + 128 * 34) and int(s["seen"]) < 9 ** 3 - 1
    assert e[41, 64, 64] == 0 and e[42, 64, 64] == 0 and e[39, 64, 64] == 777 and e[43, 64, 64] == 0 and e[34, 60, 60] == 777


@gpu
def test_gpu_the_32_bit_edge(ctx):
    """|d| = (1023, 1023, 1) and (1023, 1022, 0): the crossing times on their common denominator come within 0.25 % of 2^31."""
    g = _edge1024()
    _build(ctx, g, np.array([-8.0, -8.0, -0.5], np.float32))
    e = _check_field(ctx, "edge1024", g, EDGE_SOURCES, HALVING, 1, dr.DOSE_SKIN, None)
    listed = int((e >= 0).sum())
    assert listed == 13 * 5 + 3 * 4                                      # two layers: five face neighbours in the grid, four at a border
    assert e[1, 1023, 1023] >= 0 and e[0, 1022, 1023] >= 0 and e[1, 0, 0] >= 12345
    _check_field(ctx, "edge1024", g, EDGE_SOURCES, SIGHT, 0, dr.DOSE_SKIN, None)


@gpu
def test_gpu_closed_forms(ctx):
    _closed_forms(_gpu_run(ctx))


@gpu
def test_gpu_sphere64_equals_the_host_layer(ctx, scenes):
    """SKIN with 8 sources on a ring outside the sphere but inside the grid, against host/Dose.cpp; and through the host class."""
    import ray_tracing_octrees_amd as rto
    hip = _hip()
    g = scenes("sphere64").grid
    data = np.ascontiguousarray(g.data, np.uint8)
    dz, dy, dx = data.shape
    ring = [(int(round(dx / 2 + (dx / 2 - 2) * np.cos(a))), int(round(dy / 2 + (dy / 2 - 2) * np.sin(a))), dz // 2) for a in np.arange(8) * (np.pi / 4)]
    ring = [(min(max(i, 0), dx - 1), min(max(j, 0), dy - 1), k) for i, j, k in ring]
    assert all(data[k, j, i] == 0 for i, j, k in ring)
    src = [(*p, 50000 + 1000 * n) for n, p in enumerate(ring)]
    vg = rto.VoxelGrid.from_array(data, g.min, g.voxel_size)
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(data, g.min, g.voxel_size)
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    assert rt.doseField(src)[0] == hip.RTO_E_NO_OCTREE and rt.dose()[0] != 0
    rt.setOctreeFromGrid(rto.VoxelGrid.from_array(data, g.min, g.voxel_size))
    assert rt.dose()[0] == hip.RTO_E_INVALID and rt.doseCoverage()[0] == hip.RTO_E_INVALID        # no field yet
    for t, f, r in ((None, 0, None), (HALVING, 1, None), (HALVING, 1, 16)):
        rc, want, wcov, ws = vg.doseField(src, t, f, hip.DOSE_SKIN, hip.DOSE_NO_LIMIT if r is None else r)
        assert rc == 0 and 0 < int(ws["seen"]) < int(ws["evaluated"]) and (wcov > 0).all()                # some pairs blocked, some clear
        _check(ctx, data, (want, wcov, ws), src, t, f, hip.DOSE_SKIN, r, f"sphere64 reach {r}")
        rc, s = rt.doseField(src, t, f, hip.DOSE_SKIN, hip.DOSE_NO_LIMIT if r is None else r)
        assert rc == 0 and s.tobytes() == ws.tobytes()
        rc, e = rt.dose()
        assert rc == 0 and np.array_equal(e, want)
        rc, cov = rt.doseCoverage()
        assert rc == 0 and np.array_equal(cov, wcov)
        rc, ijk, value = rt.hottestVoxel()
        v = int(ws["peak_voxel"])
        assert rc == 0 and ijk == (v % dx, v // dx % dy, v // dx // dy) and value == int(ws["peak"])
    assert rt.doseField([(dx, 0, 0, 1)])[0] == hip.RTO_E_INVALID and rt.doseField(src, None, 0, 7)[0] == hip.RTO_E_INVALID
    assert np.array_equal(rt.dose()[1], want) and np.array_equal(rt.doseCoverage()[1], wcov) and np.array_equal(rt.grid(), data)


@gpu
def test_gpu_the_dose_field_through_the_viewers(ctx, orc):
    """dose_device() handed to render_field_device as FIELD_CALLER: per-pixel values equal to the reference field sampled at the
    same voxels (tests/field_view_ref.py), colours, summary and bins included; and source 8 stays unknown."""
    torch = pytest.importorskip("torch")
    import field_view_ref as fr
    import query_ref as q
    import test_field_view as tf
    hip = _hip()
    g, nodes, T = tf._tree(orc, "base")
    _build(ctx, g)
    src = [(0, 0, 0, 90000), (39, 11, 11, 70000), (22, 6, 6, 50000)]
    want, _, _ = _ref("base", g, src, HALVING, 1, dr.DOSE_SKIN, None)
    e, _ = ctx.dose_field(src, HALVING, 1, dr.DOSE_SKIN)
    assert np.array_equal(e, want)
    view, pos = tf._camera(orc, "outside")
    Wv, Hv = 72, 40
    f = tf._frame(view, pos, Wv, Hv)
    v = hip.make_field_view(hip.FIELD_CALLER, sample=hip.SAMPLE_FRONT, shade=True)
    ref = fr.frame(T, GMIN, VOX, pos, tf._rays(orc, view, pos, Wv, Hv), Wv, Hv, np.asarray(want), v, tf._lut())
    assert ref[2]["valued"] >= 20 and ref[2]["vmin"] < ref[2]["vmax"]
    d_lut = torch.from_numpy(tf._lut().view(np.int32)).cuda()
    d_rgba = torch.zeros(Wv * Hv * 4, dtype=torch.float32, device="cuda")
    d_values = torch.zeros(Wv * Hv, dtype=torch.int32, device="cuda")
    d_summary = torch.zeros(4, dtype=torch.int64, device="cuda")
    d_bins = torch.zeros(256, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.render_field_device(f, v, d_lut.data_ptr(), d_rgba.data_ptr(), ctx.dose_device(), d_values.data_ptr(), d_summary.data_ptr(), d_bins.data_ptr())
    ctx.synchronize()
    assert np.array_equal(d_values.cpu().numpy().reshape(Hv, Wv), ref[1])
    assert d_rgba.cpu().numpy().tobytes() == ref[0].tobytes()
    assert d_summary.cpu().numpy().view(hip.FIELD_VIEW_SUMMARY_DTYPE)[0].tolist() == tuple(int(ref[2][k]) for k in ("hits", "valued", "vmin", "vmax", "lo", "hi"))
    assert np.array_equal(d_bins.cpu().numpy(), ref[3])
    with pytest.raises(hip.RtoError) as err:
        ctx.render_field_host(f, hip.make_field_view(8), tf._lut())
    assert err.value.code == hip.RTO_E_INVALID and "unknown source" in str(err.value)
    assert np.array_equal(ctx.dose(), want)


@gpu
def test_gpu_dose_field_is_dropped_when_the_grid_changes_and_touches_nothing_else(ctx, orc, scenes):
    from conftest import assert_bit_exact, make_camera
    hip = _hip()
    tc = _tc()
    g = scenes("sphere64").grid
    data = np.ascontiguousarray(g.data, np.uint8)
    src = [(0, 0, 0, 1000), (63, 63, 63, 2000), (0, 63, 32, 3000)]

    def gone():
        for read in (ctx.dose, ctx.dose_device, ctx.dose_coverage):
            with pytest.raises(hip.RtoError) as e:
                read()
            assert e.value.code == hip.RTO_E_INVALID and "no dose field is resident" in str(e.value)

    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(data, g.min, g.voxel_size)
    gone()                                                              # never made
    view, pos = make_camera(orc, 0.5, 0.7, 1.8)
    frame = hip.make_frame(view, pos, W / H, FOV, W, H)
    before = ctx.render_host(frame)
    # labels and the six other fields resident before the call are byte-identical after it
    table = ctx.label_components(1, 6)
    labels = ctx.component_labels()
    dist, _ = ctx.distance_field(1)
    geo, _ = ctx.geodesic_field([0], 0, 26, 200)
    thick, _ = ctx.thickness_field(1, 4 * float(g.voxel_size))
    skel, _ = ctx.skeleton_field(1, 26, 1, (), 2)
    expo, _ = ctx.exposure_field([(0, 0, 1), (1, 1, 1)], None, hip.EXPO_SKIN, 8)
    ctx.segment_parts(1, 26, 500)
    parts = ctx.part_labels()
    nodes, info = ctx.download_nodes(), bytes(ctx.info())
    first, s1 = ctx.dose_field(src, HALVING, 1, hip.DOSE_SKIN)
    cov1 = ctx.dose_coverage()
    assert len(cov1) == 3 and int(s1["evaluated"]) > 0
    assert np.array_equal(ctx.component_labels(), labels) and ctx.components().tobytes() == table.tobytes()
    assert np.array_equal(ctx.distance(), dist) and np.array_equal(ctx.geodesic(), geo) and np.array_equal(ctx.thickness(), thick)
    assert np.array_equal(ctx.skeleton(), skel) and np.array_equal(ctx.exposure(), expo) and np.array_equal(ctx.part_labels(), parts)
    assert ctx.download_nodes().tobytes() == nodes.tobytes() and bytes(ctx.info()) == info and np.array_equal(ctx.download_voxels(), data)
    assert_bit_exact(ctx.render_host(frame), before, "the frame after dose_field")
    og = orc.Grid(data.shape[::-1], g.min, g.voxel_size, data)
    tc._check_render(ctx, orc, og, orc.build_flat_octree(og), view, pos, "after dose_field")
    # the other fields' calls leave it alone, and a second call replaces the first
    ctx.label_components(0, 26)
    ctx.distance_field(0)
    ctx.geodesic_field([0])
    ctx.skeleton_field()
    ctx.exposure_field([(1, 0, 0)])
    assert np.array_equal(ctx.dose(), first) and np.array_equal(ctx.dose_coverage(), cov1)
    second, s2 = ctx.dose_field(src[:2], None, 0, hip.DOSE_ALL, 4)
    assert second.shape == first.shape and int(s2["evaluated"]) == int((data == 0).sum()) > int(s1["evaluated"])
    assert np.array_equal(ctx.dose(), second) and not np.array_equal(second, first) and len(ctx.dose_coverage()) == 2
    # every call that changes or replaces the grid drops the field and the coverage table
    ctx.build_octree(data, g.min, g.voxel_size)                         # build
    gone()
    ctx.dose_field(src)
    corner = hip.make_brushes([np.asarray(g.min, np.float32) + np.float32(0.5) * g.voxel_size], 0.5 * float(g.voxel_size),
                              hip.BRUSH_SPHERE, hip.EDIT_FILL)
    assert ctx.edit_voxels(corner) == 1                                 # rto_edit_voxels
    gone()
    ctx.dose_field(src)                                                 # a source in the voxel just filled
    assert ctx.edit_skeleton(1, 26, 0, (), 1) > 0                       # rto_edit_skeleton
    gone()
    ctx.dose_field(src)
    v, tris = tc._box_mesh([0.3, 0.3, 0.3], [0.7, 0.7, 0.7])
    ctx.voxelize_mesh(v, tris, np.float32(0.125), grid=((8, 8, 8), np.zeros(3, np.float32), np.float32(0.125)))     # voxelize
    gone()
    e, _ = ctx.dose_field([(0, 0, 0, 5)])
    assert e.shape == (8, 8, 8)
    ctx.upload_octree(scenes("sphere64").nodes, g.min, g.voxel_size)    # upload: no grid either
    gone()


@gpu
def test_gpu_dose_errors_leave_the_context_untouched(ctx, orc, scenes):
    from conftest import assert_bit_exact, make_camera
    hip = _hip()
    g = scenes("sphere64").grid
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    src = [(0, 0, 0, 1000), (63, 63, 63, 2000)]
    field, _ = ctx.dose_field(src, HALVING, 1, hip.DOSE_SKIN, 40)
    cover = ctx.dose_coverage()
    expo, _ = ctx.exposure_field([(0, 0, 1)], None, hip.EXPO_SKIN, 8)
    nodes, info = ctx.download_nodes(), bytes(ctx.info())
    view, pos = make_camera(orc, 0.5, 0.7, 1.8)
    frame = hip.make_frame(view, pos, W / H, FOV, W, H)
    before = ctx.render_host(frame)
    L, h = ctx._L, ctx._h
    nvox = g.data.size
    i32 = lambda v: np.asarray(v, np.int32)
    u32 = lambda v: np.asarray(v, np.uint32)
    ok, neg, heavy, fine = i32([0, 0, 0, 1, 1, 1, 1, 1]), i32([0, 0, 0, 1, 1, 1, 1, -1]), i32([0, 0, 0, 2 ** 31 - 1, 1, 1, 1, 1]), i32([0, 0, 0, 2 ** 31 - 2, 1, 1, 1, 1])
    outside, below = i32([0, 0, 0, 1, 64, 0, 0, 1]), i32([0, -1, 0, 1, 1, 1, 1, 1])
    many = np.ones(4 * 1025, np.int32)
    table, over, long = u32(HALVING), u32([65536, 65537]), u32([1] * 65)
    small = np.zeros(nvox - 1, np.int32)
    cov1 = np.zeros(1, np.int64)
    NL = hip.DOSE_NO_LIMIT
    p = lambda a: a.ctypes.data
    cases = [
        ("NULL sources", lambda: L.rto_dose_field(h, None, 2, None, 0, 0, 0, NL, None)),
        ("n = 0", lambda: L.rto_dose_field(h, p(ok), 0, None, 0, 0, 0, NL, None)),
        ("n < 0", lambda: L.rto_dose_field(h, p(ok), -2, None, 0, 0, 0, NL, None)),
        ("n = 1025", lambda: L.rto_dose_field(h, p(many), 1025, None, 0, 0, 0, NL, None)),
        ("a negative weight", lambda: L.rto_dose_field(h, p(neg), 2, None, 0, 0, 0, NL, None)),
        ("W = 2^31", lambda: L.rto_dose_field(h, p(heavy), 2, None, 0, 0, 0, NL, None)),
        ("m = 0", lambda: L.rto_dose_field(h, p(ok), 2, p(table), 0, 0, 0, NL, None)),
        ("m = 65", lambda: L.rto_dose_field(h, p(ok), 2, p(long), 65, 0, 0, NL, None)),
        ("an entry of 65537", lambda: L.rto_dose_field(h, p(ok), 2, p(over), 2, 0, 0, NL, None)),
        ("unknown falloff", lambda: L.rto_dose_field(h, p(ok), 2, None, 0, 2, 0, NL, None)),
        ("negative falloff", lambda: L.rto_dose_field(h, p(ok), 2, None, 0, -1, 0, NL, None)),
        ("unknown mode", lambda: L.rto_dose_field(h, p(ok), 2, None, 0, 0, 2, NL, None)),
        ("negative mode", lambda: L.rto_dose_field(h, p(ok), 2, None, 0, 0, -1, NL, None)),
        ("reach = 0", lambda: L.rto_dose_field(h, p(ok), 2, None, 0, 0, 0, 0, None)),
        ("reach < 0", lambda: L.rto_dose_field(h, p(ok), 2, None, 0, 0, 0, -7, None)),
        ("a source at x = dimX", lambda: L.rto_dose_field(h, p(outside), 2, None, 0, 0, 0, NL, None)),
        ("a source at y = -1", lambda: L.rto_dose_field(h, p(below), 2, None, 0, 0, 0, NL, None)),
        ("field capacity", lambda: L.rto_download_dose(h, p(small), nvox - 1)),
        ("NULL out", lambda: L.rto_download_dose(h, None, nvox)),
        ("coverage capacity", lambda: L.rto_download_dose_coverage(h, p(cov1), 1)),
        ("NULL coverage", lambda: L.rto_download_dose_coverage(h, None, 2)),
    ]
    for what, call in cases:
        assert call() == hip.RTO_E_INVALID, what
        assert L.rto_last_error(h), what
        assert ctx.download_nodes().tobytes() == nodes.tobytes() and bytes(ctx.info()) == info, what
        assert np.array_equal(ctx.download_voxels(), g.data), what
        assert np.array_equal(ctx.dose(), field) and np.array_equal(ctx.dose_coverage(), cover) and np.array_equal(ctx.exposure(), expo), what
    assert_bit_exact(ctx.render_host(frame), before, "the frame after the refusals")
    # the order of the refusals: of several faults the first in the list is the one reported
    order = [((None, 0, p(over), 99, 9, 9, 0), "sources is NULL"), ((p(outside), 0, p(over), 99, 9, 9, 0), "n is not in"),
             ((p(neg), 2, p(over), 99, 9, 9, 0), "a weight is negative"), ((p(heavy), 2, p(over), 99, 9, 9, 0), "sum to more than"),
             ((p(outside), 2, p(over), 99, 9, 9, 0), "m is not in"), ((p(outside), 2, p(over), 2, 9, 9, 0), "a table entry is above"),
             ((p(outside), 2, p(table), 3, 9, 9, 0), "unknown falloff"), ((p(outside), 2, p(table), 3, 1, 9, 0), "unknown mode"),
             ((p(outside), 2, p(table), 3, 1, 1, 0), "reach is below 1"), ((p(outside), 2, p(table), 3, 1, 1, 1), "source 1 is outside the grid"),
             ((p(below), 2, p(table), 3, 1, 1, 1), "source 0 is outside the grid")]
    for args, text in order:
        assert L.rto_dose_field(h, *args, None) == hip.RTO_E_INVALID and text in L.rto_last_error(h).decode(), (args, L.rto_last_error(h))
    assert np.array_equal(ctx.dose(), field) and np.array_equal(ctx.download_voxels(), g.data)
    assert L.rto_dose_field(h, p(fine), 2, None, 0, 0, 0, 1, None) == 0   # the largest W, no summary asked for, m not read without a table
    assert ctx.last_dose_ms()[2] == -1 and int(ctx.dose().max()) == 2 ** 31 - 1
    # no resident grid, no octree: after the arguments, before the sources' places
    ctx.upload_octree(scenes("sphere64").nodes, g.min, g.voxel_size)
    uploaded = ctx.render_host(frame)
    with pytest.raises(hip.RtoError) as e:
        ctx.dose_field(src)
    assert e.value.code == hip.RTO_E_UNSUPPORTED
    assert L.rto_dose_field(h, p(outside), 2, None, 0, 0, 0, NL, None) == hip.RTO_E_UNSUPPORTED     # the missing grid is reported before the source's place
    assert L.rto_dose_field(h, p(neg), 2, None, 0, 0, 0, NL, None) == hip.RTO_E_INVALID             # a negative weight before the missing grid
    assert_bit_exact(ctx.render_host(frame), uploaded, "the frame after the refusals (uploaded octree)")
    fresh = hip.Context(0)
    try:
        with pytest.raises(hip.RtoError) as e:
            fresh.dose_field(src)
        assert e.value.code == hip.RTO_E_NO_OCTREE
        assert fresh._L.rto_dose_field(fresh._h, p(ok), 2, None, 0, 0, 9, NL, None) == hip.RTO_E_INVALID
        for read in (fresh.dose, fresh.dose_coverage):
            with pytest.raises(hip.RtoError) as e:
                read()
            assert e.value.code == hip.RTO_E_INVALID
    finally:
        fresh.close()
