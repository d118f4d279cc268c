"""The tile wake-up rules of the two work-list kernels, one tile-neighbour direction at a time: the marks of k_geo_seeds and
k_geo_relax (csrc/rto_geodesic.inc) and the stamps of k_skel_step (csrc/rto_skeleton.inc, section 23).

In the random grids and compact shapes of test_geodesic.py and test_skeleton.py every tile is woken many times over by its face
neighbours, so a kernel that forgot an edge or corner tile would pass them.  Here each grid is a few voxels around the centre tile
T of 3 x 3 x 3 tiles, laid out so that one notification, towards one of T's 26 neighbours, is the only way for that neighbour to
learn that its halo has changed (tests/tile_wake_model.py builds them).
CPU: the sequential models of both protocols equal the rule on every directed grid and on four grids of the two suites, and with
each of four omissions they differ from the rule on exactly the directed grids made for that omission: that is what shows that the
grids discriminate, without a broken GPU build.  GPU: field and summary bit for bit against geodesic_ref.field and
skeleton_ref.skeleton on the same grids, with limits, pass limits and 1 and 64 passes per look of the host."""
from __future__ import annotations

import numpy as np
import pytest

import geodesic_ref as gr
import skeleton_ref as sr
import tile_wake_model as tw

CONNS = (gr.CONN_FACE, gr.CONN_FULL)
SOLID = gr.SET_SOLID
DIRECTIONS = tw.DIRECTIONS
FACES = [d for d in DIRECTIONS if sum(map(abs, d)) == 1]
EDGE, CORNER = (-1, 0, 1), (1, -1, -1)                     # the directions of the looks and the pass limits
GEO_CASES = {"route": tw.route_case, "seed": tw.seed_case}


def _id(delta):
    return "".join("-0+"[v + 1] for v in delta)


def _at(field, p):
    return int(field[p[2], p[1], p[0]])


# ================================================================ the cases and the rule's answers, made once and left unchanged
_CASE, _GEO, _SKEL = {}, {}, {}


def _geo_case(kind, dims, delta):
    """(grid, seeds, c, d) of a route or seed case; for kind "detour", delta is the index into tw.DETOURS and c is None."""
    key = (kind, dims, delta)
    if key not in _CASE:
        if kind == "detour":
            g, seeds, target, _ = tw.detour_case(*tw.DETOURS[delta][1:])
            _CASE[key] = (g, seeds, None, target)
        else:
            _CASE[key] = GEO_CASES[kind](dims, delta)
    return _CASE[key]


def _geo_ref(kind, dims, delta, conn):
    key = (kind, dims, delta, conn)
    if key not in _GEO:
        g, seeds, _, _ = _geo_case(kind, dims, delta)
        f = gr.field(g, seeds, SOLID, conn)
        f.setflags(write=False)
        _GEO[key] = f
    return _GEO[key]


def _geo_limits(kind, dims, delta, conn):
    """No limit; for a route case also g(c), at which d must stay out of reach, and g(d) where the rule reaches d at all."""
    if kind != "route":
        return (None,)
    _, _, c, d = _geo_case(kind, dims, delta)
    full = _geo_ref(kind, dims, delta, conn)
    return (None, _at(full, c)) + ((_at(full, d),) if _at(full, d) != gr.NONE else ())


def _all_geo_cases():
    for dims in tw.SIZES:
        for delta in DIRECTIONS:
            for kind in GEO_CASES:
                yield kind, dims, delta
    for i in range(len(tw.DETOURS)):
        yield "detour", tw.SIZES[0], i


def _line_conns(delta):
    return (sr.CONN_FULL, sr.CONN_FACE) if delta in FACES else (sr.CONN_FULL,)


def _skel_case(dims, delta):
    key = ("line", dims, delta)
    if key not in _CASE:
        _CASE[key] = tw.line_case(dims, delta)
    return _CASE[key]


def _skel_ref(dims, delta, conn, max_passes=None):
    key = (dims, delta, conn, max_passes)
    if key not in _SKEL:
        g, anchors, _ = _skel_case(dims, delta)
        k, s = sr.skeleton(g, SOLID, conn, sr.SKEL_TOPOLOGY, anchors, sr.NO_LIMIT if max_passes is None else max_passes)
        k.setflags(write=False)
        _SKEL[key] = (k, s)
    return _SKEL[key]


# ================================================================ CPU: the cases are what they are meant to be
def test_geodesic_cases_by_hand():
    for dims in tw.SIZES:
        for delta in DIRECTIONS:
            g, seeds, c, d = _geo_case("route", dims, delta)
            assert tw.tile_counts(g.shape) == (3, 3, 3) and g.shape == dims[::-1]
            full, face = _geo_ref("route", dims, delta, gr.CONN_FULL), _geo_ref("route", dims, delta, gr.CONN_FACE)
            assert _at(full, d) == _at(full, c) + 2 + sum(map(abs, delta)) and int((full != gr.NONE).sum()) == int(g.sum())
            assert (_at(face, d) != gr.NONE) == (delta in FACES) and _at(face, c) != gr.NONE
            for conn in CONNS:                             # at g(c) the limit keeps d out, at g(d) it lets d in
                limits = _geo_limits("route", dims, delta, conn)
                assert len(limits) == (3 if conn == gr.CONN_FULL or delta in FACES else 2)
                lim = gr.field(g, seeds, SOLID, conn, limits[1])
                assert _at(lim, d) == gr.NONE and _at(lim, c) == limits[1]
                assert len(limits) == 2 or _at(gr.field(g, seeds, SOLID, conn, limits[2]), d) == limits[2]
            g, seeds, c, d = _geo_case("seed", dims, delta)
            assert int(g.sum()) == 3 and seeds.tolist() == [tw.lin(dims, c)]
            assert _at(_geo_ref("seed", dims, delta, gr.CONN_FULL), d) == 2 + sum(map(abs, delta))
    g, seeds, _, target = _geo_case("detour", tw.SIZES[0], 0)   # the first detour, cell by cell, in the plane z = 12
    cells = [(40, y) for y in range(8, 16)] + [(x, 7) for x in range(41, 64)] + [(x, 15) for x in range(40, 65)]
    cells += [(64, y) for y in range(8, 16)] + [(65, 8), (66, 8)]
    want = np.zeros_like(g)
    for x, y in cells:
        want[12, y, x] = 1
    assert np.array_equal(g, want) and seeds.tolist() == [tw.lin(tw.SIZES[0], (40, 12, 12))] and target == (64, 8, 12)
    assert [d[3] for d in (tw.detour_case(*c[1:]) for c in tw.DETOURS)] == [(1, 1, 0), (-1, -1, 0), (1, 0, -1), (0, -1, 1)]
    assert _at(_geo_ref("detour", tw.SIZES[0], 0, gr.CONN_FULL), target) == 86


def test_skeleton_cases_by_hand():
    """The rule eats the line from its free end and reaches c in pass 4 or 5 (the parity of the free end decides which); the anchor
    alone is left after 6 passes.  T'(delta) holds nothing that pass 1 to 3 could remove, so it sleeps until c goes."""
    for dims in tw.SIZES:
        for delta in DIRECTIONS:
            g, anchors, c = _skel_case(dims, delta)
            assert int(g.sum()) == 12 and g.reshape(-1)[anchors].tolist() == [1]
            for conn in _line_conns(delta):
                k, s = _skel_ref(dims, delta, conn)
                assert _at(k, c) in (4, 5) and (int(s["kept"]), int(s["removed"]), int(s["passes"])) == (1, 11, 6)
                assert k.reshape(-1)[anchors[0]] == 0
                far = k[tuple(slice(t * n, t * n + n) for t, n in zip(tw.tile_of(tw.add(c, delta)), tw.TILE[::-1]))]
                assert int((far > 0).sum()) == 3 and int(far[far > 0].min()) >= _at(k, c)


# ================================================================ CPU: the models equal the rule; each omission fails its cases
def test_geodesic_model_equals_the_rule_on_every_directed_case():
    n = 0
    for kind, dims, delta in _all_geo_cases():
        g, seeds, _, _ = _geo_case(kind, dims, delta)
        for conn in CONNS:
            for limit in _geo_limits(kind, dims, delta, conn):
                got, launches, tiles = tw.geodesic_model(g, seeds, SOLID, conn, limit)
                want = gr.threshold(_geo_ref(kind, dims, delta, conn), limit)
                assert np.array_equal(got, want), (kind, dims, delta, conn, limit)
                assert launches >= 2 and tiles >= len({tw.tile_of(p[::-1]) for p in np.argwhere(want != gr.NONE).tolist()})
                n += 1
    assert n == 2 * 2 * 26 * 2 + 2 * (26 + 26 + 26 + 6) + 4 * 2    # no limit; g(c) under both; g(d) under FULL and on FACE's faces; detours


def test_geodesic_omissions_fail_exactly_their_cases():
    """"face_marks" leaves d out of reach in the 20 edge and corner directions of the route cases at both sizes, and the longer way's
    98 (44 in the y-z plane) at the four detours' targets, all under CONN_FULL; under CONN_FACE the kernel marks faces only, so
    there the omission is none.  "seed_own_tile" never reaches d from a seed on the exit voxel: 26 directions at both sizes under
    CONN_FULL, the 6 face directions at both sizes under CONN_FACE.  Neither fails any other case."""
    failed = {o: [] for o in tw.GEO_OMISSIONS}
    for kind, dims, delta in _all_geo_cases():
        g, seeds, _, d = _geo_case(kind, dims, delta)
        for conn in CONNS:
            want = _geo_ref(kind, dims, delta, conn)
            for omit in tw.GEO_OMISSIONS:
                got = tw.geodesic_model(g, seeds, SOLID, conn, omit=omit)[0]
                if not np.array_equal(got, want):
                    assert _at(got, d) > _at(want, d)      # the voxel the case is about is among those that differ
                    failed[omit].append((kind, dims, delta, conn))
    routes = [("route", dims, delta, gr.CONN_FULL) for dims in tw.SIZES for delta in DIRECTIONS if delta not in FACES]
    detours = [("detour", tw.SIZES[0], i, gr.CONN_FULL) for i in range(4)]
    assert len(routes) == 40 and sorted(failed["face_marks"], key=repr) == sorted(routes + detours, key=repr)
    seeded = [("seed", dims, delta, conn) for dims in tw.SIZES for delta in DIRECTIONS for conn in CONNS
              if conn == gr.CONN_FULL or delta in FACES]
    assert len(seeded) == 52 + 12 and sorted(failed["seed_own_tile"], key=repr) == sorted(seeded, key=repr)
    g, seeds, _, target = _geo_case("detour", tw.SIZES[0], 0)
    assert _at(tw.geodesic_model(g, seeds, SOLID, gr.CONN_FULL, omit="face_marks")[0], target) == 98
    # with the limit at g(d) the omission shows as well; at g(c) d is out of reach either way
    for delta in (EDGE, CORNER):
        g, seeds, c, d = _geo_case("route", tw.SIZES[1], delta)
        _, at_c, at_d = _geo_limits("route", tw.SIZES[1], delta, gr.CONN_FULL)
        assert _at(tw.geodesic_model(g, seeds, SOLID, gr.CONN_FULL, at_d, omit="face_marks")[0], d) == gr.NONE
        assert _at(tw.geodesic_model(g, seeds, SOLID, gr.CONN_FULL, at_d)[0], d) == at_d
        assert _at(tw.geodesic_model(g, seeds, SOLID, gr.CONN_FULL, at_c)[0], d) == gr.NONE


def test_skeleton_model_equals_the_rule_on_every_directed_case():
    n = 0
    for dims in tw.SIZES:
        for delta in DIRECTIONS:
            g, anchors, _ = _skel_case(dims, delta)
            for conn in _line_conns(delta):
                for m in (None, 3, 4) if delta in (EDGE, CORNER) else (None,):
                    k, s, tiles = tw.skeleton_model(g, SOLID, conn, sr.SKEL_TOPOLOGY, anchors, sr.NO_LIMIT if m is None else m)
                    want, ws = _skel_ref(dims, delta, conn, m)
                    assert np.array_equal(k, want) and s.tobytes() == ws.tobytes(), (dims, delta, conn, m)
                    assert int(ws["passes"]) == (6 if m is None else m) and tiles >= 8 * 27
                    n += 1
    assert n == 52 + 12 + 2 * 2 * 2


def test_skeleton_omissions_fail_exactly_their_cases():
    """"face_stamps" leaves the voxels of T' standing in the 20 edge and corner directions at both sizes and fails no face direction;
    "sleep_below_pass" fails all 52 lines under CONN_FULL and the 12 face lines under CONN_FACE."""
    failed = {o: [] for o in tw.SKEL_OMISSIONS}
    for dims in tw.SIZES:
        for delta in DIRECTIONS:
            g, anchors, c = _skel_case(dims, delta)
            for conn in _line_conns(delta):
                want, _ = _skel_ref(dims, delta, conn)
                for omit in tw.SKEL_OMISSIONS:
                    k = tw.skeleton_model(g, SOLID, conn, sr.SKEL_TOPOLOGY, anchors, omit=omit)[0]
                    if not np.array_equal(k, want):
                        failed[omit].append((dims, delta, conn))
                        if omit == "face_stamps":          # T removes what the rule removes; T' never hears of it
                            assert _at(k, c) == _at(want, c) and [_at(k, tw.add(c, delta, i)) for i in (1, 2, 3, 4)] == [0, 0, 0, 0]
    diagonal = [(dims, delta, sr.CONN_FULL) for dims in tw.SIZES for delta in DIRECTIONS if delta not in FACES]
    assert len(diagonal) == 40 and sorted(failed["face_stamps"]) == sorted(diagonal)
    every = [(dims, delta, conn) for dims in tw.SIZES for delta in DIRECTIONS for conn in _line_conns(delta)]
    assert len(every) == 52 + 12 and sorted(failed["sleep_below_pass"]) == sorted(every)


def test_models_equal_the_rule_on_grids_of_the_two_suites():
    """Not only on lines: r33 and wide48 of test_geodesic.py, block and torus_corner of test_skeleton.py."""
    import test_geodesic as tg
    import test_skeleton as ts
    for name in ("r33", "wide48"):
        g, seeds = tg._named(name)
        for m in tg.MEDIA:
            for conn in CONNS:
                assert np.array_equal(tw.geodesic_model(g, seeds, m, conn)[0], tg._ref(name, g, seeds, m, conn)), (name, m, conn)
    for name in ("block", "torus_corner"):
        g = ts._named(name)
        for conn, mode in ts.MODES:
            want, ws = ts._ref(name, g, sr.SET_SOLID, conn, mode)
            k, s, _ = tw.skeleton_model(g, sr.SET_SOLID, conn, mode)
            assert np.array_equal(k, want) and s.tobytes() == ws.tobytes(), (name, conn, mode)


def test_survey_of_the_suites_grids_runs_and_reports(capsys):
    """tile_wake_model.survey() (what `python tests/tile_wake_model.py` prints for DESIGN.md sections 20 and 23), on one cheap grid of
    each suite per verdict: wide48 is the one grid of test_geodesic.py that tells "seed_own_tile" from the rule, and only with SOLID;
    "face_marks" and "face_stamps" pass; "sleep_below_pass" is caught where the rule needs a second pass."""
    found = tw.survey(["wide48", "x33"], ["r5x3x2_9", "r33x9x9_7"])
    assert found["face_marks"] == ([], 4) and found["seed_own_tile"] == ([("wide48", gr.SET_SOLID)], 4)
    assert found["face_stamps"] == ([], 12)
    late, n = found["sleep_below_pass"]
    assert n == 12 and ("r5x3x2_9", sr.SET_SOLID, sr.CONN_FACE, sr.SKEL_TOPOLOGY) in late
    assert len([c for c in late if c[0] == "r5x3x2_9"]) == 1 and len([c for c in late if c[0] == "r33x9x9_7"]) == 6
    lines = capsys.readouterr().out.splitlines()
    assert [l.split(":")[0] for l in lines] == ["geodesic face_marks", "geodesic seed_own_tile", "skeleton face_stamps",
                                                "skeleton sleep_below_pass"]
    assert "caught on 0 of 12" in lines[2] and "never on ['r33x9x9_7', 'r5x3x2_9']" in lines[2] and "caught on 7 of 12" in lines[3]


# ================================================================ GPU
gpu = pytest.mark.gpu
GMIN, VOX = np.array([-0.5, -0.5, -0.5], np.float32), np.float32(1.0 / 64)


def _build(ctx, grid):
    from ray_tracing_octrees_amd import hip
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(grid, GMIN, VOX)


def _check_geo(ctx, kind, dims, delta):
    """Builds the case's grid; field and summary for both connectivities and the case's limits.  The fields' bytes."""
    g, seeds, _, _ = _geo_case(kind, dims, delta)
    _build(ctx, g)
    out = []
    for conn in CONNS:
        for limit in _geo_limits(kind, dims, delta, conn):
            want = gr.threshold(_geo_ref(kind, dims, delta, conn), limit)
            what = f"{kind} {dims} {delta} conn {conn} limit {limit}"
            got, gs = ctx.geodesic_field(seeds, SOLID, conn, limit)
            assert got.dtype == np.int32 and got.shape == g.shape, what
            assert np.array_equal(got, want), f"{what}: differ at (z, y, x) {np.argwhere(got != want)[:8].tolist()}"
            assert gs.tobytes() == gr.summary(want).tobytes(), (what, gs)
            passes, tiles = ctx.geodesic_passes(tiles=True)
            holding = len({tw.tile_of(p[::-1]) for p in np.argwhere(want != gr.NONE).tolist()})
            assert 2 <= passes <= g.size + 2 and tiles >= holding, (what, passes, tiles, holding)
            out.append(got.tobytes() + gs.tobytes())
    return out


@gpu
@pytest.mark.parametrize("delta", DIRECTIONS, ids=_id)
def test_gpu_geodesic_marks_reach_the_tile_towards(ctx, delta):
    """Route (k_geo_relax's marks) and seed on the exit voxel (k_geo_seeds' marks), both sizes (the 16-byte and the byte loads), both
    connectivities, with no limit, the limit at g(c) and the limit at g(d)."""
    for dims in tw.SIZES:
        for kind in GEO_CASES:
            _check_geo(ctx, kind, dims, delta)


@gpu
def test_gpu_geodesic_shorter_route_one_launch_later_through_a_tile_edge(ctx):
    """The detours.  On the card they are the weaker pin: the tile that carries the short way and the tile that holds the target both
    run in the second launch, and a halo value read there may already be the newer one, so a kernel without the diagonal mark can
    still end at the rule's value by the order its workgroups happen to run in.  The route, seed and line cases leave no such
    chance: there the woken tile has nothing to read before the mark or stamp under test is made."""
    for i in range(len(tw.DETOURS)):
        _check_geo(ctx, "detour", tw.SIZES[0], i)


@gpu
def test_gpu_geodesic_looks_change_no_byte(ctx):
    """One corner and one edge direction of the route and seed cases and the detours, with the host looking at the device after every
    launch and after every 64."""
    cases = [(kind, dims, delta) for dims in tw.SIZES for delta in (CORNER, EDGE) for kind in GEO_CASES]
    cases += [("detour", tw.SIZES[0], i) for i in range(len(tw.DETOURS))]
    try:
        for case in cases:
            seen = []
            for look in (1, 64):
                ctx.debug_set_geodesic_look(look)
                seen.append(_check_geo(ctx, *case))
            assert seen[0] == seen[1], case
    finally:
        ctx.debug_set_geodesic_look(8)


def _check_skel(ctx, dims, delta, conn, max_passes=None):
    """The grid of the line is resident; field and summary against the rule.  The field's bytes."""
    g, anchors, _ = _skel_case(dims, delta)
    want, ws = _skel_ref(dims, delta, conn, max_passes)
    what = f"line {dims} {delta} conn {conn} max_passes {max_passes}"
    got, gs = ctx.skeleton_field(SOLID, conn, sr.SKEL_TOPOLOGY, anchors, max_passes)
    assert got.dtype == np.int32 and got.shape == g.shape, what
    assert np.array_equal(got, want), f"{what}: differ at (z, y, x) {np.argwhere(got != want)[:8].tolist()}"
    assert gs.tobytes() == ws.tobytes(), (what, gs, ws)
    launches, tiles = ctx.skeleton_passes()
    ran = int(ws["passes"]) + (0 if max_passes is not None else 1)
    assert launches % 9 == 0 and launches >= 9 * ran and tiles >= 8 * 27, (what, launches, tiles)
    return got.tobytes() + gs.tobytes()


@gpu
@pytest.mark.parametrize("delta", DIRECTIONS, ids=_id)
def test_gpu_skeleton_stamps_reach_the_tile_towards(ctx, delta):
    """The line through the seam, both sizes, CONN_FULL; the 6 face directions under CONN_FACE as well."""
    for dims in tw.SIZES:
        _build(ctx, _skel_case(dims, delta)[0])
        for conn in _line_conns(delta):
            _check_skel(ctx, dims, delta, conn)


@gpu
def test_gpu_skeleton_pass_limits_and_looks_change_no_byte(ctx):
    """One corner and one edge direction: max_passes 3 and 4 against the rule with the same limit; no limit with 1 and 64 passes per
    look of the host."""
    try:
        for dims in tw.SIZES:
            for delta in (CORNER, EDGE):
                _build(ctx, _skel_case(dims, delta)[0])
                for m in (3, 4):
                    _check_skel(ctx, dims, delta, sr.CONN_FULL, m)
                seen = []
                for look in (1, 64):
                    ctx.debug_set_skeleton_look(look)
                    seen.append(_check_skel(ctx, dims, delta, sr.CONN_FULL))
                assert seen[0] == seen[1], (dims, delta)
    finally:
        ctx.debug_set_skeleton_look(8)
