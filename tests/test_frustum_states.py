"""Every entry point's rule under a frustum update in force ("Entry points under a frustum update";
tests/frustum_states.py holds the states and scenes).  include/rto_hip.h says of each entry whether it honours the update (the box
renders, the closest-hit render, the ray-skip family with use_visibility), refuses it (rto_render_triangles_*), ignores it (the
queries, the lit renders, field views, projections, mesh extraction) or resets it (edits that change the grid).  CPU: the states
are what their names say and can tell the rules apart, on the oracle alone.  GPU: the ignoring entries give the bytes they give
with culling off, in every state, before and after the survivors are counted, and those bytes are the feature's own statement;
the honouring entries give the oracle's bytes over the reference's compacted array; the refusal changes nothing; an edit leaves
culling off.  Every comparison is bitwise."""
from __future__ import annotations

import numpy as np
import pytest

import field_view_ref as fr
import frustum_states as fs
import lit_ref as lr
import mesh_ref as mr
import projection_ref as pr
import query_ref as q
import span_ref as sp
import tri_lit_ref as tl
import tri_query_ref as tq

gpu = pytest.mark.gpu
MODES = (q.FIRST, q.CLOSEST, q.ANY)
BACKGROUND = np.array([0.0, 0.0, 0.0, 1.0], np.float32)        # a miss of every render here (include/rto_hip.h: "a miss is (0, 0, 0, 1)")
REFUSAL = "render_triangles: not available while frustum culling is active"
_SCENES: dict = {}


# ================================================================ scenes, states, the oracle's side
class _Scene:
    """One scene of frustum_states.SCENES on the oracle's side: grid (None for D), nodes, origin, voxel, the planes of its states,
    its camera, and what the reference's loop leaves of it in each state."""

    def __init__(self, orc, name):
        kind, arg = fs.SCENES[name]
        self.name, self.grid, self.rootless = name, None, None
        if kind == "sphere":
            self.grid = orc.test_sphere_grid(arg)
        elif kind == "rootless16":
            rng = np.random.default_rng(fs.SEARCH_SEED)
            gmin, vs, a, _, child_mx = fs.search_origin(np, rng, 16, arg)
            self.grid = orc.Grid((16, 16, 16), gmin, vs, fs.rootless16_data(np, rng, a, arg))
            self.rootless = (a, child_mx)
        elif kind == "checker":
            gmin, vs, a, _, child_mx = fs.search_origin(np, np.random.default_rng(fs.C_SEARCH_SEED), arg, "solid leaf")
            k, j, i = np.mgrid[0:arg, 0:arg, 0:arg]
            self.grid = orc.Grid((arg, arg, arg), gmin, vs, ((i + j + k) % 2 == 0).astype(np.uint8))
            self.rootless = (a, child_mx)
        if kind == "compacted":
            base = scene(orc, arg)
            self.min, self.voxel, self.dim = base.min, base.voxel, base.dim
            self.nodes, _ = orc.cull_compact_planes(base.nodes, base.min, base.voxel, np.array(fs.D_SOURCE_PLANES, np.float32), 0.0)
        else:
            self.min, self.voxel, self.dim = self.grid.min, self.grid.voxel_size, int(max(self.grid.dims))
            self.nodes = orc.build_flat_octree(self.grid)
        self.edge = float(np.float32(self.dim) * self.voxel)
        self.planes = {"HALF": np.array(fs.half_planes(name, float(self.min[0]), self.edge), np.float32),
                       "NONE": np.array(fs.NONE_PLANES, np.float32)}
        if self.rootless:
            self.planes["ROOTLESS"] = np.array(fs.rootless_planes(*self.rootless), np.float32)
        cam = orc.Camera(fs.CAMERA[0], fs.CAMERA[1], fs.CAMERA[2] * self.edge)
        cam.set_target(*[float(x) for x in (self.min + np.float32(0.5 * self.edge))])
        self.view, self.pos = cam.get_view(), cam.get_pos()
        self._culled, self._tree, self._rays, self._tris = {}, None, None, None

    def states(self):
        return fs.states_of(self.name)

    def culled(self, orc, state):
        """(the reference's compacted array, its visibility flags) in `state`."""
        if state not in self._culled:
            if state == "OFF":
                self._culled[state] = (self.nodes, np.ones(len(self.nodes), bool))
            else:
                self._culled[state] = orc.cull_compact_planes(self.nodes, self.min, self.voxel, self.planes[state], 0.0)
        return self._culled[state]

    def tree(self):
        if self._tree is None:
            self._tree = q.Tree32(self.nodes, self.min, self.voxel)
        return self._tree

    def rays(self):
        if self._rays is None:
            self._rays = q.seeded_rays(self.tree(), fs.RAYS, fs.RAY_SEED)
        return self._rays

    def triangles(self, orc):
        if self._tris is None:
            tris, off = orc.build_leaf_triangles(self.grid, self.nodes)
            self._tris = (np.asarray(tris, np.float32).reshape(-1, 12), np.asarray(off, np.int32))
        return self._tris


def scene(orc, name) -> _Scene:
    if name not in _SCENES:
        _SCENES[name] = _Scene(orc, name)
    return _SCENES[name]


def _pixel_rays(orc, s, W, H):
    return orc.generate_rays(s.view, s.pos, W / H, fs.FOV, W, H).reshape(-1, 3)


def _all_pixels(W, H):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([xx.ravel(), yy.ravel()], 1).astype(np.int32)


def _oracle_frame(orc, s, state, W, H):
    """(frame, stats) of the reference's culled render in `state`: orc.render over the compacted array; nothing survives: the
    dispatch over an empty array is a frame of misses."""
    compact, _ = s.culled(orc, state)
    if len(compact) == 0:
        return np.broadcast_to(BACKGROUND, (H, W, 4)).copy(), None
    return orc.render(compact, s.min, s.voxel, s.view, s.pos, W / H, fs.FOV, W, H)


def _changed_pixels(a, b):
    return int((a.view(np.uint32) != b.view(np.uint32)).any(-1).sum())


# ================================================================ CPU: the states can tell the rules apart
ALL_STATES = [(n, st) for n in fs.SCENES for st in fs.states_of(n) if st != "OFF"]


def test_the_tables_cover_the_issue():
    """The data file: every scene has HALF and NONE, ROOTLESS exactly where a rounding origin was searched for; frames of whole and
    of partial 8 x 8 tiles."""
    assert set(fs.SCENES) == {"A", "B-leaf", "B-internal", "C", "D"}
    assert set(fs.ROOTLESS_SCENES) == {n for n, (kind, _) in fs.SCENES.items() if kind in ("rootless16", "checker")}
    assert all(fs.states_of(n)[:3] == ("OFF", "HALF", "NONE") for n in fs.SCENES)
    assert any(W % 8 == 0 and H % 8 == 0 for W, H in fs.FRAMES) and any(W % 8 and H % 8 for W, H in fs.FRAMES)


@pytest.mark.parametrize("first_survivor", ["solid leaf", "internal node"])
def test_the_search_finds_the_rounding_difference(first_survivor):
    """search_origin at dim 16 under the seed of test_culled_root_with_surviving_descendants_follows_the_reference: the child's
    max plane lies above the root's, by float rounding alone."""
    gmin, vs, a, root_mx, plane = fs.search_origin(np, np.random.default_rng(fs.SEARCH_SEED), 16, first_survivor)
    assert plane > root_mx and float(plane) - float(root_mx) <= 2 * float(np.spacing(root_mx))
    assert float(gmin[a]) + 16 * float(vs) == pytest.approx(float(root_mx), rel=1e-6)


def test_scene_c_is_past_both_single_round_limits(orc):
    """The 128^3 checkerboard: more than 256 workgroups of k_cull_desc (256 internal nodes each), so the last block's reduction
    takes a second round, and more than 1,024 blocks of 256 flags, so the on-demand count's scan does."""
    s = scene(orc, "C")
    n, internal = len(s.nodes), int((s.nodes["isLeaf"] == 0).sum())
    assert (n, internal) == (2396745, 299593)
    assert -(-internal // 256) == 1171 > 256 and -(-n // 256) == 9363 > 1024
    assert s.nodes.nbytes > 140e6


def test_scene_d_is_about_half_of_sphere64(orc):
    a, d = scene(orc, "A"), scene(orc, "D")
    assert 0.4 * len(a.nodes) < len(d.nodes) < 0.6 * len(a.nodes)
    assert (d.nodes["child"] == -1).any() and d.nodes[0]["size"] == 64


@pytest.mark.parametrize("name,state", ALL_STATES)
def test_states_are_what_their_names_say(orc, name, state):
    s = scene(orc, name)
    compact, vis = s.culled(orc, state)
    n, visible = len(s.nodes), int(vis.sum())
    assert len(compact) == visible
    if state == "HALF":
        assert vis[0] and 0 < visible < n / 2
        assert name != "A" or (visible, n) == (421, 23561)          # the planes the query suites use
    elif state == "NONE":
        assert visible == 0
    else:
        assert not vis[0] and visible > 0


@pytest.mark.parametrize("name,state", [(n, st) for n, st in ALL_STATES if n != "C"])
@pytest.mark.parametrize("W,H", fs.FRAMES)
def test_oracle_frames_tell_the_states_apart(orc, name, state, W, H):
    """The reference's culled frame differs from the frame with culling off in at least 1 % of the pixels: an entry that wrongly
    honoured or wrongly ignored the state would render other bytes.  NONE: all background; ROOTLESS: something is hit."""
    s = scene(orc, name)
    full, st_full = _oracle_frame(orc, s, "OFF", W, H)
    img, st = _oracle_frame(orc, s, state, W, H)
    assert st_full["hits"] >= 0.1 * W * H
    assert _changed_pixels(img, full) >= fs.MIN_CHANGED_PIXELS * W * H
    if state == "NONE":
        assert (img == BACKGROUND).all()
    if state == "ROOTLESS":
        assert st["hits"] > 0


@pytest.mark.parametrize("state", ["HALF", "NONE", "ROOTLESS"])
def test_oracle_frames_tell_the_states_apart_on_scene_c(orc, state):
    """Scene C's one frame per state.  ROOTLESS here keeps the root's far children and what sticks out with them; whether a ray
    finds a leaf through that array is the oracle's to say, so only the difference from OFF is required."""
    s = scene(orc, "C")
    W, H = fs.BIG_FRAME
    full, st_full = _oracle_frame(orc, s, "OFF", W, H)
    img, _ = _oracle_frame(orc, s, state, W, H)
    assert st_full["hits"] >= 0.1 * W * H
    assert _changed_pixels(img, full) >= fs.MIN_CHANGED_PIXELS * W * H


@pytest.mark.parametrize("name", fs.FRAME_SCENES)
def test_a_quarter_of_the_hitting_rays_end_in_a_culled_leaf(orc, name):
    """Of the seeded rays and of the pixel rays that hit with culling off (the box queries' and the spans' rays), at least a quarter
    hit a leaf HALF culls: an ignoring entry that consulted the flags would lose them."""
    s = scene(orc, name)
    _, vis = s.culled(orc, "HALF")
    o, d, tmn, tmx = s.rays()
    W, H = fs.FRAMES[0]
    for what, rec in (("seeded", q.query32(s.tree(), o, d, tmn, tmx)), ("pixels", q.query32(s.tree(), s.pos, _pixel_rays(orc, s, W, H)))):
        for m in (q.FIRST, q.CLOSEST):
            leaf = rec[m]["node"][rec[m]["node"] >= 0]
            assert len(leaf) >= 100, (what, m, len(leaf))
            assert (~vis[leaf]).mean() >= fs.MIN_CULLED_HITS, (what, m, (~vis[leaf]).mean())
    span = sp.span32(s.tree(), o, d, tmn, tmx)
    leaf = span["node"][span["leaves"] > 0]
    assert len(leaf) >= 100 and (~vis[leaf]).mean() >= fs.MIN_CULLED_HITS


# ================================================================ GPU: helpers
def _rto():
    import ray_tracing_octrees_amd as rto
    return rto


def _hip():
    from ray_tracing_octrees_amd import hip
    return hip


def _frame(s, W, H):
    return _hip().make_frame(s.view, s.pos, W / H, fs.FOV, W, H)


def _resident(ctx, s):
    """The scene on the context, culling off: scenes with a grid through rto_build_octree (the grid stays resident), D uploaded."""
    hip = _hip()
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.debug_set_frustum_shortcut(True)
    if s.grid is not None and s.name in fs.GRID_SCENES:
        ctx.build_octree(s.grid.data, s.min, s.voxel)
        assert ctx.download_nodes().tobytes() == s.nodes.tobytes()
    else:
        ctx.upload_octree(s.nodes, s.min, s.voxel)
    info = ctx.info()
    assert info.canonical == (0 if s.name == "D" else 1) and info.culling_active == 0 and info.num_nodes == len(s.nodes)


def _set_state(ctx, s, state):
    if state == "OFF":
        ctx.update_frustum(s.view, fs.FOV, 1.0, enable=False)
    else:
        ctx.debug_update_frustum_planes(s.planes[state], 0.0)


def _restore(ctx):
    """What every test here leaves behind on the session's context."""
    hip = _hip()
    if ctx.info().num_nodes > 0:
        ctx.update_frustum(np.eye(4, dtype=np.float32).reshape(16), fs.FOV, 1.0, enable=False)
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.debug_set_frustum_shortcut(True)
    ctx.debug_set_projection_table(True)


def _blobs(outputs):
    """{label: bytes} of an entry's outputs ({label: array, record or None})."""
    return {k: (None if v is None else np.ascontiguousarray(v).tobytes()) for k, v in outputs.items()}


def _same_bytes(got, want, what):
    assert got.keys() == want.keys(), what
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, f"{what}: {len(bad)} of {len(want)} outputs differ from the call with culling off: {bad[:6]}"


def _ignoring(ctx, orc, s, call, statement):
    """`call` in every state of the scene against its own bytes with culling off: directly after the update (on canonical trees the
    survivors are not counted yet), again once rto_octree_info_get has fetched the count, and after culling is switched off
    again.  `statement(outputs)` checks the bytes with culling off against the feature's reference, once."""
    differing = []

    def same(what):
        got = _blobs(call())
        assert got.keys() == off.keys(), what
        bad = [k for k in off if got[k] != off[k]]
        if bad:
            differing.append(f"{what}: {len(bad)} of {len(off)} outputs, e.g. {bad[:3]}")

    try:
        first = call()
        statement(first)
        off = _blobs(first)
        for state in s.states()[1:]:
            visible = int(s.culled(orc, state)[1].sum())
            _set_state(ctx, s, state)
            same(f"{state}, survivors not counted yet")
            info = ctx.info()
            assert info.culling_active == 1 and info.visible_nodes == visible, (state, info.visible_nodes, visible)
            same(f"{state}, survivors counted")
            _set_state(ctx, s, "OFF")
            info = ctx.info()
            assert info.culling_active == 0 and info.visible_nodes == len(s.nodes)
            same(f"OFF_AGAIN after {state}")
        assert not differing, f"{s.name}: outputs differ from the call with culling off in {len(differing)} runs: " + "; ".join(differing)
    finally:
        _restore(ctx)


def _records_equal(got, want, key, what, mask_only=False):
    """32-byte records, field by field bitwise; mask_only: the hit / miss mask alone (ANY's leaf or triangle is unspecified)."""
    assert len(got) == len(want), what
    bad = np.nonzero((got[key] >= 0) != (want[key] >= 0))[0]
    assert not len(bad), f"{what}: {len(bad)} rays differ in hit / miss, e.g. {bad[:5]}"
    if not mask_only:
        neq = (got.view(np.int32).reshape(-1, 8) != want.view(np.int32).reshape(-1, 8)).any(1)
        assert not neq.any(), f"{what}: {int(neq.sum())} records differ from the statement, e.g. rays {np.nonzero(neq)[0][:5]}"


def _lighting(s):
    return dict(fs.LIGHT, ao_radius=float(np.float32(fs.AO_RADIUS_VOXELS * float(s.voxel))))


def _lut():
    return _hip().ramp_lut([(0, 0, 96, 255), (0, 200, 255, 255), (255, 255, 0, 200), (255, 32, 0, 255)])


def _clip(s):
    d = s.dim
    return ((d // 8, 0, d // 8), (d - d // 8, d - d // 4, d))


# ================================================================ GPU: the entries that ignore the update
IGNORING_SCENES = list(fs.FRAME_SCENES)


@gpu
@pytest.mark.parametrize("name", IGNORING_SCENES)
def test_box_queries_ignore_the_state(ctx, orc, name):
    """rto_query_rays_* and rto_query_pixels_*, the three modes: the records with culling off, which are query_ref's."""
    s = scene(orc, name)
    o, d, tmn, tmx = s.rays()
    _resident(ctx, s)

    def call():
        out = {}
        for m in MODES:
            out[f"rays mode {m}"] = ctx.query_rays(o, d, tmn, tmx, m)
            for W, H in fs.FRAMES:
                out[f"pixels {W}x{H} mode {m}"] = ctx.query_pixels(_frame(s, W, H), _all_pixels(W, H), m)
        return out

    def statement(out):
        want = q.query32(s.tree(), o, d, tmn, tmx)
        for m in MODES:
            _records_equal(out[f"rays mode {m}"], want[m], "node", f"{name} rays mode {m}", mask_only=(m == q.ANY))
            for W, H in fs.FRAMES:
                px = q.query32(s.tree(), s.pos, _pixel_rays(orc, s, W, H))
                _records_equal(out[f"pixels {W}x{H} mode {m}"], px[m], "node", f"{name} pixels {W}x{H} mode {m}", mask_only=(m == q.ANY))
        assert (want[q.CLOSEST]["node"] >= 0).sum() >= 100

    _ignoring(ctx, orc, s, call, statement)


@gpu
@pytest.mark.parametrize("name", IGNORING_SCENES)
def test_span_queries_ignore_the_state(ctx, orc, name):
    """rto_query_spans_* and rto_query_span_pixels_*: the records with culling off, which are span_ref's."""
    s = scene(orc, name)
    o, d, tmn, tmx = s.rays()
    _resident(ctx, s)

    def call():
        out = {"rays": ctx.query_spans(o, d, tmn, tmx)}
        for W, H in fs.FRAMES:
            out[f"pixels {W}x{H}"] = ctx.query_span_pixels(_frame(s, W, H), _all_pixels(W, H))
        return out

    def statement(out):
        want = sp.span32(s.tree(), o, d, tmn, tmx)
        assert out["rays"].tobytes() == want.tobytes(), f"{name}: span records differ from span_ref"
        assert (want["leaves"] > 1).sum() >= 50
        for W, H in fs.FRAMES:
            px = sp.span32(s.tree(), s.pos, _pixel_rays(orc, s, W, H))
            assert out[f"pixels {W}x{H}"].tobytes() == px.tobytes(), f"{name} {W}x{H}: pixel spans differ from span_ref"

    _ignoring(ctx, orc, s, call, statement)


@gpu
@pytest.mark.parametrize("name", fs.GRID_SCENES)
def test_triangle_queries_ignore_the_state(ctx, orc, name):
    """rto_query_triangles_* and rto_query_triangle_pixels_*, the three modes, on the triangles rto_build_leaf_triangles(NULL)
    makes: the records with culling off, which are tri_query_ref's on the oracle's triangles."""
    s = scene(orc, name)
    o, d, tmn, tmx = s.rays()
    rays = _hip().make_rays(o, d, tmn, tmx)
    tris, off = s.triangles(orc)
    _resident(ctx, s)
    ctx.build_leaf_triangles(None)

    def call():
        out = {}
        for m in MODES:
            out[f"rays mode {m}"] = ctx.query_triangle_records(rays, m)
            for W, H in fs.FRAMES:
                out[f"pixels {W}x{H} mode {m}"] = ctx.query_triangle_pixels(_frame(s, W, H), _all_pixels(W, H), m)
        return out

    def statement(out):
        want = tq.query_tri32(s.tree(), tris, off, o, d, tmn, tmx)
        for m in MODES:
            _records_equal(out[f"rays mode {m}"], want[m], "tri", f"{name} rays mode {m}", mask_only=(m == tq.ANY))
            for W, H in fs.FRAMES:
                rd = _pixel_rays(orc, s, W, H)
                px = tq.query_tri32(s.tree(), tris, off, np.broadcast_to(s.pos, rd.shape), rd)
                _records_equal(out[f"pixels {W}x{H} mode {m}"], px[m], "tri", f"{name} pixels {W}x{H} mode {m}", mask_only=(m == tq.ANY))
        assert (want[tq.CLOSEST]["tri"] >= 0).sum() >= 100

    _ignoring(ctx, orc, s, call, statement)


@gpu
@pytest.mark.parametrize("name", fs.GRID_SCENES)
def test_lit_render_ignores_the_state(ctx, orc, name):
    """rto_render_lit_*: shadow ray, four AO rays, the visibility buffer: the frame with culling off, which is lit_ref's."""
    s = scene(orc, name)
    L = _lighting(s)
    _resident(ctx, s)

    def call():
        out = {}
        for W, H in fs.FRAMES:
            out[f"rgba {W}x{H}"], out[f"vis {W}x{H}"] = ctx.render_lit_host(_frame(s, W, H), _hip().make_lighting(**L), vis=True)
        return out

    def statement(out):
        for W, H in fs.FRAMES:
            want, wvis = lr.lit_frame(s.tree(), s.voxel, s.pos, _pixel_rays(orc, s, W, H), W, H, _hip().ao_directions(),
                                      light_dir=L["light_dir"], shadow=1, K=L["ao_samples"], radius=L["ao_radius"], seed=L["seed"])
            assert out[f"rgba {W}x{H}"].tobytes() == want.tobytes(), f"{name} {W}x{H}: the lit frame differs from lit_ref"
            assert np.array_equal(out[f"vis {W}x{H}"], wvis), f"{name} {W}x{H}: the visibility differs from lit_ref"
            assert (wvis >= 256).any() and ((wvis & 255) > 0).any() and (wvis == -1).any()

    _ignoring(ctx, orc, s, call, statement)


@gpu
def test_lit_render_refuses_a_noncanonical_array_in_every_state(ctx, orc):
    """Scene D has no descriptor tree: rto_render_lit_* is RTO_E_UNSUPPORTED there (include/rto_hip.h), and the frustum state has
    no say in that either."""
    hip = _hip()
    s = scene(orc, "D")
    _resident(ctx, s)
    try:
        for state in s.states() + ("OFF",):
            _set_state(ctx, s, state)
            with pytest.raises(hip.RtoError) as e:
                ctx.render_lit_host(_frame(s, *fs.FRAMES[0]), hip.make_lighting(**_lighting(s)), vis=True)
            assert e.value.code == hip.RTO_E_UNSUPPORTED, state
    finally:
        _restore(ctx)


@gpu
@pytest.mark.parametrize("name", fs.GRID_SCENES)
def test_triangle_lit_render_ignores_the_state(ctx, orc, name):
    """rto_render_lit_triangles_*, the same settings: the frame with culling off, which is tri_lit_ref's on the oracle's triangles."""
    s = scene(orc, name)
    L = _lighting(s)
    tris, off = s.triangles(orc)
    _resident(ctx, s)
    ctx.build_leaf_triangles(None)

    def call():
        out = {}
        for W, H in fs.FRAMES:
            out[f"rgba {W}x{H}"], out[f"vis {W}x{H}"] = ctx.render_lit_triangles_host(_frame(s, W, H), _hip().make_lighting(**L), vis=True)
        return out

    def statement(out):
        for W, H in fs.FRAMES:
            want, wvis = tl.tri_lit_frame(s.tree(), tris, off, s.voxel, s.pos, _pixel_rays(orc, s, W, H), W, H, _hip().ao_directions(),
                                          light_dir=L["light_dir"], shadow=1, K=L["ao_samples"], radius=L["ao_radius"], seed=L["seed"])
            assert out[f"rgba {W}x{H}"].tobytes() == want.tobytes(), f"{name} {W}x{H}: the lit triangle frame differs from tri_lit_ref"
            assert np.array_equal(out[f"vis {W}x{H}"], wvis), f"{name} {W}x{H}: the visibility differs from tri_lit_ref"
            assert (wvis >= 0).sum() >= 100

    _ignoring(ctx, orc, s, call, statement)


def _field_views(s):
    hip = _hip()
    kw = dict(none_rgba=(0.5, 0.25, 0.125, 0.75), miss_rgba=(0.0, 0.125, 0.25, 1.0), scale=hip.SCALE_SQRT)
    return {"hit first": hip.make_field_view(hip.FIELD_DISTANCE, sample=hip.SAMPLE_HIT, mode=hip.QUERY_FIRST, shade=True, **kw),
            "front closest": hip.make_field_view(hip.FIELD_DISTANCE, sample=hip.SAMPLE_FRONT, mode=hip.QUERY_CLOSEST, valid=(0, 0x7ffffffe), **kw),
            "hit closest clipped": hip.make_field_view(hip.FIELD_DISTANCE, sample=hip.SAMPLE_HIT, mode=hip.QUERY_CLOSEST, clip=_clip(s), **kw),
            "front first clipped": hip.make_field_view(hip.FIELD_DISTANCE, sample=hip.SAMPLE_FRONT, mode=hip.QUERY_FIRST, clip=_clip(s),
                                                       shade=True, **kw)}


@gpu
@pytest.mark.parametrize("name", fs.GRID_SCENES)
def test_field_views_ignore_the_state(ctx, orc, name):
    """rto_render_field_* of the resident distance field (to EMPTY): the hit and the front sample, FIRST and CLOSEST, with and
    without a clip box: rgba, values, summary and bins with culling off, which are field_view_ref's."""
    hip = _hip()
    s = scene(orc, name)
    views = _field_views(s)
    _resident(ctx, s)
    vol = ctx.distance_field(hip.SET_EMPTY)[0]

    def call():
        out = {}
        for vname, v in views.items():
            for W, H in fs.FRAMES:
                got = ctx.render_field_host(_frame(s, W, H), v, _lut())
                out.update({f"{vname} {W}x{H} {k}": x for k, x in zip(("rgba", "values", "summary", "bins"), got)})
        return out

    def statement(out):
        valued = 0
        for vname, v in views.items():
            for W, H in fs.FRAMES:
                want = fr.frame(s.tree(), s.min, s.voxel, s.pos, _pixel_rays(orc, s, W, H), W, H, vol, v, _lut())
                for k, w in zip(("rgba", "values", "summary", "bins"), want):
                    assert np.ascontiguousarray(out[f"{vname} {W}x{H} {k}"]).tobytes() == np.ascontiguousarray(w).tobytes(), \
                        f"{name} {vname} {W}x{H}: {k} differs from field_view_ref"
                valued += int(want[2]["valued"])
        assert valued >= 100

    _ignoring(ctx, orc, s, call, statement)


@gpu
@pytest.mark.parametrize("name", fs.GRID_SCENES)
def test_field_projections_ignore_the_state(ctx, orc, name):
    """rto_project_field_* of the same field: MAX and FIRST, with the brick table and without: all seven outputs with culling off,
    which are projection_ref's (checked on the frame of partial tiles)."""
    hip = _hip()
    s = scene(orc, name)
    projs = {"MAX": hip.make_field_projection(hip.FIELD_DISTANCE, op=hip.PROJECT_MAX, scale=hip.SCALE_SQRT, valid=(1, 0x7ffffffe)),
             "FIRST": hip.make_field_projection(hip.FIELD_DISTANCE, op=hip.PROJECT_FIRST, valid=(1, 0x7ffffffe), clip=_clip(s))}
    names = ("rgba", "values", "voxels", "sums", "counts", "summary", "bins")
    _resident(ctx, s)
    vol = ctx.distance_field(hip.SET_EMPTY)[0]

    def call():
        out = {}
        for table in (True, False):
            ctx.debug_set_projection_table(table)
            for pname, p in projs.items():
                for W, H in fs.FRAMES:
                    got = ctx.project_field_host(_frame(s, W, H), p, _lut())
                    out.update({f"{pname} table {table} {W}x{H} {k}": x for k, x in zip(names, got)})
        ctx.debug_set_projection_table(True)
        return out

    def statement(out):
        W, H = fs.FRAMES[1]
        rd = _pixel_rays(orc, s, W, H)
        for pname, p in projs.items():
            want = pr.frame(s.min, s.voxel, s.pos, rd, W, H, vol, p, _lut())
            assert want[5]["valued"] >= 100
            for table in (True, False):
                for k, w in zip(names, want):
                    assert np.ascontiguousarray(out[f"{pname} table {table} {W}x{H} {k}"]).tobytes() == np.ascontiguousarray(w).tobytes(), \
                        f"{name} {pname} table {table}: {k} differs from projection_ref"

    _ignoring(ctx, orc, s, call, statement)


@gpu
@pytest.mark.parametrize("name", fs.GRID_SCENES)
def test_mesh_extraction_ignores_the_state(ctx, orc, name):
    """rto_extract_mesh, both kinds, without planes and with planes of its own (x below the box's centre plus a tenth of its edge,
    margin 0): the lists with culling off, which are mesh_ref's."""
    hip = _hip()
    s = scene(orc, name)
    tris, off = s.triangles(orc)
    c, e = s.min.astype(np.float64) + 0.5 * s.edge, s.edge
    own = np.array([[-1, 0, 0, c[0] + 0.1 * e], [1, 0, 0, 2 * e - c[0]], [0, -1, 0, c[1] + 2 * e], [0, 1, 0, 2 * e - c[1]],
                    [0, 0, -1, c[2] + 2 * e], [0, 0, 1, 2 * e - c[2]]], np.float32)
    sets = {"no planes": (None, 50.0), "own planes": (own, 0.0)}
    _resident(ctx, s)
    ctx.build_leaf_triangles(None)

    def call():
        out = {}
        for kind in (hip.MESH_MC, hip.MESH_CUBES):
            for sname, (planes, margin) in sets.items():
                out[f"kind {kind} {sname} tris"], out[f"kind {kind} {sname} nodes"] = ctx.extract_mesh(kind, planes, margin)
        return out

    def statement(out):
        for kind in (hip.MESH_MC, hip.MESH_CUBES):
            sizes = []
            for sname, (planes, margin) in sets.items():
                want, wnode = mr.extract(kind, s.nodes, s.min, s.voxel, data=s.grid.data, tris=tris, tri_offset=off, planes=planes, margin=margin)
                assert out[f"kind {kind} {sname} tris"].tobytes() == want.tobytes(), f"{name} kind {kind} {sname}: triangles differ from mesh_ref"
                assert out[f"kind {kind} {sname} nodes"].tobytes() == wnode.tobytes(), f"{name} kind {kind} {sname}: owners differ from mesh_ref"
                sizes.append(len(want))
            assert 0 < sizes[1] < sizes[0], sizes                  # the call's own planes do cull

    _ignoring(ctx, orc, s, call, statement)


@gpu
@pytest.mark.parametrize("name", fs.GRID_SCENES)
def test_grid_queries_are_a_control(ctx, orc, name):
    """rto_query_points_*, _regions_* and _nearest_* read the grid alone: one call each, against their own bytes with culling off."""
    hip = _hip()
    s = scene(orc, name)
    rng = np.random.default_rng(5)
    pts = (s.min + rng.random((256, 3)).astype(np.float32) * np.float32(s.edge)).astype(np.float32)
    brushes = hip.make_brushes(pts[:64], np.float32(0.1 * s.edge), hip.BRUSH_SPHERE, hip.EDIT_CARVE)
    _resident(ctx, s)

    def call():
        return {"points": ctx.query_points(pts), "regions": ctx.query_regions(brushes), "nearest": ctx.query_nearest_records(pts, np.inf)}

    def statement(out):
        assert (out["points"]["solid"] == 1).any() and (out["regions"]["filled"] > 0).any() and (out["nearest"]["node"] >= 0).all()

    _ignoring(ctx, orc, s, call, statement)


# ================================================================ GPU: the entries that honour the update
def _kernels(s):
    import test_gpu_parity as tgp
    rto = _rto()
    return tgp.KERNELS if s.name != "D" else [("auto", rto.KERNEL_AUTO), ("generic", rto.KERNEL_GENERIC)]


def _check_box_renders(ctx, orc, s, state, what):
    """Every box-render entry against the oracle over the reference's compacted array of `state`."""
    rto = _rto()
    compact, _ = s.culled(orc, state)
    for W, H in fs.FRAMES:
        f = _frame(s, W, H)
        want, st = _oracle_frame(orc, s, state, W, H)
        steps = orc.render_steps(compact, s.min, s.voxel, s.view, s.pos, W / H, fs.FOV, W, H) if len(compact) else None
        seen = []
        for kname, kernel in _kernels(s):
            ctx.set_kernel(kernel)
            got = ctx.render_host(f)
            assert got.tobytes() == want.tobytes(), f"{what} {W}x{H} {kname}: {_changed_pixels(got, want)} pixels differ from the oracle"
            gsteps, gs = ctx.render_steps(f), ctx.frame_stats(f)
            if st is not None:
                assert np.array_equal(gsteps, steps), f"{what} {W}x{H} {kname}: step counts"
                assert (gs["rays"], gs["pops"], gs["hits"], gs["capped"]) == (W * H, st["pops"], st["hits"], st["capped"]), (what, kname, gs, st)
            else:                                              # nothing survives: no hit, no capped ray, and the kernels agree on the rest
                assert (gs["rays"], gs["hits"], gs["capped"]) == (W * H, 0, 0), (what, kname, gs)
                seen.append((gsteps.tobytes(), gs["pops"]))
        assert len(set(seen)) <= 1, f"{what} {W}x{H}: the kernels disagree on the steps of an empty array"
        ctx.set_kernel(rto.KERNEL_AUTO)
        got, gs = ctx.render_closest_host(f, stats=True)
        if len(compact):
            wantc, stc = orc.render_closest(compact, s.min, s.voxel, s.view, s.pos, W / H, fs.FOV, W, H)
            assert got.tobytes() == wantc.tobytes(), f"{what} {W}x{H}: closest-hit render, {_changed_pixels(got, wantc)} pixels differ"
            assert (gs["rays"], gs["pops"], gs["hits"]) == (W * H, stc["pops"], stc["hits"]), (what, gs, stc)
        else:
            assert (got == BACKGROUND).all() and (gs["rays"], gs["hits"]) == (W * H, 0), (what, gs)
        ctx.render_resident(f, _hip().RESIDENT_OCTREE)
        assert ctx.download_resident().tobytes() == want.tobytes(), f"{what} {W}x{H}: the resident frame"


@gpu
@pytest.mark.parametrize("name", fs.FRAME_SCENES)
def test_box_renders_honour_the_state(ctx, orc, name):
    """rto_render_host under every kernel, rto_render_steps_host, rto_frame_stats, rto_render_closest_host with stats and
    rto_render_resident: the oracle's frame, step counts and counters over the reference's compacted array; the first frame comes
    directly after the update; the survivors and their count are the reference's, byte for byte."""
    s = scene(orc, name)
    _resident(ctx, s)
    try:
        _check_box_renders(ctx, orc, s, "OFF", f"{name} OFF")
        for state in s.states()[1:]:
            compact, _ = s.culled(orc, state)
            W, H = fs.FRAMES[0]
            _set_state(ctx, s, state)
            first = ctx.render_host(_frame(s, W, H))                         # survivors not counted yet
            want, _ = _oracle_frame(orc, s, state, W, H)
            assert first.tobytes() == want.tobytes(), f"{name} {state}: the frame directly after the update, {_changed_pixels(first, want)} pixels"
            info = ctx.info()
            assert info.culling_active == 1 and info.visible_nodes == len(compact), (state, info.visible_nodes, len(compact))
            assert ctx.download_visible_nodes().tobytes() == compact.tobytes(), f"{name} {state}: the compacted array"
            _check_box_renders(ctx, orc, s, state, f"{name} {state}")
            _set_state(ctx, s, "OFF")
            info = ctx.info()
            assert info.culling_active == 0 and info.visible_nodes == len(s.nodes)
            assert ctx.download_visible_nodes().tobytes() == s.nodes.tobytes()
            full, _ = _oracle_frame(orc, s, "OFF", W, H)
            for kname, kernel in _kernels(s):
                ctx.set_kernel(kernel)
                assert ctx.render_host(_frame(s, W, H)).tobytes() == full.tobytes(), f"{name} OFF_AGAIN after {state}, {kname}"
            ctx.set_kernel(_rto().KERNEL_AUTO)
    finally:
        _restore(ctx)


@gpu
@pytest.mark.parametrize("name", fs.FRAME_SCENES)
def test_ray_skip_family_follows_use_visibility(ctx, orc, name):
    """rto_octree_ray_skip, rto_render_skip_host and rto_probe_skip_host: with use_visibility the oracle's forms under the
    update's flags, without it the bytes with culling off (the oracle's without a map)."""
    s = scene(orc, name)
    W, H = fs.FRAMES[1]
    f = _frame(s, W, H)
    rd = _pixel_rays(orc, s, W, H)[np.random.default_rng(3).choice(W * H, 256, replace=False)]
    _resident(ctx, s)

    hip = _hip()
    canonical = s.name != "D"            # rto_render_skip_* and rto_probe_skip_* take canonical trees only, whatever the state

    def call(use):
        out = {"skip": ctx.octree_ray_skip(s.pos, rd, use_visibility=use)}
        if canonical:
            out["rgba"], out["dist"] = ctx.render_skip_host(f, use_visibility=use)
            value, out["probes"] = ctx.probe_skip_host(s.view, s.pos, W / H, 0.0, use_visibility=use, with_probes=True)
            out["probe"] = np.float32(value)
        else:
            for refused in (lambda: ctx.render_skip_host(f, use_visibility=use),
                            lambda: ctx.probe_skip_host(s.view, s.pos, W / H, 0.0, use_visibility=use)):
                with pytest.raises(hip.RtoError) as e:
                    refused()
                assert e.value.code == hip.RTO_E_UNSUPPORTED
        return _blobs(out)

    def oracle(vis):
        out = {"skip": orc.octree_ray_skip_many(s.nodes, s.min, s.voxel, s.pos, rd, visible=vis)}
        if canonical:
            out["rgba"], out["dist"] = orc.render_skip(s.nodes, s.min, s.voxel, s.view, s.pos, W / H, fs.FOV, W, H, visible=vis)
            out["probe"] = np.float32(orc.probe_skip_distance(s.nodes, s.min, s.voxel, s.view, s.pos, W / H, 0.0, visible=vis))
        return _blobs(out)

    def follows(got, want, what):                      # the oracle states everything but the 49 probe distances themselves
        _same_bytes({k: got[k] for k in want}, want, what)

    try:
        off = call(False)
        plain = oracle(None)
        follows(off, plain, f"{name} OFF")
        _same_bytes(call(True), off, f"{name} OFF use_visibility True")
        for state in s.states()[1:]:
            _, vis = s.culled(orc, state)
            _set_state(ctx, s, state)
            want = oracle(vis)
            assert want["skip"] != plain["skip"], f"{name} {state}: the flags must change the oracle's distances"
            follows(call(True), want, f"{name} {state} with the flags")
            _same_bytes(call(False), off, f"{name} {state} without the flags")
            _set_state(ctx, s, "OFF")
            for use in (False, True):
                _same_bytes(call(use), off, f"{name} OFF_AGAIN after {state} use_visibility {use}")
    finally:
        _restore(ctx)


@gpu
def test_scene_c_counts_compaction_and_frames(ctx, orc):
    """The 128^3 checkerboard, HALF, NONE and ROOTLESS: the first run of k_cull_desc's reduction beyond 256 workgroups (NONE and
    ROOTLESS: the root is culled) and of the on-demand count beyond 1,024 blocks (HALF: the root is visible, the survivors are
    counted when rto_octree_info_get asks).  Count, culling_active, the compacted array and one frame per state, on the default
    and on the generic kernel, are the oracle's."""
    rto = _rto()
    s = scene(orc, "C")
    W, H = fs.BIG_FRAME
    f = _frame(s, W, H)
    _resident(ctx, s)
    try:
        for state in ("HALF", "NONE", "ROOTLESS"):
            compact, vis = s.culled(orc, state)
            want, st = _oracle_frame(orc, s, state, W, H)
            _set_state(ctx, s, state)
            first = ctx.render_host(f)                                      # from the device-side start state alone
            assert first.tobytes() == want.tobytes(), f"C {state}: the frame directly after the update, {_changed_pixels(first, want)} pixels"
            info = ctx.info()
            assert info.culling_active == 1 and info.visible_nodes == len(compact) == int(vis.sum()), (state, info.visible_nodes, len(compact))
            assert ctx.download_visible_nodes().tobytes() == compact.tobytes(), f"C {state}: the compacted array"
            for kname, kernel in (("auto", rto.KERNEL_AUTO), ("generic", rto.KERNEL_GENERIC)):
                ctx.set_kernel(kernel)
                got = ctx.render_host(f)
                assert got.tobytes() == want.tobytes(), f"C {state} {kname}: {_changed_pixels(got, want)} pixels differ from the oracle"
                if st is not None:
                    gs = ctx.frame_stats(f)
                    assert (gs["pops"], gs["hits"], gs["capped"]) == (st["pops"], st["hits"], st["capped"]), (state, kname, gs, st)
            ctx.set_kernel(rto.KERNEL_AUTO)
            _set_state(ctx, s, "OFF")
            info = ctx.info()
            assert info.culling_active == 0 and info.visible_nodes == len(s.nodes)
        full, _ = _oracle_frame(orc, s, "OFF", W, H)
        assert ctx.render_host(f).tobytes() == full.tobytes(), "C OFF_AGAIN"
    finally:
        _restore(ctx)


# ================================================================ GPU: the refusal, and the edits
@gpu
@pytest.mark.parametrize("name", ["A", "B-internal"])
def test_triangle_render_refuses_and_changes_nothing(ctx, orc, name):
    """rto_render_triangles_host in every state but OFF: RTO_E_UNSUPPORTED with the header's message; info, nodes and triangles as
    before the call; after culling is switched off again the frame with culling off, bit for bit, which is the oracle's."""
    hip = _hip()
    s = scene(orc, name)
    tris, off = s.triangles(orc)
    W, H = fs.FRAMES[1]
    f = _frame(s, W, H)
    _resident(ctx, s)
    ctx.build_leaf_triangles(None)
    try:
        before = ctx.render_triangles_host(f, shadow=True)
        want, st = orc.render_triangles(s.nodes, tris, off, s.min, s.voxel, s.view, s.pos, W / H, fs.FOV, W, H, shadow=True)
        assert before.tobytes() == want.reshape(H, W, 4).tobytes() and st["hits"] >= 100
        for state in s.states()[1:]:
            _set_state(ctx, s, state)
            info, nodes, (t0, o0) = bytes(ctx.info()), ctx.download_nodes(), ctx.download_leaf_triangles()
            assert ctx.info().culling_active == 1
            for shadow in (True, False):
                with pytest.raises(hip.RtoError) as e:
                    ctx.render_triangles_host(f, shadow=shadow)
                assert e.value.code == hip.RTO_E_UNSUPPORTED and REFUSAL in str(e.value), (state, str(e.value))
            t1, o1 = ctx.download_leaf_triangles()
            assert bytes(ctx.info()) == info and ctx.download_nodes().tobytes() == nodes.tobytes(), state
            assert t1.tobytes() == t0.tobytes() and o1.tobytes() == o0.tobytes(), state
            _set_state(ctx, s, "OFF")
            assert ctx.render_triangles_host(f, shadow=True).tobytes() == before.tobytes(), f"OFF_AGAIN after {state}"
    finally:
        _restore(ctx)


def test_the_header_states_the_refusal():
    """include/rto_hip.h names the code and the message of the refusal the test above asserts."""
    import os
    hdr = " ".join(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rto_hip.h")).read().split())
    hdr = hdr.replace(" * ", " ")
    assert "RTO_E_UNSUPPORTED (\"" + REFUSAL + "\")" in hdr




def _left_as_a_fresh_build(ctx, orc, dims, gmin, vs, view, pos, what):
    """After a call that changed the grid: culling off, every node counted visible, the nodes the oracle's octree of the voxels
    now resident, and rto_render_host the oracle's frame of that whole tree."""
    W, H = fs.FRAMES[1]
    info = ctx.info()
    assert info.culling_active == 0 and info.visible_nodes == info.num_nodes, (what, info.visible_nodes, info.num_nodes)
    nodes = orc.build_flat_octree(orc.Grid(dims, gmin, vs, ctx.download_voxels()))
    assert ctx.download_nodes().tobytes() == nodes.tobytes(), what
    want, st = orc.render(nodes, gmin, vs, view, pos, W / H, fs.FOV, W, H)
    got = ctx.render_host(_hip().make_frame(view, pos, W / H, fs.FOV, W, H))
    assert st["hits"] >= fs.MIN_CHANGED_PIXELS * W * H, what              # a thinned grid is sparse; a frame of misses would show nothing
    assert got.tobytes() == want.tobytes(), f"{what}: {_changed_pixels(got, want)} pixels differ from the oracle on the edited tree"


@gpu
def test_a_call_that_changes_the_grid_leaves_culling_off(ctx, orc):
    """Every entry whose header says "frustum culling off", called under HALF: rto_edit_voxels, _components, _morphology,
    _geodesic and _skeleton, each on the seeded 16^3 grid, rto_edit_parts on parts_ref's two balls (the cut test_parts.py
    makes), rto_voxelize_mesh of a closed box.  Each changes voxels, by construction: a carve in the middle of 35 % noise, its
    debris, an erosion by one voxel, a flood from an empty voxel, the thinning of a solid 8^3 block, a neck between two balls.
    (tests/test_voxel_edits.py asserts the converse: an edit that changes nothing leaves culling on.)"""
    import parts_ref
    hip = _hip()
    s = scene(orc, "B-leaf")
    c = (s.min + np.float32(0.5 * s.edge)).astype(np.float32)
    empty = int(np.flatnonzero(s.grid.data.ravel() == 0)[0])
    edits = (("rto_edit_voxels", lambda: ctx.edit_voxels(hip.make_brushes([c], np.float32(0.2 * s.edge), hip.BRUSH_SPHERE, hip.EDIT_CARVE))),
             ("rto_edit_components", lambda: ctx.edit_components(hip.SET_SOLID, hip.CONN_FACE, hip.SELECT_ALL_BUT_LARGEST)),
             ("rto_edit_morphology", lambda: ctx.edit_morphology(hip.MORPH_ERODE, float(s.voxel))),
             ("rto_edit_geodesic", lambda: ctx.edit_geodesic([empty], hip.SET_EMPTY, hip.CONN_FACE, 2)),
             ("rto_edit_skeleton", lambda: ctx.edit_skeleton(hip.SET_SOLID, hip.CONN_FULL, hip.SKEL_TOPOLOGY)))
    try:
        for what, edit in edits:
            _resident(ctx, s)                                  # each edit on the grid as seeded
            _set_state(ctx, s, "HALF")
            info = ctx.info()
            assert info.culling_active == 1 and 0 < info.visible_nodes < info.num_nodes, what
            assert edit() > 0, what
            _left_as_a_fresh_build(ctx, orc, s.grid.dims, s.min, s.voxel, s.view, s.pos, what)
        # the two balls, 40 x 24 x 24 voxels of 1 / 64 from (-0.5, -0.5, -0.5); HALF: a slab of the 64-voxel root box along x
        balls = parts_ref.two_balls(40, 24, 24)
        gmin, vs = np.array([-0.5, -0.5, -0.5], np.float32), np.float32(1.0 / 64)
        ctx.build_octree(balls, gmin, vs)
        ctx.debug_update_frustum_planes(np.array(((1.0, 0.0, 0.0, 0.25), (-1.0, 0.0, 0.0, -0.20)) + (fs.KEEP,) * 4, np.float32), 0.0)
        info = ctx.info()
        assert info.culling_active == 1 and 0 < info.visible_nodes < info.num_nodes
        assert ctx.edit_parts(hip.SET_SOLID, hip.CONN_FACE, 800) > 0
        cam = orc.Camera(0.6, 0.45, 1.2)
        cam.set_target(-0.19, -0.31, -0.31)
        _left_as_a_fresh_build(ctx, orc, (40, 24, 24), gmin, vs, cam.get_view(), cam.get_pos(), "rto_edit_parts")
        # rto_voxelize_mesh replaces the scene: a closed box on a fixed 32^3 grid
        ctx.debug_update_frustum_planes(np.array(((1.0, 0.0, 0.0, 0.25), (-1.0, 0.0, 0.0, -0.20)) + (fs.KEEP,) * 4, np.float32), 0.0)
        assert ctx.info().culling_active == 1
        lo, hi = 6.3, 25.6
        xyz = np.array([[x, y, z] for z in (lo, hi) for y in (lo, hi) for x in (lo, hi)], np.float64)
        faces = np.array([[0, 1, 3], [0, 3, 2], [4, 7, 5], [4, 6, 7], [0, 5, 1], [0, 4, 5], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                          [1, 5, 7], [1, 7, 3]], np.int32)
        res = ctx.voxelize_mesh(xyz, faces, 1.0, grid=((32, 32, 32), (0.0, 0.0, 0.0), 1.0))
        assert res.filled > 0
        cam = orc.Camera(0.6, 0.45, 70.0)
        cam.set_target(16.0, 16.0, 16.0)
        _left_as_a_fresh_build(ctx, orc, (32, 32, 32), np.asarray(res.grid_min, np.float32), np.float32(res.voxel_size), cam.get_view(),
                               cam.get_pos(), "rto_voxelize_mesh")
    finally:
        _restore(ctx)
