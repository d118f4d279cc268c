"""Field views and mesh extraction (section 16) on octrees of depth 11 to 20, which their own suites never
reach: tests/test_field_view.py stops at depth 8 and tests/test_mesh_extract.py at a root of 256 voxels.  (The projections' long
rows are in tests/test_projection.py.)

Field views: the "bar" scenes of tests/deep_scenes.py, whose solid leaves are 4 or 16 voxels wide, at x up to 2^20 -- the voxel
rule floor((p - gridMin) / voxelSize) decides something only inside a leaf larger than a voxel, and only there can a float32 step of
p that is a visible part of a voxel (1/16 of one at x = 2^19 with voxel 1, 1/13 at voxel 0.1) pick another voxel.  The volume is
the voxel's own linear index, so the sampled voxel is the value.  k_field_sample's LDS stacks grow with the depth: 61,440 bytes
at depth 20.  Every frame against tests/field_view_ref.py over query_ref.Tree32, bit for bit.

Mesh extraction: MC and CUBES on the "thin" and "bar" grids at every depth of deep_scenes.DEPTHS, and MC on uploaded "spine"
trees, against tests/mesh_ref.py, byte for byte: all 21 slots of the level table, a launch per level up to the twenty-first, the
ancestor loop of the culled count over 20 levels, cube corners at x near 2^20.  Without planes and with every scene camera's.

Without a GPU: the conditions the reference frames and lists have to meet (they are asserted again in front of every GPU
comparison), the Morton order of the lists, and the host layer's renderOctree walk with its two renderers on the same scenes."""
from __future__ import annotations

import numpy as np
import pytest

import deep_scenes as ds
import distance_ref as dr
import field_view_ref as fr
import mesh_ref as mr
import query_ref as q

gpu = pytest.mark.gpu
W, H = 48, 40
FOV = 45.0
NEAR = 0.01                 # the near plane of rto_frustum_planes' projection, in world units

# (depth, grid kind) of the field-view scenes: every depth in two frames, "tenth" at 16 and 20
VIEW_SCENES = ((12, "frac"), (12, "far"), (16, "tenth"), (16, "frac"), (17, "far"), (17, "frac"), (20, "tenth"), (20, "far"))
# grid kinds of the mesh scenes by depth
MESH_KINDS = {11: ("far", "tenth"), 12: ("frac",), 16: ("tenth",), 17: ("far",), 18: ("frac",), 19: ("tenth",), 20: ("far", "tenth", "frac")}
MESH_SCENES = [(g, d) for g in ("thin", "bar") for d in ds.DEPTHS]
SPINES = (("far", 12), ("frac", 19), ("tenth", 20))
KINDS = ((mr.MESH_MC, "mc"), (mr.MESH_CUBES, "cubes"))


def _hip():
    from ray_tracing_octrees_amd import hip
    return hip


def _lut():
    return _hip().ramp_lut([(0, 0, 96, 255), (0, 200, 255, 255), (255, 255, 0, 200), (255, 32, 0, 255)])


# ================================================================ field views: the reference's frames
_index = {}


def _index_volume(dims):
    """volume[v] = v, the voxel's linear index (50 MB at 12.6 M voxels: only the last one is kept)."""
    if dims not in _index:
        _index.clear()
        dx, dy, dz = dims
        _index[dims] = np.arange(dx * dy * dz, dtype=np.int32).reshape(dz, dy, dx)
    return _index[dims]


def _views(s, i):
    """(label, make_field_view's keywords) of the frames at the camera of cube i: both modes and both samples, one shaded, and
    clip boxes that cut the cube in two across x, across z and across y, one voxel past its middle (inside its one leaf)."""
    c, (dx, dy, dz) = s.edge, s.dims
    cut = c // 2 + 1
    out = [(f"mode {m} sample {sm}", dict(mode=m, sample=sm)) for m in (0, 1) for sm in (0, 1)]
    out.append(("shaded", dict(mode=1, shade=True, scale=1)))
    out.append(("cut across x", dict(shade=True, clip=((0, 0, 0), (s.blocks[i] + cut, dy, dz)))))
    out.append(("cut across z", dict(mode=1, clip=((0, 0, 0), (dx, dy, cut)))))
    out.append(("cut across y", dict(scale=2, clip=((0, 0, 0), (dx, cut, dz)))))
    return out


def _view_frames(orc, d, kind):
    """[(label, view, pos, the rto_field_view, the statement's (rgba, values, summary, bins))] of a bar scene under the index
    volume, after the checks the statement's own frames have to pass:
      * HIT, both modes, both cameras: at least 500 hit pixels in leaves larger than a voxel, and at least 30 distinct voxels
        sampled inside them (all 37 a 4-cube shows to this camera; hundreds of a 16-cube's);
      * FRONT at the second cube: at least 50 valued pixels (the voxels in front of its +x face); at the last cube none, and at
        least 500 NONE: its +x neighbours lie past the grid's end, the others past its sides;
      * a cut: at least 100 pixels whose ray begins inside the cube's leaf (no entry face: all three axes come from the floor),
        and on them every voxel of a 4-cube's cut face, at least 100 of a 16-cube's."""
    hip = _hip()
    s = ds.scene(kind, d, "bar")
    T = q.Tree32(s.nodes, s.min, s.voxel)
    vol = _index_volume(s.dims)
    assert int(s.nodes["size"][0]) == 1 << d and set(np.unique(s.nodes["size"][s.nodes["isSolid"] == 1]).tolist()) == {1, s.edge}
    out = []
    for i, (name, view, pos) in zip((1, 3), s.cameras(orc)):
        rd = orc.generate_rays(view, pos, W / H, FOV, W, H).reshape(-1, 3)
        for label, kw in _views(s, i):
            v = hip.make_field_view(hip.FIELD_CALLER, none_rgba=(0.5, 0.25, 0.125, 0.75), miss_rgba=(0.0, 0.125, 0.25, 1.0), **kw)
            values, ndotl, hits = fr.sample(T, s.min, s.voxel, pos, rd, vol, v)
            hit = hits["node"] >= 0
            valued = hit & (values != fr.NONE)
            big = hit & (hits["size"] > 1)
            what = (d, kind, name, label)
            if "clip" in kw:
                inside = big & (hits["face"] == -1)
                seen = len(np.unique(values[inside & valued]))
                assert inside.sum() >= 100 and seen >= (16 if s.edge == 4 else 100), (what, int(inside.sum()), seen)
            else:
                assert big.sum() >= 500, (what, int(big.sum()))
                if kw.get("sample", 0) == fr.HIT:
                    assert len(np.unique(values[big & valued])) >= 30, what
                elif i == 1:
                    assert valued.sum() >= 50, (what, int(valued.sum()))
                else:
                    assert valued.sum() == 0 and (values == fr.NONE).sum() >= 500, what
            rgba, summary, bins = fr.colour(values, ndotl, v, _lut())
            out.append((f"{name} {label}", view, pos, v, (rgba.reshape(H, W, 4), values.reshape(H, W), summary, bins)))
    return s, T, vol, out


def _same_view(got, want, what):
    """A frame's four results against the statement's, bit for bit."""
    rgba, values, summary, bins = got
    wr, wv, ws, wb = want
    assert np.array_equal(values, wv), f"{what}: {int((values != wv).sum())} values differ"
    assert summary.tolist() == ws.tolist(), (what, summary, ws)
    assert np.array_equal(bins, wb), what
    assert rgba.shape == wr.shape and rgba.tobytes() == wr.tobytes(), \
        f"{what}: {int((rgba.view(np.uint32) != wr.view(np.uint32)).any(-1).sum())} pixels differ"


@pytest.mark.parametrize("d,kind", VIEW_SCENES)
def test_bar_frames_meet_their_conditions(orc, d, kind):
    """The statement alone: every frame the GPU test compares passes _view_frames' checks, and the frames of a scene differ from
    one another where they should (CLOSEST is FIRST on these convex views; FRONT is not HIT; a cut is not the whole)."""
    s, T, vol, frames = _view_frames(orc, d, kind)
    assert len(frames) == 16
    by = {label: want for label, _, _, _, want in frames}
    for cam in ("block1", "block3"):
        assert np.array_equal(by[f"{cam} mode 0 sample 0"][1], by[f"{cam} mode 1 sample 0"][1])
        assert not np.array_equal(by[f"{cam} mode 0 sample 0"][1], by[f"{cam} mode 0 sample 1"][1])
        for cut in ("x", "z", "y"):
            assert not np.array_equal(by[f"{cam} mode 0 sample 0"][1], by[f"{cam} cut across {cut}"][1])
    # a float32 step of the hit point is a visible part of a voxel where the issue says it is
    x = float(s.world((s.blocks[3], 0, 0))[0])
    if (d, kind) in ((20, "far"), (20, "tenth")):
        assert float(np.spacing(np.float32(x))) / float(s.voxel) >= 1 / 16


# ================================================================ field views: the GPU's frames
def _device_frames(ctx, torch, hip, d_vol, d_lut):
    """render(frame, view) -> (rgba, values, summary, bins) through rto_render_field_device with the volume already resident."""
    n = W * H
    d_rgba = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
    d_values = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_summary = torch.zeros(4, dtype=torch.int64, device="cuda")
    d_bins = torch.zeros(256, dtype=torch.int64, device="cuda")

    def render(f, v):
        d_rgba.fill_(7.0); d_values.fill_(7); d_summary.fill_(7); d_bins.fill_(7)
        torch.cuda.synchronize()
        ctx.render_field_device(f, v, d_lut.data_ptr(), d_rgba.data_ptr(), d_vol.data_ptr() if d_vol is not None else 0, d_values.data_ptr(),
                                d_summary.data_ptr(), d_bins.data_ptr())
        ctx.synchronize()
        torch.cuda.synchronize()
        return (d_rgba.cpu().numpy().reshape(H, W, 4), d_values.cpu().numpy().reshape(H, W),
                d_summary.cpu().numpy().view(hip.FIELD_VIEW_SUMMARY_DTYPE)[0], d_bins.cpu().numpy())
    return render


@gpu
@pytest.mark.parametrize("d,kind", VIEW_SCENES)
def test_gpu_field_views_on_deep_trees(ctx, orc, d, kind):
    """rto_build_octree leaves deep_scenes' array resident (depth d); then values, rgba, summary and bins of the sixteen frames
    of _view_frames against the statement, bit for bit, through the device form with the index volume uploaded once, and the
    first frame of either camera through the host form too.  Depth 20 launches k_field_sample with 61,440 bytes of LDS.  At
    depth 12 also the resident distance to EMPTY, held to tests/distance_ref.py first."""
    torch = pytest.importorskip("torch")
    hip = _hip()
    s, T, vol, frames = _view_frames(orc, d, kind)
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(s.data, s.min, s.voxel)
    assert ctx.download_nodes().tobytes() == s.nodes.tobytes()
    info = ctx.info()
    assert info.canonical == 1 and info.depth == d
    d_lut = torch.from_numpy(_lut().view(np.int32)).cuda()
    d_vol = torch.from_numpy(vol).cuda()
    render = _device_frames(ctx, torch, hip, d_vol, d_lut)
    for label, view, pos, v, want in frames:
        f = hip.make_frame(view, pos, W / H, FOV, W, H)
        _same_view(render(f, v), want, f"d {d} {kind} {label}")
        if label.endswith("mode 0 sample 0"):
            _same_view(ctx.render_field_host(f, v, _lut(), vol), want, f"d {d} {kind} {label}, host form")
    del d_vol
    if d != 12:
        return
    field = ctx.distance_field(hip.SET_EMPTY)[0]
    assert np.array_equal(field, dr.field(s.data, dr.SET_EMPTY))
    render = _device_frames(ctx, torch, hip, None, d_lut)
    for name, view, pos in s.cameras(orc):
        rd = orc.generate_rays(view, pos, W / H, FOV, W, H).reshape(-1, 3)
        f = hip.make_frame(view, pos, W / H, FOV, W, H)
        for kw in (dict(scale=1, shade=True), dict(mode=1, valid=(2, 0x7ffffffe))):
            v = hip.make_field_view(hip.FIELD_DISTANCE, **kw)
            want = fr.frame(T, s.min, s.voxel, pos, rd, W, H, field, v, _lut())
            assert not fr.degenerate(want[1], v) and want[2]["vmax"] >= 36, (name, kw, want[2])
            _same_view(render(f, v), want, f"d {d} {kind} {name} distance {kw}")
            _same_view(ctx.render_field_host(f, v, _lut()), want, f"d {d} {kind} {name} distance {kw}, host form")


# ================================================================ mesh extraction: the reference's lists
_mesh = {}


def _margin(s):
    """renderOctree's default 50 world units, but in the unit-sized "frac" frame -- which 50 would swallow -- 4 voxels past the
    near plane's 0.01: the scenes' near cameras stand closer to their blobs than that plane."""
    return 50.0 if s.kind != "frac" else NEAR + 4 * float(s.voxel)


def _plane_sets(orc, s):
    hip = _hip()
    return [("no planes", None)] + [(name, hip.frustum_planes(view, FOV, W / H)) for name, view, _ in s.cameras(orc)]


def _mesh_case(orc, geometry, d, kind):
    """(scene, leaf triangles, offsets, {(mesh kind, plane set): (tris, tri_node)}) of a scene, made once; a spine scene (no
    dense grid) has MC only, on test_triangle_queries' triangles.  Condition on the lists: for either kind some camera keeps
    some but not all of the triangles."""
    key = (geometry, d, kind)
    if key not in _mesh:
        s = ds.scene(kind, d, geometry)
        if geometry == "spine":
            from test_triangle_queries import _spine_triangles
            tris, off = _spine_triangles(s)
            kinds = KINDS[:1]
        else:
            tris, off = orc.build_leaf_triangles(orc.Grid(s.dims, s.min, s.voxel, s.data), s.nodes)
            tris, off = np.ascontiguousarray(tris, np.float32).reshape(-1, 12), np.asarray(off, np.int32)
            kinds = KINDS
        ref = {}
        for mk, _ in kinds:
            for pname, planes in _plane_sets(orc, s):
                ref[mk, pname] = mr.extract(mk, s.nodes, s.min, s.voxel, data=None if geometry == "spine" else s.data, tris=tris, tri_offset=off,
                                            planes=planes, margin=_margin(s))
            full = len(ref[mk, "no planes"][0])
            kept = [len(t) for (k, p), (t, _) in ref.items() if k == mk and p != "no planes"]
            assert full > 0 and any(0 < n < full for n in kept), (key, mk, full, kept)
        _mesh[key] = (s, tris, off, ref)
    return _mesh[key]


def _mesh_params():
    return [(g, d, kind) for g, d in MESH_SCENES for kind in MESH_KINDS[d]] + [("spine", d, kind) for kind, d in SPINES]


@pytest.mark.parametrize("geometry,d,kind", _mesh_params())
def test_deep_lists_are_culled_in_part_and_in_morton_order(orc, geometry, d, kind):
    """The statement alone, on every scene the GPU test runs: a camera that keeps some but not all triangles (_mesh_case); the
    owning leaves in ascending Morton order of their corners, each leaf's triangles contiguous; corners up to 2^d."""
    s, tris, off, ref = _mesh_case(orc, geometry, d, kind)
    assert int(s.nodes["size"][0]) == 1 << d
    for (mk, pname), (t, owner) in ref.items():
        if len(owner) == 0:
            continue
        leaves = owner[np.concatenate([[True], owner[1:] != owner[:-1]])]
        assert len(set(leaves.tolist())) == len(leaves)
        code = mr.morton(s.nodes["x"][leaves], s.nodes["y"][leaves], s.nodes["z"][leaves])
        assert (code[1:] > code[:-1]).all(), (geometry, d, kind, mk, pname)
    if geometry != "spine":
        cubes = ref[mr.MESH_CUBES, "no planes"][0]
        solid = s.nodes[(s.nodes["isLeaf"] == 1) & (s.nodes["isSolid"] == 1)]
        assert (solid["x"] + solid["size"]).max() >= s.dims[0] - 1 > 0.74 * (1 << d)
        assert cubes[:, 0:9:3].max() == mr.boxes(solid, s.min, s.voxel)[1][:, 0].max()     # a cube face at the grid's +x end
        assert {1, 2 if geometry == "thin" else s.edge} <= set(s.nodes["size"][ref[mr.MESH_CUBES, "no planes"][1]].tolist())


def _rec12(t18):
    t18 = np.asarray(t18, np.float32).reshape(-1, 18)
    assert t18[:, 9:12].tobytes() == t18[:, 12:15].tobytes() == t18[:, 15:18].tobytes()
    return np.ascontiguousarray(t18[:, :12])


@pytest.mark.parametrize("geometry,d", MESH_SCENES)
def test_host_walk_equals_the_rule_on_deep_grids(orc, geometry, d):
    """host/Renderer.cpp through host_capi on the deep grids: createOctreeFromVoxelGrid, then renderOctree's walk with
    MarchingCubesRenderer and VoxelCubeRenderer, without planes and under every camera's, against tests/mesh_ref.py."""
    from ray_tracing_octrees_amd import host
    kind = MESH_KINDS[d][-1]
    s, tris, off, ref = _mesh_case(orc, geometry, d, kind)
    grid = host.VoxelGrid.from_array(s.data, s.min, s.voxel)
    root = host.createOctreeFromVoxelGrid(grid)
    try:
        assert root.flatten().tobytes() == s.nodes.tobytes()
        for mk, kname in KINDS:
            r = host.MarchingCubesRenderer() if mk == mr.MESH_MC else host.VoxelCubeRenderer()
            for pname, planes in _plane_sets(orc, s):
                got = _rec12(host.renderOctreePlanes(root, grid, r, planes, _margin(s)))
                assert got.tobytes() == ref[mk, pname][0].tobytes(), (geometry, d, kind, kname, pname, len(got))
    finally:
        host.freeOctree(root)


# ================================================================ mesh extraction: the GPU's lists
def _check_lists(ctx, orc, s, ref, kinds, what):
    for mk, kname in kinds:
        for pname, planes in _plane_sets(orc, s):
            want, wnode = ref[mk, pname]
            got, gnode = ctx.extract_mesh(mk, planes, _margin(s))
            assert got.tobytes() == want.tobytes(), (what, kname, pname, got.shape, want.shape)
            assert gnode.tobytes() == wnode.tobytes(), (what, kname, pname)
            assert ctx.mesh_device()[2] == len(want)


@gpu
@pytest.mark.parametrize("geometry,d", MESH_SCENES)
def test_gpu_lists_on_deep_grids(ctx, orc, geometry, d):
    """rto_build_octree and rto_build_leaf_triangles on the dense grid leave deep_scenes' array and the oracle's triangles
    resident; then the triangle list and tri_node of both kinds against the rule, byte for byte, without planes and under
    every scene camera's.  At depth 20 through both build paths."""
    hip = _hip()
    ctx.set_kernel(hip.KERNEL_AUTO)
    try:
        for kind in MESH_KINDS[d]:
            s, tris, off, ref = _mesh_case(orc, geometry, d, kind)
            for level_by_level in ((False, True) if d == 20 and kind == "far" else (False,)):
                ctx.debug_set_build_path(level_by_level)
                ctx.build_octree(s.data, s.min, s.voxel)
                assert ctx.download_nodes().tobytes() == s.nodes.tobytes()
                assert ctx.info().depth == d
                ctx.build_leaf_triangles()
                gt, go = ctx.download_leaf_triangles()
                assert go.tobytes() == off.tobytes() and gt.tobytes() == tris.tobytes()
                _check_lists(ctx, orc, s, ref, KINDS, f"{geometry} d {d} {kind} level by level {level_by_level}")
    finally:
        ctx.debug_set_build_path(False)


@gpu
@pytest.mark.parametrize("kind,d", SPINES)
def test_gpu_mc_lists_on_uploaded_spines(ctx, orc, kind, d):
    """Uploaded trees of 2^d voxels a side with a few uploaded triangles per solid leaf: MC's list under no planes, the two near
    cameras and the far one.  The corner ball's leaves sit below 20 levels of ancestors, each of which a plane may cull."""
    hip = _hip()
    s, tris, off, ref = _mesh_case(orc, "spine", d, kind)
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.upload_octree(s.nodes, s.min, s.voxel)
    assert ctx.info().canonical == 1 and ctx.info().depth == d
    ctx.upload_leaf_triangles(tris, off)
    _check_lists(ctx, orc, s, ref, KINDS[:1], f"spine d {d} {kind}")
