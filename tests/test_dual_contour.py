"""Dual contouring (rto_extract_dual_contour, rto_query_dual_vertices_*): the reference's per-voxel vertex rule
and its triangulation buildTrianglesCPU over the resident grid.

The expected vertices and lists are the reference's own compiled functions' outputs (tests/golden/ref_dc.npz, made by
tests/golden/make_golden_dc.py); tests/dc_ref.py states the rule in numpy float32 and agrees with them byte for byte, so it serves
as the reference wherever the fixture holds a count and a SHA-256 only, and for tri_cell, the summary and the clip box.  The larger
grids (the clip sweep, the 64^3 sphere) are held against the CPU form dualContourVolume, which the tests below pin to both.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dc_ref as dc
from ray_tracing_octrees_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "ref_dc.npz"))
NAMES = [str(n) for n in Z["names"]]
GRIDS = sorted({str(v) for v in Z["case_grid"]})


def _grid(name):
    dx, dy, dz = (int(v) for v in Z[f"dims_{name}"])
    vox = np.unpackbits(Z[f"bits_{name}"])[:dx * dy * dz].reshape(dz, dy, dx).astype(np.uint8)
    return dict(name=name, vox=vox, gmin=Z[f"min_{name}"], vs=np.float32(Z[f"vs_{name}"]), vsha=bytes(Z[f"vsha_{name}"]),
                verts=Z[f"verts_{name}"] if f"verts_{name}" in Z else None)


def _case(name):
    i = NAMES.index(name)
    g = _grid(str(Z["case_grid"][i]))
    return dict(g, case=name, rule=int(Z["area_rule"][i]), count=int(Z["counts"][i]), dropped=int(Z["dropped"][i]), sha=bytes(Z["sha256"][i]),
                tris=Z[f"tris_{name}"] if f"tris_{name}" in Z else None)


_VERTS, _REF = {}, {}


def _ref_vertices(g):
    """dc_ref's vertex volume of a fixture grid as (verts, points, 16-byte records), computed once."""
    if g["name"] not in _VERTS:
        verts, points, _ = dc.vertices(g["vox"], g["gmin"], g["vs"])
        rec = np.zeros(g["vox"].shape, hip.DUAL_VERTEX_DTYPE)
        rec["p"], rec["points"] = verts, points
        _VERTS[g["name"]] = (verts, points, rec)
    return _VERTS[g["name"]]


def _ref(c, clip=None, rule=None):
    """dc_ref's (tris, tri_cell, summary) of a fixture case, computed once."""
    rule = c["rule"] if rule is None else rule
    key = (c["name"], rule, clip)
    if key not in _REF:
        verts, points, _ = _ref_vertices(c)
        _REF[key] = dc.extract(c["vox"], c["gmin"], c["vs"], rule, clip, verts, points)
    return _REF[key]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()


def _summary(s):
    return dict(faces=s.faces, triangles=s.triangles, dropped=s.dropped, degenerate=s.degenerate, vertex_voxels=s.vertex_voxels)


def _same_list(got, want, what):
    tris, cell, summary = got
    wt, wc, ws = want
    assert tris.shape == wt.shape, f"{what}: {tris.shape} against {wt.shape}"
    assert tris.tobytes() == wt.tobytes(), f"{what}: {int((tris.view(np.uint32) != wt.view(np.uint32)).any(axis=1).sum())} records differ"
    assert np.array_equal(cell, wc), f"{what}: tri_cell"
    assert _summary(summary) == ws and summary.reserved == 0, f"{what}: summary {_summary(summary)} against {ws}"


def _from18(t18):
    assert (t18[:, 9:12] == t18[:, 12:15]).all() and (t18[:, 9:12] == t18[:, 15:18]).all()
    return np.ascontiguousarray(t18[:, :12])


def _host(vox, gmin, vs, rule, clip=None):
    from ray_tracing_octrees_amd import host
    t18, cell, summary = host.dualContourVolume(vox, gmin, vs, hip.make_dc_params(rule, clip))
    return _from18(t18), cell, summary


# ---------------------------------------------------------------- without a GPU
@pytest.mark.parametrize("name", GRIDS)
def test_dc_ref_vertices_equal_the_reference(name):
    g = _grid(name)
    rec = _ref_vertices(g)[2]
    assert _sha(rec) == g["vsha"]
    if g["verts"] is not None:
        assert rec.tobytes() == g["verts"].tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_dc_ref_lists_equal_the_reference(name):
    c = _case(name)
    tris, cell, summary = _ref(c)
    assert len(tris) == c["count"] and _sha(tris) == c["sha"] and summary["dropped"] == c["dropped"]
    if c["tris"] is not None:
        assert tris.tobytes() == c["tris"].tobytes()


@pytest.mark.parametrize("name", GRIDS)
def test_host_vertices_equal_the_reference(name):
    """Both CPU forms: the arithmetic the kernels run, and the reference's own shape with its points stored."""
    from ray_tracing_octrees_amd import host
    g = _grid(name)
    got = host.dualVertexVolume(g["vox"], g["gmin"], g["vs"])
    assert _sha(got) == g["vsha"]
    adc = host.adaptiveDualContouringVertices(g["vox"], g["gmin"], g["vs"])
    want = _ref_vertices(g)
    assert adc[..., :3].tobytes() == want[0].tobytes() and np.array_equal(adc[..., 3], want[1].astype(np.float32))


@pytest.mark.parametrize("name", NAMES)
def test_host_lists_equal_the_reference(name):
    from ray_tracing_octrees_amd import host
    c = _case(name)
    got = _host(c["vox"], c["gmin"], c["vs"], c["rule"])
    assert len(got[0]) == c["count"] and _sha(got[0]) == c["sha"]
    _same_list(got, _ref(c), name)
    if c["rule"] == dc.AREA_REFERENCE:                   # the reference's entry point, under its name
        r18 = host.adaptiveDualContouringRender(c["vox"], c["gmin"], c["vs"])
        assert _sha(_from18(r18)) == c["sha"]


def test_struct_sizes_match_the_header():
    text = open(os.path.join(ROOT, "include", "rto_hip.h")).read()
    assert re.search(r"typedef struct rto_dc_params \{\s*/\* 48 bytes \*/", text)
    assert re.search(r"typedef struct rto_dc_summary \{\s*/\* 48 bytes \*/", text)
    assert re.search(r"typedef struct rto_dual_vertex \{\s*/\* 16 bytes \*/", text)
    assert C.sizeof(hip.DcParams) == 48 and C.sizeof(hip.DcSummary) == 48 and hip.DUAL_VERTEX_DTYPE.itemsize == 16
    assert hip.DcParams.clip_lo.offset == 8 and hip.DcParams.clip_hi.offset == 20 and hip.DcParams.reserved.offset == 32
    assert hip.DUAL_VERTEX_DTYPE.fields["points"][1] == 12
    for s in ("rto_extract_dual_contour", "rto_dual_contour_device", "rto_download_dual_contour", "rto_last_dual_contour_ms",
              "rto_query_dual_vertices_device", "rto_query_dual_vertices_host"):
        assert s in hip.SYMBOLS and re.search(r"\b%s\(" % s, text)


@pytest.mark.parametrize("name", ["rand12", "sphere16_fine"])
def test_clip_boxes_that_partition_the_cells_partition_the_list(name):
    c = _case(name)
    whole, wcell, ws = _ref(c)
    dz, dy, dx = c["vox"].shape
    for axis, cuts in ((2, (0, 5, 6, dz)), (1, (0, 9, dy)), (0, (0, 1, 8, dx - 1, dx))):
        parts, cells, faces, dropped = [], [], 0, 0
        for a, b in zip(cuts[:-1], cuts[1:]):
            lo, hi = [0, 0, 0], [dx, dy, dz]
            lo[axis], hi[axis] = a, b
            t, cl, s = _ref(c, (tuple(lo), tuple(hi)))
            _same_list(_host(c["vox"], c["gmin"], c["vs"], c["rule"], (tuple(lo), tuple(hi))), (t, cl, s), f"{name} axis {axis} [{a}, {b})")
            parts.append(t); cells.append(cl); faces += s["faces"]; dropped += s["dropped"]
        t, cl = np.concatenate(parts), np.concatenate(cells)
        order = np.argsort(cl, kind="stable")                      # tri_cell rises in raster order
        assert np.array_equal(cl[order], wcell) and t[order].tobytes() == whole.tobytes(), axis
        assert (faces, dropped) == (ws["faces"], ws["dropped"])
        if axis == 2:                                               # slabs along z: plain concatenation
            assert t.tobytes() == whole.tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_summary_counts_add_up(name):
    c = _case(name)
    for rule in (dc.AREA_REFERENCE, dc.AREA_NONE):
        tris, cell, s = _host(c["vox"], c["gmin"], c["vs"], rule)
        assert s.triangles == len(tris) and s.triangles + s.dropped == 2 * s.faces
        zero = int((tris[:, 9:12] == 0).all(axis=1).sum())
        assert s.degenerate == zero
        if rule == dc.AREA_NONE:
            assert s.dropped == 0
        assert s.vertex_voxels == _ref(c, rule=rule)[2]["vertex_voxels"] <= int((_ref_vertices(c)[1] > 0).sum())


def test_the_fine_sphere_shows_the_area_rule_and_degenerates_are_counted():
    c = _case("sphere16_fine")
    assert c["dropped"] == 294 and c["count"] == 1050 and _case("sphere16_fine_all")["count"] == 1344 == _case("sphere16")["count"]
    # a voxel size so small that every cross product underflows: all triangles are degenerate under RTO_DC_AREA_NONE
    tris, cell, s = _host(c["vox"], c["gmin"], np.float32(1e-24), dc.AREA_NONE)
    assert s.degenerate == len(tris) == 1344 and (tris[:, 9:12].view(np.uint32) == 0).all()
    _same_list((tris, cell, s), dc.extract(c["vox"], c["gmin"], np.float32(1e-24), dc.AREA_NONE), "underflow")
    assert _host(c["vox"], c["gmin"], np.float32(1e-24), dc.AREA_REFERENCE)[2].triangles == 0


@pytest.mark.parametrize("name", GRIDS)
def test_every_vertex_lies_within_the_bounds_the_rule_gives_it(name):
    """A vertex without a point is its voxel's centre; a vertex of the plane branch lies within its voxel's inset bounds [lo, hi],
    exactly (it is clamped last).  A vertex of the QEF branches does NOT in general, in the reference either: it is
    0.9 * clamp(solution, lo, hi) + 0.1 * mass point, and the mass point lies in the hull of the gathered points, which reaches
    from the voxel's corner to 1.5 voxels beyond it.  Of the fixture's 30,653 vertices 3,555 lie outside [lo, hi], all of them in
    the branches 'at most 2 points' and 'mass-point fallback' (the reference's own outputs, byte for byte).  What the rule does
    imply for them is asserted: 0.9 * lo + 0.1 * corner <= v <= 0.9 * hi + 0.1 * (corner + 1.5 * voxelSize), with four float32
    ulps of the largest coordinate for the rounding of the products and sums."""
    g = _grid(name)
    verts, points, branch = dc.vertices(g["vox"], g["gmin"], g["vs"])
    dz, dy, dx = g["vox"].shape
    zz, yy, xx = np.indices((dz, dy, dx))
    vs = g["vs"]
    plane = branch == dc.B_PLANE
    qef = (branch != dc.B_PLANE) & (branch != dc.B_NO_POINT)
    for a, idx in enumerate((xx, yy, zz)):
        corner = g["gmin"][a] + idx.astype(np.float32) * vs
        centre = corner + np.float32(0.5) * vs
        lo, hi = (centre - vs * np.float32(0.5)) + vs * np.float32(0.001), (centre + vs * np.float32(0.5)) - vs * np.float32(0.001)
        v = verts[..., a]
        assert (v[branch == dc.B_NO_POINT] == centre[branch == dc.B_NO_POINT]).all()
        assert (v[plane] >= lo[plane]).all() and (v[plane] <= hi[plane]).all()
        slack = 4 * np.float64(np.spacing(np.float32(np.abs(corner).max() + 2 * vs)))
        low = 0.9 * lo.astype(np.float64) + 0.1 * corner.astype(np.float64) - slack
        high = 0.9 * hi.astype(np.float64) + 0.1 * (corner.astype(np.float64) + 1.5 * np.float64(vs)) + slack
        assert (v[qef] >= low[qef]).all() and (v[qef] <= high[qef]).all()


def test_dc_kernels_use_no_scratch():
    """The built gfx950 code object's metadata: every k_dc_* kernel has a private segment of 0 bytes and spills no VGPR."""
    import test_isa_contract as isa
    asm = isa.built_asm()
    if asm is None:
        pytest.skip("no hipcc in this environment")
    meta = isa.kernel_meta(asm)
    names = [k for k in meta if "k_dc_" in k]
    for want in ("k_dc_count", "k_dc_place", "k_dc_emit", "k_dc_query"):
        assert any(want in k for k in names), want
    assert len(names) == 4, names
    for k in names:
        assert meta[k]["scratch"] == 0 and meta[k]["vgpr_spill"] == 0, (k, meta[k])


def test_selftest_passes_under_the_sanitizers(tmp_path):
    """tools/dc_selftest.cpp as a stand-alone program, by the g++ line its header gives."""
    src = os.path.join(ROOT, "tools", "dc_selftest.cpp")
    head = open(src).read(4000)
    m = re.search(r"^//\s+(g\+\+ .*-fsanitize=address,undefined.*)$", head, re.M)
    assert m, "the header gives no build line"
    exe = str(tmp_path / "dc_selftest")
    cmd = m.group(1).split()
    assert cmd[-2:] == ["-o", "dc_selftest"]
    subprocess.run(cmd[:-1] + [exe], cwd=ROOT, check=True)
    r = subprocess.run([exe, "300"], capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_stl_export_of_a_dual_contour(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mesh_export as me
    c = _case("sphere16")
    tris = _ref(c)[0]
    path = str(tmp_path / "dc.stl")
    me.write_stl(path, tris)
    assert os.path.getsize(path) == 84 + 50 * len(tris) and me.read_stl(path).tobytes() == tris.tobytes()


# ---------------------------------------------------------------- on the GPU
def _build(ctx, g):
    ctx.build_octree(g["vox"], g["gmin"], g["vs"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", GRIDS)
def test_gpu_fixture_cases_equal_the_reference(ctx, name):
    g = _grid(name)
    _build(ctx, g)
    for cname in [n for n, gn in zip(NAMES, Z["case_grid"]) if str(gn) == name]:
        c = _case(cname)
        got = ctx.extract_dual_contour(hip.make_dc_params(c["rule"]))
        assert len(got[0]) == c["count"] and _sha(got[0]) == c["sha"], cname
        _same_list(got, _ref(c), cname)
        ms = ctx.last_dual_contour_ms()
        assert len(ms) == 3 and (all(m >= 0 for m in ms) if name != "thin1" else tuple(ms) == (-1.0, -1.0, -1.0))     # no cell, no kernel
        assert ctx.dual_contour_device()[2] == c["count"]
        _same_list(ctx.extract_dual_contour(hip.make_dc_params(1 - c["rule"])), _ref(c, rule=1 - c["rule"]), cname + " the other rule")


@pytest.mark.gpu
@pytest.mark.parametrize("name", GRIDS)
def test_gpu_vertex_queries_equal_the_reference(ctx, name):
    import torch
    g = _grid(name)
    _build(ctx, g)
    n = g["vox"].size
    want = _ref_vertices(g)[2].reshape(-1)
    idx = np.concatenate([np.arange(n, dtype=np.int64), np.array([-1, n, n + 5, -(1 << 40), 1 << 40], np.int64)])
    got = ctx.query_dual_vertices(idx)
    assert _sha(got[:n]) == g["vsha"] and got[:n].tobytes() == want.tobytes()
    assert (got["points"][n:] == -1).all() and (got["p"][n:].view(np.uint32) == 0).all()
    perm = np.random.default_rng(3).permutation(len(idx))
    d_idx = torch.from_numpy(idx[perm]).cuda()
    d_out = torch.zeros(len(idx) * 4, dtype=torch.int32, device="cuda")
    ctx.query_dual_vertices(d_idx, d_out)
    assert d_out.cpu().numpy().view(hip.DUAL_VERTEX_DTYPE).tobytes() == got[perm].tobytes()
    assert len(ctx.query_dual_vertices(np.zeros(0, np.int64))) == 0


@pytest.mark.gpu
def test_gpu_same_lists_in_every_state_of_the_context(ctx, orc):
    """Both octree build paths and a frustum update in force: one list, one set of vertices."""
    c = _case("rand12")
    clip = ((1, 0, 2), (11, 12, 9))
    cam = orc.Camera(0.5, 0.7, 0.6)
    try:
        for level_by_level in (False, True):
            ctx.debug_set_build_path(level_by_level)
            _build(ctx, c)
            for frustum in (False, True):
                ctx.update_frustum(cam.get_view(), 45.0, 4.0 / 3.0, frustum)
                what = f"path {level_by_level} frustum {frustum}"
                _same_list(ctx.extract_dual_contour(hip.make_dc_params(dc.AREA_REFERENCE)), _ref(c), what)
                _same_list(ctx.extract_dual_contour(hip.make_dc_params(dc.AREA_NONE, clip)), _ref(c, clip, dc.AREA_NONE), what + " clip")
                assert ctx.query_dual_vertices(np.arange(c["vox"].size)).tobytes() == _ref_vertices(c)[2].tobytes()
    finally:
        ctx.debug_set_build_path(False)
        ctx.update_frustum(cam.get_view(), 45.0, 4.0 / 3.0, False)


@pytest.mark.gpu
def test_gpu_after_voxelize_and_after_an_edit(ctx):
    lo, hi = np.array([-3.0, -2.0, -1.5]), np.array([3.0, 2.0, 1.5])
    xyz = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for k in (0, 1) for j in (0, 1) for i in (0, 1)], np.float64)
    tris = np.array([(0, 1, 3), (0, 3, 2), (4, 7, 5), (4, 6, 7), (0, 5, 1), (0, 4, 5), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)], np.int32)
    r = ctx.voxelize_mesh(xyz, tris, 0.5)
    gmin, vs = np.array(list(r.grid_min), np.float32), np.float32(r.voxel_size)
    grid = ctx.download_voxels()
    assert grid.any()
    p = hip.make_dc_params(dc.AREA_REFERENCE)
    want = dc.extract(grid, gmin, vs)
    assert len(want[0]) > 0
    _same_list(ctx.extract_dual_contour(p), want, "after voxelize_mesh")
    # an edit: the snapshot survives; a new call sees the edited grid
    centre = (gmin + vs * np.array(grid.shape[::-1], np.float32) * np.float32(0.5)).astype(np.float32)
    assert ctx.edit_voxels(hip.make_brushes([centre], 2 * float(vs), hip.BRUSH_SPHERE, hip.EDIT_CARVE)) > 0
    tris_after, cell_after = ctx.download_dual_contour()
    assert tris_after.tobytes() == want[0].tobytes() and np.array_equal(cell_after, want[1])
    edited = ctx.download_voxels()
    assert not np.array_equal(edited, grid)
    new = dc.extract(edited, gmin, vs)
    assert new[0].tobytes() != want[0].tobytes()
    _same_list(ctx.extract_dual_contour(p), new, "after the edit")
    verts, points, _ = dc.vertices(edited, gmin, vs)
    got = ctx.query_dual_vertices(np.arange(edited.size))
    assert got["p"].tobytes() == verts.tobytes() and np.array_equal(got["points"], points.reshape(-1))


@pytest.mark.gpu
def test_gpu_errors_in_their_order_leave_the_previous_list(orc):
    import ray_tracing_octrees_amd as rto
    ctx = rto.Context(0)
    try:
        c = _case("sphere16")
        ok = hip.make_dc_params(dc.AREA_REFERENCE)

        def refused(code, params, text=None):
            with pytest.raises(hip.RtoError) as e:
                ctx.extract_dual_contour(params)
            assert e.value.code == code, (e.value.code, str(e.value))
            if text:
                assert text in str(e.value)

        def bad(rule=dc.AREA_REFERENCE, clip=None, reserved=None):
            p = hip.make_dc_params(rule, clip)
            if reserved is not None:
                p.reserved[reserved] = 1
            return p

        backwards = ((5, 5, 5), (2, 2, 2))
        # 1. RTO_E_INVALID comes before "nothing uploaded"
        refused(hip.RTO_E_INVALID, None)
        refused(hip.RTO_E_INVALID, bad(rule=2), "area_rule")
        refused(hip.RTO_E_INVALID, bad(rule=-1), "area_rule")
        refused(hip.RTO_E_INVALID, bad(reserved=3), "reserved")
        # 2. RTO_E_NO_OCTREE, before the clip box is looked at
        refused(hip.RTO_E_NO_OCTREE, bad(clip=backwards))
        with pytest.raises(hip.RtoError):
            ctx.download_dual_contour()
        with pytest.raises(hip.RtoError) as e:
            ctx.query_dual_vertices(np.arange(4))
        assert e.value.code == hip.RTO_E_NO_OCTREE
        # 3. RTO_E_UNSUPPORTED without a resident grid, before the clip box
        g = orc.test_sphere_grid(16)
        ctx.upload_octree(orc.build_flat_octree(g), g.min, g.voxel_size)
        refused(hip.RTO_E_UNSUPPORTED, bad(clip=backwards), "no voxel grid is resident")
        refused(hip.RTO_E_INVALID, bad(rule=7, clip=backwards), "area_rule")
        with pytest.raises(hip.RtoError) as e:
            ctx.query_dual_vertices(np.arange(4))
        assert e.value.code == hip.RTO_E_UNSUPPORTED
        # a good extraction, then every refusal again: the list stays
        _build(ctx, c)
        want = _ref(c)
        _same_list(ctx.extract_dual_contour(ok), want, "before the refusals")
        # 4. the clip box
        for lo, hi in (((-1, 0, 0), (4, 4, 4)), ((0, 0, 0), (4, 17, 4)), ((3, 3, 3), (4, 4, 3)), backwards):
            refused(hip.RTO_E_INVALID, bad(clip=(lo, hi)), "clip box")
        refused(hip.RTO_E_INVALID, bad(rule=2))
        refused(hip.RTO_E_INVALID, None)
        tris, cell = ctx.download_dual_contour()
        assert tris.tobytes() == want[0].tobytes() and np.array_equal(cell, want[1])
        # a box without a cell is no error: an empty list, no kernel
        s = ctx.extract_dual_contour(hip.make_dc_params(dc.AREA_NONE, ((15, 0, 0), (16, 16, 16))))
        assert len(s[0]) == 0 and _summary(s[2]) == dict(faces=0, triangles=0, dropped=0, degenerate=0, vertex_voxels=0)
        assert tuple(ctx.last_dual_contour_ms()) == (-1.0, -1.0, -1.0)
        # download: the capacity; the query: its arguments
        _same_list(ctx.extract_dual_contour(ok), want, "again")
        n = C.c_int64()
        buf = np.zeros((4, 12), np.float32)
        assert ctx._L.rto_download_dual_contour(ctx._h, buf.ctypes.data, 4, None, C.byref(n)) == hip.RTO_E_INVALID and n.value == len(want[0])
        assert ctx._L.rto_query_dual_vertices_host(ctx._h, None, 3, buf.ctypes.data) == hip.RTO_E_INVALID
        assert ctx._L.rto_query_dual_vertices_host(ctx._h, buf.ctypes.data, -1, buf.ctypes.data) == hip.RTO_E_INVALID
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_the_three_lists_keep_buffers_of_their_own(ctx, orc):
    import distance_ref as dr
    import iso_ref as ir
    c = _case("sphere16")
    _build(ctx, c)
    ctx.build_leaf_triangles(None)
    mesh = ctx.extract_mesh(hip.MESH_MC)
    d2 = dr.field(c["vox"], dr.SET_EMPTY)
    iso_want = ir.extract(d2, c["gmin"], c["vs"], 2.5, 0.0)
    iso = ctx.extract_isosurface(hip.make_iso_params(hip.FIELD_CALLER, 2.5, 0.0), d2)
    assert len(mesh[0]) > 0 and iso[0].tobytes() == iso_want[0].tobytes()
    want = _ref(c)
    _same_list(ctx.extract_dual_contour(hip.make_dc_params(dc.AREA_REFERENCE)), want, "sphere16")
    again = ctx.download_mesh()
    assert again[0].tobytes() == mesh[0].tobytes() and np.array_equal(again[1], mesh[1])
    assert ctx.download_isosurface()[0].tobytes() == iso_want[0].tobytes()
    ctx.extract_mesh(hip.MESH_CUBES)
    ctx.extract_isosurface(hip.make_iso_params(hip.FIELD_CALLER, 1.5, 0.0), d2)
    tris, cell = ctx.download_dual_contour()
    assert tris.tobytes() == want[0].tobytes() and np.array_equal(cell, want[1])
    assert len({ctx.mesh_device()[0], ctx.isosurface_device()[0], ctx.dual_contour_device()[0]}) == 3


@pytest.mark.gpu
def test_gpu_host_class_equals_the_python_path(ctx):
    import ray_tracing_octrees_amd as rto
    c = _case("sphere16")
    grid = rto.VoxelGrid.test_sphere(16)
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    rt.setOctreeFromGrid(grid)
    vox = rt.grid()
    ctx.build_octree(vox, grid.min, grid.voxelSize)
    for rule, clip in ((dc.AREA_REFERENCE, None), (dc.AREA_NONE, ((2, 3, 4), (14, 16, 9)))):
        want = ctx.extract_dual_contour(hip.make_dc_params(rule, clip))
        t18, cell, s = rt.dualContour(hip.make_dc_params(rule, clip))
        assert len(want[0]) > 0 and _from18(t18).tobytes() == want[0].tobytes() and np.array_equal(cell, want[1]), rt.lastError
        assert _summary(s) == _summary(want[2])
    idx = np.array([0, 5, vox.size - 1, vox.size, -3], np.int64)
    assert rt.dualVertices(idx).tobytes() == ctx.query_dual_vertices(idx).tobytes()
    assert len(rt.dualContour(hip.make_dc_params(5))[0]) == 0 and "area_rule" in rt.lastError


def _sweep_grid():
    vox = (np.random.default_rng(17).random((27, 28, 100)) < 0.3).astype(np.uint8)
    return vox, np.array([-0.5, -0.25, -0.125], np.float32), np.float32(1.0 / 64)


@pytest.mark.gpu
def test_gpu_clip_boxes_at_the_tile_edges(ctx):
    """A 100 x 28 x 27 seeded grid: box ends on, before and after the tile edges at x = 32 and 64 and y, z = 8 and 16, boxes
    without a cell among them, ordered long list, empty list, short list, so that lists land in buffers made for longer ones."""
    vox, gmin, vs = _sweep_grid()
    ctx.build_octree(vox, gmin, vs)
    whole = _host(vox, gmin, vs, dc.AREA_REFERENCE)
    _same_list(ctx.extract_dual_contour(hip.make_dc_params(dc.AREA_REFERENCE)), (whole[0], whole[1], _summary(whole[2])), "whole")
    boxes = []
    for x0, x1 in ((0, 100), (99, 100), (31, 33), (0, 32), (32, 64), (33, 63), (31, 65), (63, 64), (64, 100), (65, 99)):
        boxes.append(((x0, 0, 0), (x1, 28, 27)))
    for y0, y1 in ((27, 28), (7, 9), (0, 8), (8, 16), (9, 15), (7, 17), (16, 28), (15, 16)):
        boxes.append(((30, y0, 3), (70, y1, 20)))
    for z0, z1 in ((26, 27), (7, 9), (0, 8), (8, 16), (9, 15), (7, 17), (16, 27), (15, 16)):
        boxes.append(((5, 2, z0), (95, 26, z1)))
    boxes += [((31, 7, 7), (32, 8, 8)), ((32, 8, 8), (33, 9, 9)), ((64, 16, 16), (65, 17, 17)), ((99, 27, 26), (100, 28, 27))]
    empties = 0
    for i, clip in enumerate(boxes):
        rule = dc.AREA_NONE if i % 3 == 0 else dc.AREA_REFERENCE
        want = _host(vox, gmin, vs, rule, clip)
        got = ctx.extract_dual_contour(hip.make_dc_params(rule, clip))
        _same_list(got, (want[0], want[1], _summary(want[2])), f"box {clip}")
        empties += len(want[0]) == 0
    assert empties >= 4


@pytest.mark.gpu
def test_gpu_degenerate_triangles_are_written_and_counted(ctx):
    """Voxel sizes at which the squared cross products underflow: at 6e-12 (grid minimum 0) for some triangles of the seeded 12^3
    grid, at 1e-24 for all of the sphere's.  The kernel writes (+0, +0, +0) normals and its summary counts them."""
    c = _case("rand12")
    gmin, vs = np.zeros(3, np.float32), np.float32(6e-12)
    want = dc.extract(c["vox"], gmin, vs, dc.AREA_NONE)
    assert 0 < want[2]["degenerate"] < len(want[0])
    ctx.build_octree(c["vox"], gmin, vs)
    got = ctx.extract_dual_contour(hip.make_dc_params(dc.AREA_NONE))
    _same_list(got, want, "some degenerate")
    zero = (got[0][:, 9:12].view(np.uint32) == 0).all(axis=1)
    assert int(zero.sum()) == got[2].degenerate == want[2]["degenerate"]
    s = _case("sphere16_fine")
    want = dc.extract(s["vox"], s["gmin"], np.float32(1e-24), dc.AREA_NONE)
    assert want[2]["degenerate"] == len(want[0]) == 1344
    ctx.build_octree(s["vox"], s["gmin"], np.float32(1e-24))
    got = ctx.extract_dual_contour(hip.make_dc_params(dc.AREA_NONE))
    _same_list(got, want, "all degenerate")
    assert (got[0][:, 9:12].view(np.uint32) == 0).all()
    none = ctx.extract_dual_contour(hip.make_dc_params(dc.AREA_REFERENCE))
    assert len(none[0]) == 0 and _summary(none[2]) == dict(faces=672, triangles=0, dropped=1344, degenerate=0, vertex_voxels=want[2]["vertex_voxels"])


@pytest.mark.gpu
def test_gpu_sphere64_by_count_and_sha(ctx, orc):
    g = orc.test_sphere_grid(64)
    data = np.asarray(g.data, np.uint8).reshape(64, 64, 64)
    ctx.build_octree(data, g.min, g.voxel_size)
    for rule in (dc.AREA_REFERENCE, dc.AREA_NONE):
        want = _host(data, g.min, g.voxel_size, rule)
        assert len(want[0]) > 10000
        tris, cell, summary = ctx.extract_dual_contour(hip.make_dc_params(rule))
        assert len(tris) == len(want[0]) and _sha(tris) == _sha(want[0]) and _sha(cell) == _sha(want[1])
        assert _summary(summary) == _summary(want[2])
