"""Field isosurfaces (rto_extract_isosurface_*): marching cubes of an int32 volume of the resident grid.

The expected lists are the reference's own marchingCubesVolume / marchingCubesCell outputs (tests/golden/ref_iso.npz, made by
tests/golden/make_golden_iso.py); tests/iso_ref.py states the rule in numpy float32 and agrees with them byte for byte, so it
serves as the reference wherever the fixture holds a count and a SHA-256 only, and for normals, tri_cell and the summary.

Closedness is asserted on the padded sphere lists only: on noise the classic table's face ambiguities leave the reference's own
list open (372 unmatched edges in its padded 12^3 case at level 3.5), which is documented and not fixed.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

import distance_ref as dr
import iso_ref as ir
from ray_tracing_octrees_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "ref_iso.npz"))
NAMES = [str(n) for n in Z["names"]]
VOLUMES = sorted({str(v) for v in Z["case_volume"]})


def _case(name):
    i = NAMES.index(name)
    vol = str(Z["case_volume"][i])
    p = Z["params"][i]
    clip = None if p[5] == 0 else (tuple(int(v) for v in p[6:9]), tuple(int(v) for v in p[9:12]))
    return dict(name=name, volume=Z[f"vol_{vol}"], gmin=Z[f"min_{vol}"], vs=np.float32(Z[f"vs_{vol}"]), level=np.float32(p[0]),
                outside=np.float32(p[1]), valid=(int(p[2]), int(p[3])), pad=int(p[4]), clip=clip, count=int(Z["counts"][i]),
                sha=bytes(Z["sha256"][i]), verts=Z[f"verts_{name}"] if f"verts_{name}" in Z else None)


def _cases_of(vol):
    return [_case(n) for n, v in zip(NAMES, Z["case_volume"]) if str(v) == vol]


_REF = {}


def _ref(c):
    """iso_ref's answer for a fixture case, computed once."""
    if c["name"] not in _REF:
        _REF[c["name"]] = ir.extract(c["volume"], c["gmin"], c["vs"], c["level"], c["outside"], c["valid"], c["pad"], c["clip"])
    return _REF[c["name"]]


def _params(c, source=hip.FIELD_CALLER):
    return hip.make_iso_params(source, c["level"], c["outside"], c["valid"], bool(c["pad"]), c["clip"])


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()


def _same_list(got, want, what):
    """(tris, tri_cell, summary) against iso_ref's triple, bit for bit."""
    tris, cell, summary = got
    wt, wc, ws = want
    assert tris.shape == wt.shape, f"{what}: {tris.shape} against {wt.shape}"
    assert tris.tobytes() == wt.tobytes(), f"{what}: {int((tris.view(np.uint32) != wt.view(np.uint32)).any(axis=1).sum())} records differ"
    assert np.array_equal(cell, wc), f"{what}: tri_cell"
    assert (summary.triangles, summary.active_cells, summary.degenerate, summary.reserved) == \
        (ws["triangles"], ws["active_cells"], ws["degenerate"], 0), f"{what}: summary"


def _from18(t18):
    """(n, 18) host-layer triangles -> (n, 12) records; the three normals of a triangle are equal."""
    assert (t18[:, 9:12] == t18[:, 12:15]).all() and (t18[:, 9:12] == t18[:, 15:18]).all()
    return np.ascontiguousarray(t18[:, :12])


# ---------------------------------------------------------------- without a GPU
@pytest.mark.parametrize("name", NAMES)
def test_iso_ref_equals_the_reference(name):
    c = _case(name)
    tris, cell, summary = _ref(c)
    assert len(tris) == c["count"] and _sha(tris[:, :9]) == c["sha"]
    if c["verts"] is not None:
        assert tris[:, :9].tobytes() == c["verts"].tobytes()
    assert summary["degenerate"] == int((tris[:, 9:12] == 0).all(axis=1).sum())


@pytest.mark.parametrize("name", NAMES)
def test_host_forms_equal_the_reference(name):
    from ray_tracing_octrees_amd import host
    c = _case(name)
    t18, cell, summary = host.isoSurfaceVolume(c["volume"], c["gmin"], c["vs"], _params(c))
    tris = _from18(t18)
    assert len(tris) == c["count"] and _sha(tris[:, :9]) == c["sha"]
    _same_list((tris, cell, summary), _ref(c), name)
    # the reference's own entry point, under its name: the substituted sample block as its float field
    S, first = ir.samples(c["volume"], c["level"], c["outside"], c["valid"], c["pad"], c["clip"])
    origin = (c["gmin"] + np.float32(0.5) * c["vs"] + first.astype(np.float32) * c["vs"]).astype(np.float32)
    exact = bool((origin == c["gmin"] + np.float32(0.5) * c["vs"]).all())          # a moved origin rounds the positions differently
    m18 = host.marchingCubesVolume(S, origin, c["vs"], c["level"])
    assert len(m18) == c["count"]
    assert (m18[:, 9:] == np.tile(np.array([0, 1, 0], np.float32), 3)).all()      # the placeholder normals
    if exact:
        assert _sha(m18[:, :9]) == c["sha"]


def test_struct_sizes_match_the_header():
    text = open(os.path.join(ROOT, "include", "rto_hip.h")).read()
    assert re.search(r"typedef struct rto_iso_params \{\s*/\* 64 bytes \*/", text)
    assert re.search(r"typedef struct rto_iso_summary \{\s*/\* 32 bytes \*/", text)
    assert C.sizeof(hip.IsoParams) == 64 and C.sizeof(hip.IsoSummary) == 32
    assert hip.IsoParams.level.offset == 12 and hip.IsoParams.clip_lo.offset == 28 and hip.IsoParams.reserved.offset == 52
    for s in ("rto_extract_isosurface_device", "rto_extract_isosurface_host", "rto_isosurface_device", "rto_download_isosurface",
              "rto_last_isosurface_ms"):
        assert s in hip.SYMBOLS and re.search(r"\b%s\(" % s, text)


def test_clip_boxes_partition_the_unpadded_list():
    """Boxes that share their boundary sample planes own disjoint cells; along one axis their lists, merged by cell in raster
    order, are the whole list."""
    c = _case("sphere16_l25_nopad")
    whole, wcell, _ = _ref(c)
    for axis, cuts in ((2, (0, 5, 6, 16)), (1, (0, 9, 16)), (0, (0, 1, 8, 15, 16))):
        parts, cells = [], []
        for a, b in zip(cuts[:-1], cuts[1:]):
            lo, hi = [0, 0, 0], [16, 16, 16]
            lo[axis], hi[axis] = a, min(b + 1, 16)                  # the plane at b belongs to both neighbours
            t, cl, _ = ir.extract(c["volume"], c["gmin"], c["vs"], c["level"], c["outside"], c["valid"], False, (tuple(lo), tuple(hi)))
            parts.append(t); cells.append(cl)
        t, cl = np.concatenate(parts), np.concatenate(cells)
        assert len(np.intersect1d(cells[0], cells[1])) == 0
        order = np.argsort(cl, kind="stable")                      # tri_cell rises in raster order
        assert np.array_equal(cl[order], wcell) and t[order].tobytes() == whole.tobytes(), axis
        if axis == 2:                                               # slabs along z: plain concatenation
            assert t.tobytes() == whole.tobytes()


@pytest.mark.parametrize("name", ["sphere16_l05_pad", "sphere16_l25_pad"])
def test_padded_sphere_lists_are_closed(name):
    tris, _, summary = _ref(_case(name))
    assert len(tris) > 0 and summary["degenerate"] == 0
    assert ir.unmatched_edges(tris) == 0


def test_level_on_a_sample_value_gives_degenerates_and_the_summary_counts_them():
    tris, _, summary = _ref(_case("sphere16_l40_pad"))
    zero = int((tris[:, 9:12].view(np.uint32) == 0).all(axis=1).sum())
    assert 0 < zero < len(tris) and summary["degenerate"] == zero


def test_the_volumes_cover_what_they_are_for():
    assert len(np.unique(ir.cells_of_samples(Z["vol_noise12"].astype(np.float32), 3.5))) == 256
    assert Z["vol_big24"].max() > (1 << 24) and (Z["vol_big24"].astype(np.float32).astype(np.int64) != Z["vol_big24"]).any()
    assert Z["vol_signed"].min() < 0
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ref_iso.npz")) < 100_000


def test_iso_kernels_use_no_private_segment():
    """The built gfx950 code object's metadata: every k_iso_* kernel has a private segment of 0 bytes and spills nothing."""
    import test_isa_contract as isa
    asm = isa.built_asm()
    if asm is None:
        pytest.skip("no hipcc in this environment")
    meta = isa.kernel_meta(asm)
    names = [k for k in meta if "k_iso_" in k]
    for want in ("k_iso_bricks", "k_iso_count", "k_iso_sums", "k_iso_scan_sums", "k_iso_offsets", "k_iso_place", "k_iso_emit"):
        assert any(want in k for k in names), want
    assert len(names) == 7, names
    for k in names:
        m = meta[k]
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (k, m)


def test_stl_round_trip_of_an_isosurface(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mesh_export as me
    tris = _ref(_case("sphere16_l40_pad"))[0]                         # zero normals included
    path = str(tmp_path / "iso.stl")
    me.write_stl(path, tris)
    assert os.path.getsize(path) == 84 + 50 * len(tris) and me.read_stl(path).tobytes() == tris.tobytes()


# ---------------------------------------------------------------- on the GPU
def _resident(ctx, c):
    """A resident grid of the case's dims (the voxels do not enter a CALLER extraction)."""
    ctx.build_octree((c["volume"] & 1).astype(np.uint8), c["gmin"], c["vs"])


@pytest.mark.gpu
@pytest.mark.parametrize("vol", VOLUMES)
def test_gpu_caller_volumes_equal_the_rule(ctx, vol):
    import torch
    cases = _cases_of(vol)
    _resident(ctx, cases[0])
    d_vol = torch.from_numpy(np.ascontiguousarray(cases[0]["volume"])).cuda()
    for c in cases:
        want = _ref(c)
        got = ctx.extract_isosurface(_params(c), c["volume"])
        assert len(got[0]) == c["count"] and _sha(got[0][:, :9]) == c["sha"], c["name"]
        _same_list(got, want, c["name"] + " host volume")
        _same_list(ctx.extract_isosurface(_params(c), d_vol), want, c["name"] + " device volume")
        _same_list(ctx.extract_isosurface(_params(c), int(d_vol.data_ptr())), want, c["name"] + " device pointer")
        ms = ctx.last_isosurface_ms()
        assert len(ms) == 3 and (all(m >= 0 for m in ms) if c["name"] != "thin1_l35_nopad" else tuple(ms) == (-1.0, -1.0, -1.0))   # no cell, no kernel
        _, _, n = ctx.isosurface_device()
        assert n == c["count"]


def _sphere(orc, ctx, dim):
    g = orc.test_sphere_grid(dim)
    data = np.asarray(g.data, np.uint8).reshape(dim, dim, dim)
    ctx.build_octree(data, g.min, g.voxel_size)
    return g, data


def _named_fields(ctx, dim, vs):
    """(source, level, outside, valid, the field as its own entry point made and returned it)"""
    out = [(hip.FIELD_DISTANCE, 2.5, 0.0, (0, 0x7ffffffe), ctx.distance_field(hip.SET_EMPTY)[0]),
           (hip.FIELD_THICKNESS, 0.5, 0.0, (0, 0x7ffffffe), ctx.thickness_field(hip.SET_SOLID, 6 * float(vs))[0]),
           (hip.FIELD_GEODESIC, 6.5, 1.0e6, (0, 0x7ffffffe), ctx.geodesic_field(np.array([0], np.int64), hip.SET_EMPTY, hip.CONN_FACE)[0]),
           (hip.FIELD_SKELETON, 0.5, 9.0, (0, 0x7ffffffe), ctx.skeleton_field()[0])]
    ctx.label_components(hip.SET_SOLID, hip.CONN_FACE)
    labels = ctx.component_labels()              # the surface around the labelled voxels: every label above the level, -1 below
    out.append((hip.FIELD_LABELS, float(labels[labels >= 0].min()) - 0.5, -1.0, (0, 0x7ffffffe), labels))
    ctx.segment_parts(hip.SET_SOLID, hip.CONN_FACE)
    parts = ctx.part_labels()
    out.append((hip.FIELD_PARTS, float(parts[parts >= 0].min()) - 0.5, -1.0, (0, 0x7ffffffe), parts))
    out.append((hip.FIELD_EXPOSURE, 0.5, 0.0, (0, 0x7ffffffe), ctx.exposure_field(np.array([[0, 0, 1], [1, 0, 0], [0, -1, 0]], np.int32))[0]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [16, 32])
def test_gpu_named_sources_equal_the_rule_on_the_downloaded_field(ctx, orc, dim):
    g, _ = _sphere(orc, ctx, dim)
    for source, level, outside, valid, field in _named_fields(ctx, dim, g.voxel_size):
        for pad in (True, False):
            p = hip.make_iso_params(source, level, outside, valid, pad)
            want = ir.extract(field, g.min, g.voxel_size, level, outside, valid, pad)
            assert len(want[0]) > 0, source
            _same_list(ctx.extract_isosurface(p), want, f"sphere{dim} source {source} pad {pad}")


@pytest.mark.gpu
def test_gpu_same_lists_in_every_state_of_the_context(ctx, orc):
    """Both octree build paths, a frustum update in force, the brick table on and off: one list."""
    g = orc.test_sphere_grid(32)
    data = np.asarray(g.data, np.uint8).reshape(32, 32, 32)
    d2 = dr.field(data, dr.SET_EMPTY)
    want = {pad: ir.extract(d2, g.min, g.voxel_size, 2.5, 0.0, pad=pad, clip=clip) for pad, clip in ((True, None), (False, ((3, 0, 5), (30, 32, 31))))}
    cam = orc.Camera(0.5, 0.7, 0.6)
    try:
        for level_by_level in (False, True):
            ctx.debug_set_build_path(level_by_level)
            ctx.build_octree(data, g.min, g.voxel_size)
            assert np.array_equal(ctx.distance_field(hip.SET_EMPTY)[0], d2)
            for frustum in (False, True):
                ctx.update_frustum(cam.get_view(), 45.0, 4.0 / 3.0, frustum)
                for table in (True, False):
                    ctx.debug_set_projection_table(table)
                    for pad, clip in ((True, None), (False, ((3, 0, 5), (30, 32, 31)))):
                        what = f"path {level_by_level} frustum {frustum} table {table} pad {pad}"
                        _same_list(ctx.extract_isosurface(hip.make_iso_params(hip.FIELD_DISTANCE, 2.5, 0.0, pad=pad, clip=clip)), want[pad], what)
                        _same_list(ctx.extract_isosurface(hip.make_iso_params(hip.FIELD_CALLER, 2.5, 0.0, pad=pad, clip=clip), d2), want[pad], what + " CALLER")
    finally:
        ctx.debug_set_projection_table(True)
        ctx.debug_set_build_path(False)
        ctx.update_frustum(cam.get_view(), 45.0, 4.0 / 3.0, False)


@pytest.mark.gpu
def test_gpu_no_output_depends_on_the_brick_table(ctx):
    """Every fixture case of the volumes with uniform stretches, and a distance field most of whose tiles the level does not
    cross, with the table on and off."""
    try:
        for vol in ("sphere16", "noise12", "long200", "edge34", "signed"):
            cases = _cases_of(vol)
            _resident(ctx, cases[0])
            for c in cases:
                for table in (True, False):
                    ctx.debug_set_projection_table(table)
                    _same_list(ctx.extract_isosurface(_params(c), c["volume"]), _ref(c), f"{c['name']} table {table}")
    finally:
        ctx.debug_set_projection_table(True)


@pytest.mark.gpu
def test_gpu_after_voxelize_and_after_an_edit(ctx):
    # a box mesh, voxelized on the GPU
    lo, hi = np.array([-3.0, -2.0, -1.5]), np.array([3.0, 2.0, 1.5])
    xyz = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for k in (0, 1) for j in (0, 1) for i in (0, 1)], np.float64)
    tris = np.array([(0, 1, 3), (0, 3, 2), (4, 7, 5), (4, 6, 7), (0, 5, 1), (0, 4, 5), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)], np.int32)
    r = ctx.voxelize_mesh(xyz, tris, 0.5)
    gmin, vs = np.array(list(r.grid_min), np.float32), np.float32(r.voxel_size)
    grid = ctx.download_voxels()
    assert grid.any()
    p = hip.make_iso_params(hip.FIELD_DISTANCE, 2.5, 1.0e6)
    d2 = ctx.distance_field(hip.SET_SOLID)[0]
    assert np.array_equal(d2, dr.field(grid, dr.SET_SOLID))
    want = ir.extract(d2, gmin, vs, 2.5, 1.0e6)
    assert len(want[0]) > 0
    _same_list(ctx.extract_isosurface(p), want, "after voxelize_mesh")
    # an edit: the snapshot survives, the named source is refused in its reader's words, CALLER still works
    centre = (gmin + vs * np.array(grid.shape[::-1], np.float32) * np.float32(0.5)).astype(np.float32)
    assert ctx.edit_voxels(hip.make_brushes([centre], 2 * float(vs), hip.BRUSH_SPHERE, hip.EDIT_CARVE)) > 0
    tris_after, cell_after = ctx.download_isosurface()
    assert tris_after.tobytes() == want[0].tobytes() and np.array_equal(cell_after, want[1])
    with pytest.raises(hip.RtoError) as e:
        ctx.extract_isosurface(p)
    assert e.value.code == hip.RTO_E_INVALID and "no distance field is resident" in str(e.value)
    assert ctx.download_isosurface()[0].tobytes() == want[0].tobytes()
    _same_list(ctx.extract_isosurface(hip.make_iso_params(hip.FIELD_CALLER, 2.5, 1.0e6), d2), want, "CALLER after the edit")
    edited = ctx.download_voxels()
    d2e = ctx.distance_field(hip.SET_SOLID)[0]
    assert np.array_equal(d2e, dr.field(edited, dr.SET_SOLID)) and not np.array_equal(d2e, d2)
    _same_list(ctx.extract_isosurface(p), ir.extract(d2e, gmin, vs, 2.5, 1.0e6), "the field made after the edit")


@pytest.mark.gpu
def test_gpu_errors_in_their_order_leave_the_previous_isosurface(orc):
    import ray_tracing_octrees_amd as rto
    ctx = rto.Context(0)
    try:
        c = _case("sphere16_l25_pad")
        vol = c["volume"]
        ok = _params(c)

        def refused(code, params, volume=None, text=None):
            with pytest.raises(hip.RtoError) as e:
                ctx.extract_isosurface(params, volume)
            assert e.value.code == code, (e.value.code, str(e.value))
            if text:
                assert text in str(e.value)

        def bad(**kw):
            p = _params(c)
            for k, v in kw.items():
                if k in ("clip_lo", "clip_hi"):
                    for a in range(3):
                        getattr(p, k)[a] = v[a]
                elif k == "reserved":
                    p.reserved[v] = 1
                else:
                    setattr(p, k, v)
            return p

        # 1. RTO_E_INVALID comes before "nothing uploaded"
        refused(hip.RTO_E_INVALID, None, vol)
        refused(hip.RTO_E_INVALID, ok, None, "needs a volume")
        with pytest.raises(hip.RtoError) as e:          # a misaligned device pointer
            ctx.extract_isosurface(ok, 0x1002)
        assert e.value.code == hip.RTO_E_INVALID and "aligned" in str(e.value)
        refused(hip.RTO_E_INVALID, bad(source=8), vol, "unknown source")
        refused(hip.RTO_E_INVALID, bad(source=-1), vol, "unknown source")
        refused(hip.RTO_E_INVALID, bad(reserved=2), vol, "reserved")
        refused(hip.RTO_E_INVALID, bad(valid_lo=5, valid_hi=4), vol, "valid_lo")
        refused(hip.RTO_E_INVALID, bad(valid_lo=-2147483647), vol, "valid_lo")
        refused(hip.RTO_E_INVALID, bad(level=float("nan")), vol, "finite")
        refused(hip.RTO_E_INVALID, bad(outside=float("inf")), vol, "finite")
        refused(hip.RTO_E_INVALID, bad(pad=2), vol, "pad")
        refused(hip.RTO_E_INVALID, bad(source=hip.FIELD_DISTANCE), vol, "RTO_FIELD_CALLER only")
        # 2. RTO_E_NO_OCTREE, before the clip box is looked at
        refused(hip.RTO_E_NO_OCTREE, bad(clip=1, clip_lo=(5, 5, 5), clip_hi=(2, 2, 2)), vol)
        with pytest.raises(hip.RtoError):
            ctx.download_isosurface()
        # 3. RTO_E_UNSUPPORTED without a resident grid, before the clip box and the source
        g = orc.test_sphere_grid(16)
        ctx.upload_octree(orc.build_flat_octree(g), g.min, g.voxel_size)
        refused(hip.RTO_E_UNSUPPORTED, bad(clip=1, clip_lo=(5, 5, 5), clip_hi=(2, 2, 2)), vol, "no voxel grid is resident")
        refused(hip.RTO_E_UNSUPPORTED, bad(source=hip.FIELD_DISTANCE), None)
        refused(hip.RTO_E_INVALID, bad(pad=3, clip=1, clip_lo=(5, 5, 5), clip_hi=(2, 2, 2)), vol, "pad")
        # a good extraction, then every refusal again: the list stays
        _resident(ctx, c)
        want = _ref(c)
        _same_list(ctx.extract_isosurface(ok, vol), want, "before the refusals")
        # 4. the clip box, then the source that is not resident
        for lo, hi in (((-1, 0, 0), (4, 4, 4)), ((0, 0, 0), (4, 17, 4)), ((3, 3, 3), (4, 4, 3))):
            refused(hip.RTO_E_INVALID, bad(clip=1, clip_lo=lo, clip_hi=hi), vol, "clip box")
        refused(hip.RTO_E_INVALID, bad(source=hip.FIELD_THICKNESS, clip=1, clip_lo=(0, 0, 0), clip_hi=(0, 4, 4)), None, "clip box")
        refused(hip.RTO_E_INVALID, bad(source=hip.FIELD_THICKNESS), None, "no thickness field is resident")
        refused(hip.RTO_E_INVALID, bad(source=hip.FIELD_LABELS), None, "no labels are resident")
        refused(hip.RTO_E_INVALID, bad(pad=-1), vol, "pad")
        refused(hip.RTO_E_INVALID, None, vol)
        tris, cell = ctx.download_isosurface()
        assert tris.tobytes() == want[0].tobytes() and np.array_equal(cell, want[1])
        # download: the capacity
        n = C.c_int64()
        buf = np.zeros((4, 12), np.float32)
        assert ctx._L.rto_download_isosurface(ctx._h, buf.ctypes.data, 4, None, C.byref(n)) == hip.RTO_E_INVALID and n.value == len(want[0])
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_the_mesh_and_the_isosurface_keep_buffers_of_their_own(ctx, orc):
    g, data = _sphere(orc, ctx, 16)
    ctx.build_leaf_triangles(None)
    mesh = ctx.extract_mesh(hip.MESH_MC)
    assert len(mesh[0]) > 0
    d2 = dr.field(data, dr.SET_EMPTY)
    want = ir.extract(d2, g.min, g.voxel_size, 2.5, 0.0)
    _same_list(ctx.extract_isosurface(hip.make_iso_params(hip.FIELD_CALLER, 2.5, 0.0), d2), want, "sphere16")
    again = ctx.download_mesh()
    assert again[0].tobytes() == mesh[0].tobytes() and np.array_equal(again[1], mesh[1])
    cubes = ctx.extract_mesh(hip.MESH_CUBES)
    assert len(cubes[0]) > 0 and len(cubes[0]) != len(want[0])
    tris, cell = ctx.download_isosurface()
    assert tris.tobytes() == want[0].tobytes() and np.array_equal(cell, want[1])
    assert ctx.mesh_device()[0] != ctx.isosurface_device()[0]


@pytest.mark.gpu
def test_gpu_host_class_equals_the_python_path(ctx, orc):
    import ray_tracing_octrees_amd as rto
    grid = rto.VoxelGrid.test_sphere(16)
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    rt.setOctreeFromGrid(grid)
    g, data = _sphere(orc, ctx, 16)
    d2 = dr.field(data, dr.SET_EMPTY)
    for pad in (True, False):
        want, _, _ = ctx.extract_isosurface(hip.make_iso_params(hip.FIELD_CALLER, 2.5, 0.0, pad=pad), d2)
        got = _from18(rt.isoSurface(hip.FIELD_CALLER, 2.5, 0.0, pad, d2))
        assert len(got) > 0 and got.tobytes() == want.tobytes(), rt.lastError
    ctx.distance_field(hip.SET_SOLID)
    want, _, _ = ctx.extract_isosurface(hip.make_iso_params(hip.FIELD_DISTANCE, 6.25, 1.0e9))
    got = _from18(rt.offsetSurface(2.5))
    assert len(got) > 0 and got.tobytes() == want.tobytes(), rt.lastError
    assert len(rt.isoSurface(hip.FIELD_THICKNESS, 4.5)) == 0 and "no thickness field is resident" in rt.lastError


@pytest.mark.gpu
def test_gpu_sphere64_by_count_and_sha(ctx, orc):
    """A level that crosses many tiles of a 64^3 field: 3 x 9 x 9 tiles under pad, runs of every length."""
    g, data = _sphere(orc, ctx, 64)
    d2 = ctx.distance_field(hip.SET_EMPTY)[0]
    assert np.array_equal(d2, dr.field(data, dr.SET_EMPTY))
    want = ir.extract(d2, g.min, g.voxel_size, 12.5, 0.0)
    assert len(want[0]) > 20000
    tris, cell, summary = ctx.extract_isosurface(hip.make_iso_params(hip.FIELD_DISTANCE, 12.5, 0.0))
    assert len(tris) == len(want[0]) and _sha(tris) == _sha(want[0]) and _sha(cell) == _sha(want[1])
    assert (summary.triangles, summary.active_cells, summary.degenerate) == (len(tris), want[2]["active_cells"], 0)


def _d2h(ptr, nbytes):
    L = hip.load()
    out = np.zeros(nbytes, np.uint8)
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert L.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), nbytes, 2) == 0          # hipMemcpyDeviceToHost
    return out


@pytest.mark.gpu
def test_gpu_more_than_2_to_the_23_active_runs(ctx):
    """The runs that hold a triangle are ranked in a word of their own: 2900 x 2900 = 8,410,000 > 2^23 of them, which a count packed
    above 40 bits of a signed 64-bit word would not hold.  A 2 x 2901 x 2901 volume without pad has one cell a run; the value 0
    at x = 0 and even y and z, 7 elsewhere, puts exactly one corner of every cell below the level: one triangle a cell.  tri_cell
    and the summary are checked in full, the records on three slabs of z (the first, the last and the one that holds offset 2^23)
    against iso_ref of the slab as a clip box."""
    N = 2901
    vol = np.full((N, N, 2), 7, np.int32)
    vol[::2, ::2, 0] = 0
    gmin, vs = np.array([-0.5, -0.5, -0.5], np.float32), np.float32(1.0 / 4096)
    ctx.build_octree(np.zeros((N, N, 2), np.uint8), gmin, vs)
    summary = ctx.extract_isosurface_count(hip.make_iso_params(hip.FIELD_CALLER, 3.5, 0.0, pad=False), vol)
    runs = (N - 1) * (N - 1)
    assert runs > 1 << 23
    assert (summary.triangles, summary.active_cells, summary.degenerate) == (runs, runs, 0)
    d_tris, d_cell, n = ctx.isosurface_device()
    assert n == runs
    cell = _d2h(d_cell, 4 * n).view(np.int32)
    z, y = np.divmod(np.arange(runs, dtype=np.int64), N - 1)
    assert np.array_equal(cell, (((z + 1) * (N + 1) + (y + 1)) * 3 + 1).astype(np.int32))
    for z0 in (0, (1 << 23) // (N - 1), N - 2):
        want, wcell, _ = ir.extract(vol, gmin, vs, 3.5, 0.0, pad=False, clip=((0, 0, z0), (2, N, z0 + 2)))
        first = z0 * (N - 1)
        assert len(want) == N - 1 and np.array_equal(wcell, cell[first:first + N - 1])
        assert _d2h(d_tris + 48 * first, 48 * (N - 1)).tobytes() == want.tobytes(), z0
