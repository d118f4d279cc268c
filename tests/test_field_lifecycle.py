"""The lifecycle the resident per-voxel products share (labels, measures, and the distance, geodesic, thickness, skeleton and
exposure fields), as one matrix: which call drops which product, which call keeps them all, and what a refused call or a failed
allocation leaves behind.  The products' values are the subject of their own suites; here every product is made on one small grid
and compared with its CPU rule (tests/*_ref.py) so that "can be made again" means "is right again".

The grid is 40 x 12 x 12: two tiles in x, off the tile in every dimension, dimX and the voxel count no multiples of 16, so every
kernel takes its narrow form.  SOLID: a block x 4..19, y 2..9, z 2..9 and one detached voxel at (30, 6, 6)."""
from __future__ import annotations

import numpy as np
import pytest

import component_ref as cr
import distance_ref as dr
import exposure_ref as er
import geodesic_ref as gr
import measure_ref as mr
import skeleton_ref as sr
import thickness_ref as tr

gpu = pytest.mark.gpu
GMIN, VOX = np.array([-0.5, -0.5, -0.5], np.float32), np.float32(1.0 / 64)
DIRS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.int32)
REACH = 8
THICK_C = 4                                       # a radius of 2 voxels
MESH_VOX = np.float32(0.125)                      # the voxel size of the grid voxelize_mesh makes
FIELDS = ("distance", "geodesic", "thickness", "skeleton", "exposure")


def _hip():
    import ray_tracing_octrees_amd.hip as hip
    return hip


def _grid():
    g = np.zeros((12, 12, 40), np.uint8)
    g[2:10, 2:10, 4:20] = 1
    g[6, 6, 30] = 1
    return g


_REF = {}


def _ref(g):
    """Every product of grid g by the CPU rules, computed once per distinct grid and left unchanged."""
    key = (g.shape, g.tobytes())
    if key not in _REF:
        labels, table = cr.label(g, cr.SET_SOLID, cr.CONN_FACE)
        r = {"labels": labels, "table": table, "measures": mr.measure(labels, len(table), cr.CONN_FACE),
             "distance": dr.field(g, 1), "geodesic": gr.field(g, [0], gr.SET_EMPTY, gr.CONN_FACE),
             "thickness": tr.field(g, 1, THICK_C, dr.separable), "skeleton": sr.skeleton(g)[0],
             "exposure": er.exposure(g, DIRS, None, er.EXPO_SKIN, REACH)[0]}
        r["histogram"] = tr.histogram(r["thickness"], THICK_C)
        r["paths"] = gr.paths(r["geodesic"], gr.CONN_FACE, [0], 4)
        _REF[key] = r
    return _REF[key]


def _same_records(got, want, what):
    assert got.shape == want.shape, what
    for f in want.dtype.names:
        assert np.array_equal(got[f], want[f]), (what, f)


def _make_all(ctx, vox=VOX):
    """Makes the seven products on the resident grid (voxel size vox) and checks each against the rule."""
    hip = _hip()
    r = _ref(ctx.download_voxels())
    _same_records(ctx.label_components(hip.SET_SOLID, hip.CONN_FACE), r["table"], "component table")
    assert np.array_equal(ctx.component_labels(), r["labels"])
    table, total = ctx.measure_components()
    _same_records(table, r["measures"][0], "measures")
    _same_records(np.atleast_1d(total), np.atleast_1d(r["measures"][1]), "total row")
    assert np.array_equal(ctx.distance_field(hip.SET_SOLID)[0], r["distance"])
    assert np.array_equal(ctx.geodesic_field([0], hip.SET_EMPTY, hip.CONN_FACE)[0], r["geodesic"])
    assert np.array_equal(ctx.thickness_field(hip.SET_SOLID, 2 * float(vox))[0], r["thickness"])
    assert np.array_equal(ctx.skeleton_field(hip.SET_SOLID, hip.CONN_FULL, hip.SKEL_TOPOLOGY)[0], r["skeleton"])
    assert np.array_equal(ctx.exposure_field(DIRS, None, hip.EXPO_SKIN, REACH)[0], r["exposure"])
    assert np.array_equal(ctx.thickness_histogram(), r["histogram"])
    rows, lengths = ctx.geodesic_paths([0], 4)
    assert np.array_equal(rows, r["paths"][0]) and np.array_equal(lengths, r["paths"][1])


def _start(ctx):
    hip = _hip()
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(_grid(), GMIN, VOX)
    _make_all(ctx)


def _reads(ctx):
    """Every read of a resident product, by name."""
    return {
        "component_labels": ctx.component_labels, "component_labels_device": ctx.component_labels_device,
        "component_measures": ctx.component_measures, "component_measures_device": ctx.component_measures_device,
        "distance": ctx.distance, "distance_device": ctx.distance_device, "geodesic": ctx.geodesic, "geodesic_device": ctx.geodesic_device,
        "thickness": ctx.thickness, "thickness_device": ctx.thickness_device, "skeleton": ctx.skeleton, "skeleton_device": ctx.skeleton_device,
        "exposure": ctx.exposure, "exposure_device": ctx.exposure_device,
        "geodesic_paths": lambda: ctx.geodesic_paths([0], 4), "thickness_histogram": ctx.thickness_histogram,
    }


def _all_gone(ctx):
    """Every read answers RTO_E_INVALID.  The measures go with the labels, and their own text says so: "the labels have gone since";
    every other read names the cause, "the grid has changed since"."""
    hip = _hip()
    for name, read in _reads(ctx).items():
        with pytest.raises(hip.RtoError) as e:
            read()
        why = "the labels have gone since" if name.startswith("component_measures") else "the grid has changed since"
        assert e.value.code == hip.RTO_E_INVALID and why in str(e.value), (name, str(e.value))


def _snapshot(ctx):
    """The bytes of the seven products and the five fields' device pointers."""
    host = {"labels": ctx.component_labels(), "table": ctx.components(), "measures": ctx.component_measures(), "distance": ctx.distance(),
            "geodesic": ctx.geodesic(), "thickness": ctx.thickness(), "skeleton": ctx.skeleton(), "exposure": ctx.exposure(),
            "histogram": ctx.thickness_histogram()}
    return {k: v.tobytes() for k, v in host.items()}, _pointers(ctx)


def _pointers(ctx):
    return tuple(getattr(ctx, f + "_device")() for f in FIELDS)


# ---------------------------------------------------------------- the drop matrix
def _tetrahedron():
    v = np.array([[0.2, 0.2, 0.2], [0.8, 0.2, 0.2], [0.2, 0.8, 0.2], [0.2, 0.2, 0.8]], np.float64)
    return v, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)


def _corner_brush(hip, op):
    return hip.make_brushes([GMIN + np.float32(0.5) * VOX], 0.5 * float(VOX), hip.BRUSH_SPHERE, op)


# name -> (the call, returning the number of voxels changed or None for a call that replaces the grid; the grid expected
# afterwards as a function of the one before, or None where the call's own suite says what it leaves)
def _changes(hip):
    def fill0(g):
        g = g.copy(); g[0, 0, 0] = 1
        return g

    def no_debris(g):
        g = g.copy(); g[6, 6, 30] = 0
        return g

    def flooded(g):
        g = g.copy(); g[0, 0, 0] = g[0, 0, 1] = g[0, 1, 0] = g[1, 0, 0] = 1
        return g

    def voxelize(ctx):
        ctx.voxelize_mesh(*_tetrahedron(), MESH_VOX, grid=((8, 8, 8), np.zeros(3, np.float32), MESH_VOX))

    return {
        "build_octree": (lambda ctx: ctx.build_octree(_grid(), GMIN, VOX), lambda g: g),
        "voxelize_mesh": (voxelize, None),
        "edit_voxels": (lambda ctx: ctx.edit_voxels(_corner_brush(hip, hip.EDIT_FILL)), fill0),
        "edit_components": (lambda ctx: ctx.edit_components(hip.SET_SOLID, hip.CONN_FACE, hip.SELECT_ALL_BUT_LARGEST), no_debris),
        "edit_morphology": (lambda ctx: ctx.edit_morphology(hip.MORPH_DILATE, float(VOX)), lambda g: dr.morphology(g, dr.DILATE, 64)[0]),
        "edit_geodesic": (lambda ctx: ctx.edit_geodesic([0], hip.SET_EMPTY, hip.CONN_FACE, 1), flooded),
        "edit_skeleton": (lambda ctx: ctx.edit_skeleton(hip.SET_SOLID, hip.CONN_FULL, hip.SKEL_TOPOLOGY), lambda g: sr.edit(g)[0]),
    }


CHANGES = ("build_octree", "voxelize_mesh", "edit_voxels", "edit_components", "edit_morphology", "edit_geodesic", "edit_skeleton")


@gpu
@pytest.mark.parametrize("name", CHANGES)
def test_gpu_a_call_that_changes_the_grid_drops_every_product(ctx, name):
    """All seven products resident; one call that changes or replaces the grid; then every read is refused, and every product can
    be made again and equals the rule on the grid the call left.  Every editing call reports changed > 0."""
    hip = _hip()
    call, after = _changes(hip)[name]
    _start(ctx)
    changed = call(ctx)
    if name.startswith("edit_"):
        assert changed > 0, name
    _all_gone(ctx)
    if after is not None:
        want = after(_grid())
        assert np.array_equal(ctx.download_voxels(), want), name
        if name.startswith("edit_"):
            assert changed == int((want != _grid()).sum()), name
    _make_all(ctx, MESH_VOX if name == "voxelize_mesh" else VOX)


@gpu
def test_gpu_upload_octree_drops_every_product(ctx, scenes):
    """rto_upload_octree replaces the octree and leaves no voxel grid: every read is refused like after any other change, every
    maker is refused for want of a grid (RTO_E_UNSUPPORTED), and after a build of the grid everything can be made again."""
    hip = _hip()
    _start(ctx)
    ctx.upload_octree(scenes("sphere16").nodes, GMIN, VOX)             # any octree; the same origin and voxel size, so that the radii still pass
    _all_gone(ctx)
    makers = (lambda: ctx.label_components(hip.SET_SOLID, hip.CONN_FACE), lambda: ctx.distance_field(hip.SET_SOLID),
              lambda: ctx.geodesic_field([0], hip.SET_EMPTY, hip.CONN_FACE), lambda: ctx.thickness_field(hip.SET_SOLID, 2 * float(VOX)),
              lambda: ctx.skeleton_field(), lambda: ctx.exposure_field(DIRS, None, hip.EXPO_SKIN, REACH))
    for make in makers:
        with pytest.raises(hip.RtoError) as e:
            make()
        assert e.value.code == hip.RTO_E_UNSUPPORTED and "no voxel grid is resident" in str(e.value)
    _all_gone(ctx)
    _start(ctx)


# ---------------------------------------------------------------- edits that change nothing keep everything
@gpu
def test_gpu_an_edit_that_changes_no_voxel_keeps_every_product(ctx):
    """Five edits that return 0: afterwards the seven products read back byte for byte and the five device pointers are the same."""
    hip = _hip()
    g = _grid()
    _start(ctx)
    before = _snapshot(ctx)
    solid = np.flatnonzero(g.reshape(-1) == 1)
    far = hip.make_brushes([GMIN - np.float32(10.0)], 0.5 * float(VOX), hip.BRUSH_SPHERE, hip.EDIT_FILL)
    edits = {
        "a brush outside the grid": lambda: ctx.edit_voxels(far),
        "morphology with radius 0": lambda: ctx.edit_morphology(hip.MORPH_DILATE, 0.0),
        "a flood seeded in the other medium": lambda: ctx.edit_geodesic([0], hip.SET_SOLID, hip.CONN_FACE),
        "thinning with every solid voxel an anchor": lambda: ctx.edit_skeleton(hip.SET_SOLID, hip.CONN_FULL, hip.SKEL_TOPOLOGY, solid),
        "the component of an EMPTY voxel": lambda: ctx.edit_components(hip.SET_SOLID, hip.CONN_FACE, hip.SELECT_CONTAINING, 0),
    }
    for what, edit in edits.items():
        assert edit() == 0, what
        assert _snapshot(ctx) == before, what
    assert np.array_equal(ctx.download_voxels(), g)


# ---------------------------------------------------------------- a maker that fails keeps the old field
def _makers(ctx, hip):
    """field -> (the call that made the resident field, a call the library refuses)."""
    nvox = _grid().size
    return {
        "distance": (lambda: ctx.distance_field(hip.SET_SOLID), lambda: ctx.distance_field(7)),
        "geodesic": (lambda: ctx.geodesic_field([0], hip.SET_EMPTY, hip.CONN_FACE), lambda: ctx.geodesic_field([nvox], hip.SET_EMPTY, hip.CONN_FACE)),
        "thickness": (lambda: ctx.thickness_field(hip.SET_SOLID, 2 * float(VOX)), lambda: ctx.thickness_field(hip.SET_SOLID, 100 * float(VOX))),
        "skeleton": (lambda: ctx.skeleton_field(hip.SET_SOLID, hip.CONN_FULL, hip.SKEL_TOPOLOGY),
                     lambda: ctx.skeleton_field(hip.SET_SOLID, hip.CONN_FACE, hip.SKEL_CURVE)),
        "exposure": (lambda: ctx.exposure_field(DIRS, None, hip.EXPO_SKIN, REACH),
                     lambda: ctx.exposure_field([[1, 0, 0], [0, 0, 0]], None, hip.EXPO_SKIN, REACH)),
    }


def _field_state(ctx, field):
    return getattr(ctx, field)().tobytes(), getattr(ctx, field + "_device")(), getattr(ctx, "last_" + field + "_ms")()


@gpu
@pytest.mark.parametrize("field", FIELDS)
def test_gpu_a_refused_maker_keeps_the_old_field(ctx, field):
    """A seed equal to the voxel count, set = 7, a radius of 100 voxels, SKEL_CURVE with CONN_FACE, a zero direction: the resident
    field's bytes, its device pointer and last_*_ms are what they were."""
    hip = _hip()
    _start(ctx)
    before = _field_state(ctx, field)
    with pytest.raises(hip.RtoError) as e:
        _makers(ctx, hip)[field][1]()
    assert e.value.code == (hip.RTO_E_UNSUPPORTED if field == "thickness" else hip.RTO_E_INVALID), str(e.value)
    assert _field_state(ctx, field) == before
    assert np.array_equal(getattr(ctx, field)(), _ref(_grid())[field])


@gpu
@pytest.mark.parametrize("field", FIELDS)
def test_gpu_a_failed_allocation_keeps_the_old_field(ctx, field):
    """rto_debug_fault_alloc(1): the maker's allocation of its new field fails (a simulated host-side failure; nothing runs on the
    device).  The call answers RTO_E_HIP, the old field reads back byte for byte under the same pointer and times, and the same
    call succeeds once the hook is disarmed."""
    hip = _hip()
    L = hip.load()
    _start(ctx)
    make = _makers(ctx, hip)[field][0]
    before = _field_state(ctx, field)
    try:
        assert L.rto_debug_fault_alloc(1) == 0
        with pytest.raises(hip.RtoError) as e:
            make()
    finally:
        assert L.rto_debug_fault_alloc(0) == 0
    assert e.value.code == hip.RTO_E_HIP, str(e.value)
    assert _field_state(ctx, field) == before
    assert np.array_equal(make()[0], _ref(_grid())[field])
    assert getattr(ctx, field)().tobytes() == before[0]
