"""Mesh extraction (rto_extract_mesh, Context.extract_mesh, RayTracerBVH::extractMesh): the triangle lists
of the reference's renderOctree for MarchingCubesRenderer and VoxelCubeRenderer.  CPU: the float32 statement of the rule
(tests/mesh_ref.py) and the host layer's VoxelCubeRenderer / renderOctree against lists made by the reference's own code
(tests/golden/ref_mesh_extract.npz), the order property, the ABI's layout, the plane helper, the STL round trip, the built kernels'
private segments.  GPU: the lists against that statement, byte for byte, on every build path that can leave an octree resident."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_ref as mr
from conftest import GOLDEN, ROOT, SPHERE_CAM, make_camera

sys.path.insert(0, os.path.join(ROOT, "tools"))

KINDS = ((mr.MESH_MC, "mc"), (mr.MESH_CUBES, "cubes"))
_Z = np.load(os.path.join(GOLDEN, "ref_mesh_extract.npz"))
NAMES = [str(n) for n in _Z["names"]]


class Case:
    """One golden grid with the oracle's octree and leaf triangles, made once and never changed."""

    def __init__(self, orc, name):
        z = _Z
        self.name = name
        self.dims = tuple(int(x) for x in z[f"{name}_dims"])
        dx, dy, dz = self.dims
        self.data = np.unpackbits(z[f"{name}_packed"])[: dx * dy * dz].reshape(dz, dy, dx).astype(np.uint8)
        self.min = z[f"{name}_min"].astype(np.float32)
        self.vs = np.float32(z[f"{name}_vs"])
        self.sets = [str(s) for s in z[f"{name}_sets"]]
        self.planes = [z[f"{name}_planes"][i] if z[f"{name}_has_planes"][i] else None for i in range(len(self.sets))]
        self.margins = [float(m) for m in z[f"{name}_margins"]]
        self.counts = z[f"{name}_counts"]
        self.sha = z[f"{name}_sha256"]
        self.grid = orc.Grid(self.dims, self.min, self.vs, self.data)
        self.nodes = orc.build_flat_octree(self.grid)
        self.tris, self.off = orc.build_leaf_triangles(self.grid, self.nodes)
        self._ref = {}

    def ref(self, kind, si):
        if (kind, si) not in self._ref:
            self._ref[(kind, si)] = mr.extract(kind, self.nodes, self.min, self.vs, data=self.data, tris=self.tris, tri_offset=self.off,
                                               planes=self.planes[si], margin=self.margins[si])
        return self._ref[(kind, si)]

    def check_golden(self, got, kind, kname, si, what):
        assert len(got) == self.counts[si, kind], (what, self.name, self.sets[si], kname, len(got), int(self.counts[si, kind]))
        assert hashlib.sha256(got.tobytes()).digest() == self.sha[si, kind].tobytes(), (what, self.name, self.sets[si], kname)
        key = f"{self.name}_{self.sets[si]}_{kname}"
        if key in _Z:
            assert got.tobytes() == _Z[key].tobytes(), (what, key)


@pytest.fixture(scope="module")
def cases(orc):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Case(orc, name)
        return cache[name]
    return get


def _rec12(t18):
    """(n, 18) v0, v1, v2, n0, n1, n2 -> (n, 12) v0, v1, v2, n0 after checking that the three normals are bitwise equal."""
    t18 = np.asarray(t18, np.float32).reshape(-1, 18)
    assert t18[:, 9:12].tobytes() == t18[:, 12:15].tobytes() == t18[:, 15:18].tobytes()
    return np.ascontiguousarray(t18[:, :12])


# ================================================================ without a GPU
@pytest.mark.parametrize("name", NAMES)
def test_numpy_rule_equals_the_reference_lists(cases, name):
    c = cases(name)
    for si in range(len(c.sets)):
        for kind, kname in KINDS:
            c.check_golden(c.ref(kind, si)[0], kind, kname, si, "mesh_ref")


@pytest.mark.parametrize("name", NAMES)
def test_host_layer_walk_equals_the_reference_lists(cases, name):
    """host/Renderer.cpp: VoxelCubeRenderer, MarchingCubesRenderer and renderOctree's walk through host_capi."""
    from ray_tracing_octrees_amd import host
    c = cases(name)
    grid = host.VoxelGrid.from_array(c.data, c.min, c.vs)
    root = host.createOctreeFromVoxelGrid(grid)
    try:
        for kind, kname in KINDS:
            r = host.MarchingCubesRenderer() if kind == mr.MESH_MC else host.VoxelCubeRenderer()
            for si in range(len(c.sets)):
                got = _rec12(host.renderOctreePlanes(root, grid, r, c.planes[si], c.margins[si]))
                c.check_golden(got, kind, kname, si, "renderOctreePlanes")
            c.check_golden(_rec12(r.render(root, grid)), kind, kname, 0, "Renderer.render")
    finally:
        host.freeOctree(root)


def test_host_render_octree_takes_the_cameras_own_frustum(cases, orc):
    """renderOctree(root, grid, renderer, camera, aspect, margin) = the walk over Frustum(perspective(45, aspect, 0.01, 5000) * view)."""
    from ray_tracing_octrees_amd import hip, host
    c = cases("sphere16")
    grid = host.VoxelGrid.from_array(c.data, c.min, c.vs)
    root = host.createOctreeFromVoxelGrid(grid)
    cam = host.Camera(0.5, 0.7, 0.9)
    planes = hip.frustum_planes(cam.getView(), 45.0, 4.0 / 3.0)
    try:
        for r in (host.MarchingCubesRenderer(), host.VoxelCubeRenderer()):
            a = host.renderOctree(root, grid, r, cam, 4.0 / 3.0, 0.0)
            b = host.renderOctreePlanes(root, grid, r, planes, 0.0)
            assert len(a) and a.tobytes() == b.tobytes()
            if isinstance(r, host.MarchingCubesRenderer):                              # this camera culls some of the surface
                assert len(a) < len(host.renderOctreePlanes(root, grid, r, None, 0.0))
    finally:
        host.freeOctree(root)


@pytest.mark.parametrize("name", NAMES)
def test_depth_first_order_is_morton_order(cases, name):
    """Property of the lists: the owning leaves appear in ascending Morton order of their corners (x in the lowest bit)."""
    c = cases(name)
    for kind, _ in KINDS:
        for si in range(len(c.sets)):
            owner = c.ref(kind, si)[1]
            if len(owner) == 0:
                continue
            leaves = owner[np.concatenate([[True], owner[1:] != owner[:-1]])]
            assert len(set(leaves.tolist())) == len(leaves)                            # a leaf's triangles are contiguous
            code = mr.morton(c.nodes["x"][leaves], c.nodes["y"][leaves], c.nodes["z"][leaves])
            assert (code[1:] > code[:-1]).all(), (name, c.sets[si])


def test_centre_only_rule_and_special_cases(cases):
    """The reference tests one voxel per face: the 8^3 leaf's +X face (x = 0) is absent when that voxel is FILLED, present when the
    FILLED voxel sits one off the centre; one solid leaf gives 12 triangles; an empty grid none."""
    def plus_x_at_zero(t):
        return int(((t[:, 9] == 1.0) & (t[:, 0] == 0.0) & (t[:, 3] == 0.0) & (t[:, 6] == 0.0)).sum())
    assert plus_x_at_zero(cases("centre_covered").ref(mr.MESH_CUBES, 0)[0]) == 0
    assert plus_x_at_zero(cases("centre_open").ref(mr.MESH_CUBES, 0)[0]) == 2
    full = cases("full8")
    assert len(full.nodes) == 1 and len(full.ref(mr.MESH_CUBES, 0)[0]) == 12
    assert len(cases("empty8").ref(mr.MESH_CUBES, 0)[0]) == 0 and len(cases("empty8").ref(mr.MESH_MC, 0)[0]) == 0
    assert (cases("checker8").nodes["size"][cases("checker8").nodes["isLeaf"] == 1] == 1).all()
    assert cases("long200").nodes["size"][0] == 256
    s = cases("sphere16")
    partial = [si for si, n in enumerate(s.sets) if n.startswith("rand")
               and all(0.1 * s.counts[0, k] < s.counts[0, k] - s.counts[si, k] < 0.9 * s.counts[0, k] for k in range(2))]
    assert len(partial) >= 2
    assert (s.counts[s.sets.index("cam_m50")] == s.counts[0]).all() and (s.counts[s.sets.index("rootcull")] == 0).all()


def test_abi_layout_and_symbols():
    from ray_tracing_octrees_amd import hip
    assert C.sizeof(hip.MeshCull) == 100
    header = os.path.join(ROOT, "include", "rto_hip.h")
    src = '#include "rto_hip.h"\n_Static_assert(sizeof(rto_mesh_cull) == 100, "rto_mesh_cull");\n' \
          '_Static_assert(RTO_MESH_MC == 0 && RTO_MESH_CUBES == 1, "kinds");\n'
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.dirname(header), "-x", "c", "-"], input=src.encode(), check=True)
    text = open(header).read()
    L = hip.load()
    for s in ("rto_frustum_planes", "rto_extract_mesh", "rto_mesh_device", "rto_download_mesh", "rto_last_mesh_ms"):
        assert s in hip.SYMBOLS and hasattr(L, s) and s + "(" in text, s
    assert (hip.MESH_MC, hip.MESH_CUBES) == (0, 1)


def test_frustum_planes_are_the_update_frustums(orc, golden):
    """rto_frustum_planes = Frustum(perspective(radians(fov), aspect, 0.01, 5000) * view) as the oracle and the reference's stored
    view-projection matrices give it."""
    from ray_tracing_octrees_amd import hip
    z = golden("ref_cameras.npz")
    for cam in ("sphere", "calgary_default", "calgary_oblique", "panned"):
        view, persp, vp = z[f"{cam}_view"], z[f"{cam}_persp"], z[f"{cam}_vp"]
        aspect = float(np.float32(persp[5]) / np.float32(persp[0]))
        got = hip.frustum_planes(view, 45.0, aspect)
        mine = orc.mat4_mul(orc.perspective(orc.radians(45.0), aspect, 0.01, 5000.0), view)
        if mine.tobytes() == vp.astype(np.float32).tobytes():                         # the stored matrix is this aspect's
            assert got.tobytes() == orc.frustum_planes(vp).tobytes(), cam
        assert got.tobytes() == orc.frustum_planes(mine).tobytes(), cam
    for aspect, fov in ((4.0 / 3.0, 45.0), (16.0 / 9.0, 60.0)):
        view, _ = make_camera(orc, *SPHERE_CAM)
        want = orc.frustum_planes(orc.mat4_mul(orc.perspective(orc.radians(fov), aspect, 0.01, 5000.0), view))
        assert hip.frustum_planes(view, fov, aspect).tobytes() == want.tobytes()
    assert hip.load().rto_frustum_planes(None, 45.0, 1.0, None) == hip.RTO_E_INVALID


def test_stl_round_trip(cases, tmp_path):
    import mesh_export as me
    tris = cases("noncubic").ref(mr.MESH_CUBES, 0)[0]
    path = str(tmp_path / "m.stl")
    me.write_stl(path, tris)
    assert os.path.getsize(path) == 84 + 50 * len(tris)
    raw = open(path, "rb").read()
    assert np.frombuffer(raw[80:84], "<u4")[0] == len(tris)
    assert raw[84:96] == tris[0, 9:12].tobytes() and raw[96:132] == tris[0, 0:9].tobytes()       # normal first, then v0, v1, v2
    assert me.read_stl(path).tobytes() == tris.tobytes()
    me.write_stl(path, np.zeros((0, 12), np.float32))
    assert me.read_stl(path).shape == (0, 12)


def test_mesh_kernels_use_no_private_segment():
    """The built gfx950 code object's metadata: every k_mesh_* kernel has a private segment of 0 bytes and spills nothing."""
    import test_isa_contract as isa
    asm = isa.built_asm()
    if asm is None:
        pytest.skip("no hipcc in this environment")
    meta = isa.kernel_meta(asm)
    names = [k for k in meta if "k_mesh_" in k]
    for want in ("k_mesh_levels", "k_mesh_count", "k_mesh_sum_level", "k_mesh_offset_level", "k_mesh_emit_mc", "k_mesh_emit_cubes"):
        assert any(want in k for k in names), want
    assert len(names) == 7, names                                     # k_mesh_count once per kind
    for k in names:
        m = meta[k]
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (k, m)


# ================================================================ on the GPU
def _d2h(ptr, nbytes):
    from ray_tracing_octrees_amd import hip
    L = hip.load()
    out = np.zeros(nbytes, np.uint8)
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert L.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), nbytes, 2) == 0          # hipMemcpyDeviceToHost
    return out


def _check_owner(case_nodes, gmin, vs, tris, owner, kind, off=None, src=None):
    """Each triangle lies in its node's box; MC triangles are their node's resident range, in order."""
    if len(tris) == 0:
        return
    nd = case_nodes[owner]
    assert (nd["isLeaf"] == 1).all()
    lo = np.asarray(gmin, np.float64)[None, :] + np.stack([nd["x"], nd["y"], nd["z"]], 1) * float(vs)
    hi = lo + nd["size"][:, None] * float(vs)
    eps = 1e-4 * float(vs) * float(case_nodes["size"][0])
    pad = float(vs) if kind == mr.MESH_MC else 0.0                   # localMC's cells reach one voxel past the leaf's far faces
    for v in range(3):
        p = tris[:, 3 * v:3 * v + 3].astype(np.float64)
        assert (p >= lo - eps).all() and (p <= hi + pad + eps).all()
    if kind == mr.MESH_MC:
        first = np.concatenate([[True], owner[1:] != owner[:-1]])
        start = np.maximum.accumulate(np.where(first, np.arange(len(owner)), 0))
        srcidx = off[owner] + (np.arange(len(owner)) - start)
        assert (srcidx < off[owner + 1]).all()
        assert tris.tobytes() == src[srcidx].tobytes()
    else:
        assert (nd["isSolid"] == 1).all()


def _resident(ctx, c, triangles=True):
    ctx.build_octree(c.data, c.min, c.vs)
    if triangles:
        ctx.build_leaf_triangles()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_lists_equal_the_rule(ctx, cases, name):
    from ray_tracing_octrees_amd import hip
    c = cases(name)
    _resident(ctx, c)
    assert ctx.download_nodes().tobytes() == c.nodes.tobytes()
    for kind, kname in KINDS:
        for si in range(len(c.sets)):
            want, wnode = c.ref(kind, si)
            got, gnode = ctx.extract_mesh(kind, c.planes[si], c.margins[si])
            assert got.tobytes() == want.tobytes(), (name, kname, c.sets[si], got.shape, want.shape)
            assert gnode.tobytes() == wnode.tobytes(), (name, kname, c.sets[si])
            c.check_golden(got, kind, kname, si, "rto_extract_mesh")
            _check_owner(c.nodes, c.min, c.vs, got, gnode, kind, c.off, c.tris)
            d_t, d_n, n = ctx.mesh_device()
            assert n == len(want)
            if n:
                assert _d2h(d_t, 48 * n).tobytes() == got.tobytes() and _d2h(d_n, 4 * n).tobytes() == gnode.tobytes()
    assert all(m >= 0 for m in ctx.last_mesh_ms())
    assert hip.MESH_CUBES == mr.MESH_CUBES


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere16", "noncubic", "long200", "full8"])
def test_gpu_both_build_paths_and_frustum_state(ctx, cases, orc, name):
    """The level-by-level build leaves the same array, hence the same lists; rto_update_frustum in force changes nothing."""
    c = cases(name)
    view, _ = make_camera(orc, 0.5, 0.7, 0.9)
    try:
        for lbl in (True, False):
            ctx.debug_set_build_path(lbl)
            _resident(ctx, c)
            for culling in (False, True):
                if culling:
                    ctx.update_frustum(view, 45.0, 4.0 / 3.0, True)
                    ctx.debug_update_frustum_planes(c.planes[c.sets.index("rand%d" % int(_Z["seeds"][0]))], 0.0)
                for kind, kname in KINDS:
                    for si in range(len(c.sets)):
                        got, gnode = ctx.extract_mesh(kind, c.planes[si], c.margins[si])
                        want, wnode = c.ref(kind, si)
                        assert got.tobytes() == want.tobytes() and gnode.tobytes() == wnode.tobytes(), (name, lbl, culling, kname, c.sets[si])
            ctx.update_frustum(view, 45.0, 4.0 / 3.0, False)
    finally:
        ctx.debug_set_build_path(False)


@pytest.mark.gpu
def test_gpu_after_voxelize_and_edit(ctx, cases, orc):
    """Through rto_voxelize_mesh and after rto_edit_voxels: a mesh extracted before the edit still downloads unchanged, a new
    extraction matches the edited grid."""
    from ray_tracing_octrees_amd import hip
    # a closed box mesh voxelized into a fixed 24 x 20 x 18 grid
    lo, hi = np.array([0.13, 0.21, 0.17]), np.array([0.71, 0.62, 0.55])
    xyz = np.array([[(hi if (k >> a) & 1 else lo)[a] for a in range(3)] for k in range(8)], np.float64)
    faces = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                      [1, 5, 7], [1, 7, 3]], np.int32)
    gmin, vs = np.array([-0.05, 0.0, 0.02], np.float32), np.float32(1.0 / 32)
    ctx.voxelize_mesh(xyz, faces, vs, grid=((24, 20, 18), gmin, vs), triangles=True)

    def reference(planes, margin):
        data = ctx.download_voxels()
        g = orc.Grid((data.shape[2], data.shape[1], data.shape[0]), gmin, vs, data)
        nodes = orc.build_flat_octree(g)
        tris, off = orc.build_leaf_triangles(g, nodes)
        assert ctx.download_nodes().tobytes() == nodes.tobytes()
        return {kind: mr.extract(kind, nodes, gmin, vs, data=data, tris=tris, tri_offset=off, planes=planes, margin=margin) for kind, _ in KINDS}

    planes = hip.frustum_planes(make_camera(orc, 0.5, 0.7, 0.9)[0], 45.0, 4.0 / 3.0)
    for pl in (None, planes):
        want = reference(pl, 0.0)
        for kind, kname in KINDS:
            got, gnode = ctx.extract_mesh(kind, pl, 0.0)
            assert len(got) and got.tobytes() == want[kind][0].tobytes() and gnode.tobytes() == want[kind][1].tobytes(), kname
    before, before_node = ctx.extract_mesh(hip.MESH_CUBES, None, 0.0)
    changed = ctx.edit_voxels(hip.make_brushes([[0.4, 0.4, 0.55]], 0.2, hip.BRUSH_SPHERE, hip.EDIT_CARVE))
    assert changed > 0
    again, again_node = ctx.download_mesh()                        # the snapshot: untouched by the edit and its rebuild
    assert again.tobytes() == before.tobytes() and again_node.tobytes() == before_node.tobytes()
    want = reference(None, 0.0)
    for kind, kname in KINDS:
        got, gnode = ctx.extract_mesh(kind, None, 0.0)
        assert got.tobytes() == want[kind][0].tobytes() and gnode.tobytes() == want[kind][1].tobytes(), kname
    assert ctx.extract_mesh(hip.MESH_CUBES, None, 0.0)[0].tobytes() != before.tobytes()


@pytest.mark.gpu
def test_gpu_host_class_equals_the_c_abi(cases, orc):
    """RayTracerBVH::extractMesh (a camera) and extractMeshPlanes against Context.extract_mesh on the class's own context."""
    import ray_tracing_octrees_amd as rto
    from ray_tracing_octrees_amd import hip, host
    c = cases("sphere16")
    grid = host.VoxelGrid.from_array(c.data, c.min, c.vs)
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    rt.setOctreeFromGrid(grid)
    rt.buildLeafTriangles()
    cam = host.Camera(0.5, 0.7, 0.9)
    planes = hip.frustum_planes(cam.getView(), 45.0, 4.0 / 3.0)
    for kind, kname in KINDS:
        a = _rec12(rt.extractMesh(kind, cam, 4.0 / 3.0, 0.0))
        want = mr.extract(kind, c.nodes, c.min, c.vs, data=c.data, tris=c.tris, tri_offset=c.off, planes=planes, margin=0.0)[0]
        assert len(a) and a.tobytes() == want.tobytes(), (kname, rt.lastError)
        si = c.sets.index("rand%d" % int(_Z["seeds"][0]))
        b = _rec12(rt.extractMesh(kind, None, 1.0, c.margins[si], planes=c.planes[si]))
        assert b.tobytes() == c.ref(kind, si)[0].tobytes(), kname
        assert _rec12(rt.extractMesh(kind, None, 1.0, 50.0, planes=None)).tobytes() == c.ref(kind, 0)[0].tobytes(), kname


@pytest.mark.gpu
def test_gpu_errors_leave_the_previous_mesh(cases, orc):
    """Every refusal returns its code, in the stated order, and the mesh extracted before stays downloadable."""
    import ray_tracing_octrees_amd as rto
    from ray_tracing_octrees_amd import hip
    c = cases("noncubic")
    ctx = rto.Context(0)
    L = hip.load()
    n = C.c_int64(-7)
    try:
        with pytest.raises(hip.RtoError) as e:                       # nothing uploaded; INVALID comes first
            ctx.extract_mesh_count(hip.MESH_CUBES)
        assert e.value.code == hip.RTO_E_NO_OCTREE
        with pytest.raises(hip.RtoError) as e:
            ctx.extract_mesh_count(7)
        assert e.value.code == hip.RTO_E_INVALID
        with pytest.raises(hip.RtoError) as e:
            ctx.download_mesh()
        assert e.value.code == hip.RTO_E_INVALID
        _resident(ctx, c, triangles=False)
        keep, keep_node = ctx.extract_mesh(hip.MESH_CUBES, None, 0.0)
        assert keep.tobytes() == c.ref(mr.MESH_CUBES, 0)[0].tobytes()

        def still_there():
            t, nd = ctx.download_mesh()
            assert t.tobytes() == keep.tobytes() and nd.tobytes() == keep_node.tobytes()

        def refused(code, kind, planes=None, margin=0.0):
            with pytest.raises(hip.RtoError) as e:
                ctx.extract_mesh_count(kind, planes, margin)
            assert e.value.code == code, (e.value.code, code)
            still_there()

        refused(hip.RTO_E_INVALID, 2)
        refused(hip.RTO_E_INVALID, -1)
        assert L.rto_extract_mesh(ctx._h, hip.MESH_CUBES, None, None) == hip.RTO_E_INVALID
        still_there()
        bad = np.array(c.planes[1], np.float32)
        bad[5] = np.nan
        refused(hip.RTO_E_INVALID, hip.MESH_CUBES, bad, 0.0)
        bad[5] = np.inf
        refused(hip.RTO_E_INVALID, hip.MESH_CUBES, bad, 0.0)
        refused(hip.RTO_E_INVALID, hip.MESH_CUBES, c.planes[1], float("nan"))
        refused(hip.RTO_E_INVALID, hip.MESH_MC, bad, 0.0)            # INVALID before "no triangles"
        refused(hip.RTO_E_NO_OCTREE, hip.MESH_MC)                    # an octree, but no leaf triangles resident
        # an uploaded octree: no grid resident -> CUBES unsupported, MC served once triangles are uploaded
        ctx.upload_octree(c.nodes, c.min, c.vs)
        refused(hip.RTO_E_UNSUPPORTED, hip.MESH_CUBES)
        refused(hip.RTO_E_NO_OCTREE, hip.MESH_MC)
        ctx.upload_leaf_triangles(c.tris, c.off)
        got, gnode = ctx.extract_mesh(hip.MESH_MC, c.planes[5], c.margins[5])
        assert got.tobytes() == c.ref(mr.MESH_MC, 5)[0].tobytes() and gnode.tobytes() == c.ref(mr.MESH_MC, 5)[1].tobytes()
        keep, keep_node = got, gnode
        # a non-canonical array of more than one node: the same tree with two siblings' subtrees swapped in the array is refused
        odd = c.nodes.copy()
        odd["child"][0][[0, 1]] = odd["child"][0][[1, 0]]
        ctx.upload_octree(odd, c.min, c.vs)
        assert not ctx.info().canonical
        refused(hip.RTO_E_UNSUPPORTED, hip.MESH_MC)
        refused(hip.RTO_E_UNSUPPORTED, hip.MESH_CUBES)
        refused(hip.RTO_E_INVALID, 5)                                # INVALID still first
        assert L.rto_extract_mesh(ctx._h, hip.MESH_MC, None, C.byref(n)) == hip.RTO_E_UNSUPPORTED and n.value == -7
        # a one-node tree is served on both paths
        one = cases("full8")
        ctx.upload_octree(one.nodes, one.min, one.vs)
        ctx.upload_leaf_triangles(one.tris, one.off)
        assert ctx.extract_mesh_count(hip.MESH_MC) == 0
        refused_code = None
        try:
            ctx.extract_mesh_count(hip.MESH_CUBES)
        except hip.RtoError as err:
            refused_code = err.code
        assert refused_code == hip.RTO_E_UNSUPPORTED                 # uploaded: no grid
        ctx.build_octree(one.data, one.min, one.vs)
        t, nd = ctx.extract_mesh(hip.MESH_CUBES)
        assert len(t) == 12 and t.tobytes() == one.ref(mr.MESH_CUBES, 0)[0].tobytes() and (nd == 0).all()
        empty = cases("empty8")
        ctx.build_octree(empty.data, empty.min, empty.vs)
        assert ctx.extract_mesh_count(hip.MESH_CUBES) == 0 and ctx.download_mesh()[0].shape == (0, 12)
    finally:
        ctx.close()


def _subtree(nodes, i):
    """Indices of node i's descendants, following the child fields whatever the flags say."""
    out, stack = [], [int(c) for c in nodes["child"][i] if c >= 0]
    while stack:
        j = stack.pop()
        out.append(j)
        stack.extend(int(c) for c in nodes["child"][j] if c >= 0)
    return np.array(sorted(out), np.int64)


@pytest.mark.gpu
def test_gpu_unreachable_leaves_are_not_emitted(cases):
    """A canonical array may hold leaves that the tree does not reach: the subtree below a node marked isUniform without isLeaf
    (terminal for every traversal), and orphans after the last level.  With triangle ranges of their own they are counted by no
    ancestor and handed no offset; the mesh is the reachable tree's, with and without planes."""
    import ray_tracing_octrees_amd as rto
    from ray_tracing_octrees_amd import hip
    c = cases("sphere16")
    nodes = c.nodes
    cut = next(i for i in range(1, 9) if nodes["isLeaf"][i] == 0 and nodes["isUniform"][i] == 0
               and (np.diff(c.off)[_subtree(nodes, i)] > 0).any())
    lost = _subtree(nodes, cut)
    assert (nodes["isLeaf"][lost] == 1).any() and nodes["size"][lost].max() < nodes["size"][cut]
    odd = np.concatenate([nodes, np.repeat(nodes[-1:], 8)])           # 8 orphans of the last level's size, copies of the last leaf
    assert odd["isLeaf"][-1] == 1 and odd["size"][-1] == odd["size"].min()
    odd["isUniform"][cut] = 1
    orphans = np.arange(len(nodes), len(odd))
    extra = np.arange(8 * 3 * 12, dtype=np.float32).reshape(24, 12)   # three triangles for every orphan
    tris = np.concatenate([c.tris.reshape(-1, 12), extra])
    off = np.concatenate([c.off, c.off[-1] + 3 * np.arange(1, 9, dtype=np.int32)]).astype(np.int32)
    ctx = rto.Context(0)
    try:
        ctx.upload_octree(odd, c.min, c.vs)
        assert ctx.info().canonical
        ctx.upload_leaf_triangles(tris, off)
        for si in range(len(c.sets)):
            full, full_node = c.ref(mr.MESH_MC, si)
            keep = ~np.isin(full_node, lost)
            want, wnode = mr.extract(mr.MESH_MC, odd, c.min, c.vs, tris=tris, tri_offset=off, planes=c.planes[si], margin=c.margins[si])
            assert want.tobytes() == full[keep].tobytes() and wnode.tobytes() == full_node[keep].tobytes()
            if si == 0:
                assert 0 < len(want) < len(full)
            got, gnode = ctx.extract_mesh(hip.MESH_MC, c.planes[si], c.margins[si])
            assert got.tobytes() == want.tobytes() and gnode.tobytes() == wnode.tobytes(), c.sets[si]
            assert not np.isin(gnode, lost).any() and not np.isin(gnode, orphans).any()
            d_t, d_n, n = ctx.mesh_device()
            assert n == len(want)
    finally:
        ctx.close()


def _depth_first_array(nodes):
    """The same tree with every node's 8 children side by side, but each subtree stored before the next sibling's."""
    order, first = [0], {}

    def place(old, new):
        if nodes["isLeaf"][old] == 1 or nodes["isUniform"][old] == 1:
            return
        c0 = len(order)
        first[new] = c0
        order.extend(int(k) for k in nodes["child"][old])
        for k in range(8):
            place(int(nodes["child"][old][k]), c0 + k)
    place(0, 0)
    out = nodes[np.array(order)].copy()
    for new, c0 in first.items():
        out["child"][new] = c0 + np.arange(8)
    return out


@pytest.mark.gpu
def test_gpu_depth_first_array_is_refused(cases):
    """A valid tree stored depth first is canonical (every child block lies after its parent) but its levels are not contiguous
    ranges: RTO_E_UNSUPPORTED for both kinds' first reachable check, the previous mesh still downloadable."""
    import ray_tracing_octrees_amd as rto
    from ray_tracing_octrees_amd import hip
    c = cases("sphere16")
    dfs = _depth_first_array(c.nodes)
    assert len(dfs) == len(c.nodes) and (np.diff(dfs["size"].astype(np.int64)) > 0).any()      # the sizes grow somewhere
    ctx = rto.Context(0)
    try:
        ctx.upload_octree(c.nodes, c.min, c.vs)
        ctx.upload_leaf_triangles(c.tris, c.off)
        keep, keep_node = ctx.extract_mesh(hip.MESH_MC, None, 0.0)
        assert keep.tobytes() == c.ref(mr.MESH_MC, 0)[0].tobytes()
        ctx.upload_octree(dfs, c.min, c.vs)
        assert ctx.info().canonical
        ctx.upload_leaf_triangles(np.zeros((0, 12), np.float32), np.zeros(len(dfs) + 1, np.int32))
        for planes in (None, c.planes[1]):
            with pytest.raises(hip.RtoError) as e:
                ctx.extract_mesh_count(hip.MESH_MC, planes, 0.0)
            assert e.value.code == hip.RTO_E_UNSUPPORTED
            t, nd = ctx.download_mesh()
            assert t.tobytes() == keep.tobytes() and nd.tobytes() == keep_node.tobytes()
        ctx.upload_octree(c.nodes, c.min, c.vs)                       # the level table is per array: the BFS form is served again
        ctx.upload_leaf_triangles(c.tris, c.off)
        assert ctx.extract_mesh(hip.MESH_MC, None, 0.0)[0].tobytes() == keep.tobytes()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_host_class_without_an_octree_sets_its_error():
    """extractMesh before any octree: an empty list with lastError set by this call, never a message left by an earlier one."""
    import ray_tracing_octrees_amd as rto
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    assert len(rt.extractMesh(mr.MESH_MC, None, 1.0, 0.0, planes=None)) == 0
    assert "no octree" in rt.lastError
