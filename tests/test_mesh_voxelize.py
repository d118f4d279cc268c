"""Mesh voxelization (rto_voxelize_mesh, rto_last_voxelize_ms, Context.voxelize_mesh, RayTracerBVH::loadMesh,
loadCSVDataIntoVoxelGrid): the reference's loadCSVDataIntoVoxelGrid rule on the GPU, into the resident grid and the octree.
CPU: the numpy rule (tests/voxelize_ref.py) against the reference's own outputs (tests/golden/ref_voxelize.npz) and, where the
reference is present, against it freshly compiled on random meshes; the ABI; the kernels' budget.  GPU: grids, dims, gridMin and
voxelSize against every golden through the C ABI and the C++ CSV loader; the context against rto_build_octree of the same grid;
recentring; FIXED grids; leaf triangles; edits; a synthetic downtown; error paths."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import voxelize_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_voxelize.npz")
VOX_VGPR_BUDGET = 64        # 8 waves per SIMD; the kernels are store- and scan-bound
SYMS = ("rto_voxelize_mesh", "rto_last_voxelize_ms")


def _hip():
    from ray_tracing_octrees_amd import hip
    return hip


def _goldens():
    z = np.load(GOLDEN)
    out = {}
    for name in z["names"]:
        name = str(name)
        dims = tuple(int(d) for d in z[f"{name}_dims"])
        n = dims[0] * dims[1] * dims[2]
        out[name] = dict(
            verts_csv=z[f"{name}_verts_csv"].tobytes().decode(), faces_csv=z[f"{name}_faces_csv"].tobytes().decode(),
            voxel=np.float32(z[f"{name}_voxel"]), xyz=z[f"{name}_xyz"], tris=z[f"{name}_tris"], dims=dims,
            min=z[f"{name}_min"].astype(np.float32), vs=np.float32(z[f"{name}_vs"]),
            grid=np.unpackbits(z[f"{name}_packed"])[:n].reshape(dims[2], dims[1], dims[0]))
    return out


G = _goldens()
NAMES = sorted(G)


def _bits(a):
    return np.asarray(a, np.float32).tobytes()


# ================================================================ CPU
@pytest.mark.parametrize("name", NAMES)
def test_rule_equals_the_reference_golden(name):
    g = G[name]
    xyz, tris, nfaces = vr.parse_csv_mesh(g["verts_csv"], g["faces_csv"])
    assert np.array_equal(xyz, g["xyz"]) and np.array_equal(tris, g["tris"]) and nfaces >= len(tris)
    grid, dims, gmin, vs, _ = vr.voxelize(g["xyz"], g["tris"], g["voxel"])
    assert dims == g["dims"] and _bits(gmin) == _bits(g["min"]) and _bits(vs) == _bits(g["vs"]), name
    assert np.array_equal(grid, g["grid"]), name


def test_goldens_cover_the_quirks():
    """The fixture holds what the issue asks of it: the scale-1 branch, a rescaled voxel size, polar faces the 1e-7f cut rejects."""
    assert 1000 < G["dim1500"]["dims"][0] < 2000 and G["dim1500"]["vs"] == np.float32(1.0)
    assert G["dim2500"]["vs"] == np.float32(2.0)
    s = G["uv_sphere"]
    T = vr.face_terms(s["xyz"], s["tris"], s["min"], s["vs"], s["dims"])
    with np.errstate(all="ignore"):
        rejected = np.abs(T["d00"] * T["d11"] - T["d01"] * T["d01"]) < np.float32(1e-7)
    assert rejected.sum() > 0 and (~rejected).sum() > 0


def test_fresh_reference_equals_the_rule_on_random_meshes():
    """Where the reference exists: its loadCSVDataIntoVoxelGrid, compiled now, against voxelize_ref on random soups."""
    src = "/root/reference/453-skeleton/BuildingLoader.cpp"
    if not os.path.isfile(src):
        pytest.skip("the reference is not on this machine")
    import importlib.util
    spec = importlib.util.spec_from_file_location("mgv", os.path.join(ROOT, "tests", "golden", "make_golden_voxelize.py"))
    mgv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mgv)
    rng = np.random.default_rng(2024)
    with tempfile.TemporaryDirectory() as tmp:
        exe = mgv.build(tmp)
        for k in range(4):
            base = np.array([7.0e5, 5.66e6, 1.0e3]) if k % 2 else np.zeros(3)
            pts = base + rng.uniform(0, [40, 30, 20], size=(60, 3)).round(4)
            rows = [(1, i, *map(float, p)) for i, p in enumerate(pts)]
            faces = [(1, *map(int, rng.integers(0, 60, 3))) for _ in range(80)]
            vox = float(rng.choice([0.7, 1.3, 2.5]))
            vcsv, fcsv = mgv.to_csv(rows, faces)
            dims, gmin, vs, data = mgv.run_ref(exe, tmp, vcsv, fcsv, vox)
            grid, d, m, v, _ = vr.voxelize(pts, [f[1:] for f in faces], vox)
            assert tuple(dims) == d and _bits(gmin) == _bits(m) and _bits(vs) == _bits(v), k
            assert np.array_equal(grid.reshape(-1), data), k
        # the AUTO families of tests/voxelize_families.py: the rescale's edges with NaN rows and degenerate faces, and a mesh
        # whose every face is degenerate (FIXED grids have no counterpart in the reference)
        import voxelize_families as vf
        autos = {f"auto_{d}": vf.auto_edges(d) for d in vf.AUTO_EDGE_DIMS}
        autos["all_degenerate_auto"] = vf.empty_all_degenerate(auto=True)
        for name, c in autos.items():
            rows = [(1, i, *map(float, p)) for i, p in enumerate(c.xyz)]
            vcsv, fcsv = mgv.to_csv(rows, [(1, *map(int, t)) for t in c.tris])
            dims, gmin, vs, data = mgv.run_ref(exe, tmp, vcsv, fcsv, c.voxel)
            grid, d, m, v, _ = vr.voxelize(c.xyz, c.tris, c.voxel)
            assert tuple(dims) == d and _bits(gmin) == _bits(m) and _bits(vs) == _bits(v), name
            assert np.array_equal(grid.reshape(-1), data), name


def test_voxelize_abi_layout_and_exports():
    hip = _hip()
    assert C.sizeof(hip.VoxelizeParams) == 40 and C.sizeof(hip.VoxelizeResult) == 48
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.fail("no C compiler: the header's layout cannot be checked")
    fields_p = ("mode", "voxel_size", "dims", "grid_min", "recenter_passes", "triangles")
    fields_r = ("dims", "grid_min", "voxel_size", "reserved", "filled", "pairs")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "abi.c")
        body = " ".join(f'printf("%zu ", offsetof(rto_voxelize_params, {f}));' for f in fields_p)
        body += " ".join(f'printf("%zu ", offsetof(rto_voxelize_result, {f}));' for f in fields_r)
        with open(src, "w") as f:
            f.write('#include <stddef.h>\n#include <stdio.h>\n#include "rto_hip.h"\nint main(void) { printf("%zu %zu %d %d ", '
                    'sizeof(rto_voxelize_params), sizeof(rto_voxelize_result), RTO_VOXELIZE_AUTO, RTO_VOXELIZE_FIXED); '
                    + body + ' return 0; }\n')
        exe = os.path.join(tmp, "abi")
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:4] == [40, 48, hip.VOXELIZE_AUTO, hip.VOXELIZE_FIXED]
    assert out[4:10] == [getattr(hip.VoxelizeParams, f).offset for f in fields_p]
    assert out[10:] == [getattr(hip.VoxelizeResult, f).offset for f in fields_r]
    L = hip.load()
    header = open(os.path.join(ROOT, "include", "rto_hip.h")).read()
    for s in SYMS:
        assert s in hip.SYMBOLS and hasattr(L, s) and s + "(" in header, s


def test_voxelize_kernels_keep_their_budgets():
    """The built assembly (the product's flags): every k_vox_* kernel and the voxelizer's k_scan_counts without scratch, spills or v_mfma, within the VGPR budget."""
    import test_isa_contract as isa
    asm = isa.built_asm()
    if asm is None:
        pytest.fail("no hipcc: the budget cannot be checked")
    meta = isa.kernel_meta(asm)
    names = [k for k in meta if "k_vox_" in k or "k_scan_countsILi1024Exx" in k]      # the scan of the block sums: the shared kernel's 64-bit form
    assert len(names) == 5, names
    for k in names:
        m = meta[k]
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (k, m)
        assert m["vgpr"] <= VOX_VGPR_BUDGET, (k, m)
        ins = isa.body(asm, k[len("_ZN3rto"):])
        assert not any(t.startswith(("scratch_", "buffer_load", "buffer_store")) or "v_mfma" in t for t in ins), k
        if "k_vox_fill" in k:
            assert any(t.startswith("global_store_byte") for t in ins), k


# ================================================================ GPU
gpu = pytest.mark.gpu
W, H, FOV = 128, 96, 45.0


@pytest.fixture(scope="module")
def ctx2():
    c = _hip().Context(0)
    yield c
    c.close()


def _check_result(r, dims, gmin, vs, grid):
    assert tuple(r.dims) == tuple(dims)
    assert _bits(list(r.grid_min)) == _bits(gmin) and _bits(r.voxel_size) == _bits(vs)
    assert r.filled == int(np.count_nonzero(grid))


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_voxelize_equals_every_golden(ctx, name, tmp_path):
    """Through the C ABI and through the C++ loadCSVDataIntoVoxelGrid on the fixture's CSV text."""
    import ray_tracing_octrees_amd as rto
    g = G[name]
    r = ctx.voxelize_mesh(g["xyz"], g["tris"], g["voxel"])
    _check_result(r, g["dims"], g["min"], g["vs"], g["grid"])
    assert np.array_equal(ctx.download_voxels(), g["grid"]), name
    ms = ctx.last_voxelize_ms()
    assert all(m >= 0 for m in ms), ms
    (tmp_path / "v.csv").write_text(g["verts_csv"])
    (tmp_path / "f.csv").write_text(g["faces_csv"])
    vg = rto.loadCSVDataIntoVoxelGrid(str(tmp_path / "v.csv"), str(tmp_path / "f.csv"), g["voxel"])
    assert vg.dims == g["dims"] and _bits(vg.min) == _bits(g["min"]) and _bits(vg.voxelSize) == _bits(g["vs"]), name
    assert np.array_equal(vg.data, g["grid"]), name


@gpu
def test_gpu_csv_loader_empty_inputs(tmp_path):
    """No vertex row or no face row: the reference's empty grid.  Face rows that all name missing vertices: the full AUTO grid, all
    EMPTY."""
    import ray_tracing_octrees_amd as rto
    g = G["soup"]
    (tmp_path / "v.csv").write_text(g["verts_csv"])
    (tmp_path / "f0.csv").write_text("MeshNumber,V1,V2,V3\n")
    (tmp_path / "f1.csv").write_text("MeshNumber,V1,V2,V3\n77,1,2,3\n3,900,901,902\n")
    (tmp_path / "v0.csv").write_text("header\n")
    assert rto.loadCSVDataIntoVoxelGrid(str(tmp_path / "v.csv"), str(tmp_path / "f0.csv"), 1.0).dims == (0, 0, 0)
    assert rto.loadCSVDataIntoVoxelGrid(str(tmp_path / "v0.csv"), str(tmp_path / "f1.csv"), 1.0).dims == (0, 0, 0)
    vg = rto.loadCSVDataIntoVoxelGrid(str(tmp_path / "v.csv"), str(tmp_path / "f1.csv"), 1.0)
    assert vg.dims == g["dims"] and _bits(vg.min) == _bits(g["min"]) and not vg.data.any()


def _look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """glm::lookAt (right-handed) as the column-major float[16] the frames take, and the eye."""
    eye, target, up = (np.asarray(x, np.float64) for x in (eye, target, up))
    f = (target - eye) / np.linalg.norm(target - eye)
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    m = np.eye(4)
    m[0, :3], m[1, :3], m[2, :3] = s, u, -f                    # rows of the view matrix
    m[:3, 3] = [-s @ eye, -u @ eye, f @ eye]
    return m.T.astype(np.float32).reshape(16), eye.astype(np.float32)


def _same_context(ctx, ctx2, grid, gmin, vs, what):
    """ctx (voxelized) equals ctx2 after rto_build_octree(grid): nodes, info, scene bounds, and a rendered frame bit for bit."""
    from ray_tracing_octrees_amd import hip
    ctx2.build_octree(grid, gmin, vs)
    assert ctx.download_nodes().tobytes() == ctx2.download_nodes().tobytes(), what
    assert bytes(ctx.info()) == bytes(ctx2.info()), what
    assert bytes(ctx.scene_bounds()) == bytes(ctx2.scene_bounds()), what
    dims = np.asarray(grid.shape[::-1], np.float32)
    ext = float(vs) * float(dims.max())
    centre = np.asarray(gmin, np.float64) + 0.5 * float(vs) * dims
    view, pos = _look_at(centre + ext * np.array([1.1, 0.9, 1.3]), centre)
    f = hip.make_frame(view, pos, W / H, FOV, W, H)
    a, b = ctx.render_host(f), ctx2.render_host(f)
    assert a.tobytes() == b.tobytes(), what
    return a


@gpu
@pytest.mark.parametrize("name", ["utm_blocks_1p3", "uv_sphere", "ground"])
def test_gpu_voxelize_equals_build_octree(ctx, ctx2, name):
    from ray_tracing_octrees_amd import hip
    g = G[name]
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx2.set_kernel(hip.KERNEL_AUTO)
    ctx.voxelize_mesh(g["xyz"], g["tris"], g["voxel"])
    img = _same_context(ctx, ctx2, g["grid"], g["min"], g["vs"], name)
    assert (img[..., :3] != 0).any(), name


@gpu
@pytest.mark.parametrize("passes", [1, 2])
def test_gpu_recentring_equals_voxelgrid_recenter(ctx, ctx2, passes):
    import ray_tracing_octrees_amd as rto
    for name in ("utm_blocks_3p7", "soup", "dim2500"):
        g = G[name]
        r = ctx.voxelize_mesh(g["xyz"], g["tris"], g["voxel"], recenter=passes)
        vg = rto.VoxelGrid.from_array(g["grid"], g["min"], g["vs"])
        for _ in range(passes):
            assert vg.recenter()
        assert _bits(list(r.grid_min)) == _bits(vg.min), (name, passes)
        assert _bits(vr.recenter(g["grid"], g["min"], g["vs"], passes)) == _bits(vg.min), (name, passes)
        _same_context(ctx, ctx2, g["grid"], vg.min, g["vs"], f"{name} recentred {passes}x")


@gpu
def test_gpu_fixed_power_of_two_grid(ctx, ctx2):
    """FIXED 256^3 on power-of-two voxels (the exact-grid proof holds): the numpy rule's grid, and rto_build_octree's context."""
    xyz, tris = vr.uv_sphere(64, 128, 0.45)
    vs = np.float32(1.0 / 256)
    gmin = np.full(3, -0.5, np.float32)
    want, _ = vr.fill(xyz, tris, gmin, vs, (256, 256, 256))
    r = ctx.voxelize_mesh(xyz, tris, vs, grid=((256, 256, 256), gmin, vs))
    _check_result(r, (256, 256, 256), gmin, vs, want)
    assert np.array_equal(ctx.download_voxels(), want)
    _same_context(ctx, ctx2, want, gmin, vs, "fixed 256^3")


@gpu
def test_gpu_leaf_triangles_after_voxelize(ctx, ctx2):
    g = G["utm_blocks_3p7"]
    ctx.voxelize_mesh(g["xyz"], g["tris"], g["voxel"], recenter=2, triangles=True)
    gmin = vr.recenter(g["grid"], g["min"], g["vs"], 2)
    ctx2.build_octree(g["grid"], gmin, g["vs"])
    ctx2.build_leaf_triangles(None)
    a, b = ctx.download_leaf_triangles(), ctx2.download_leaf_triangles()
    assert len(a[0]) > 0
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@gpu
def test_gpu_edit_after_voxelize(ctx, ctx2):
    import edit_ref as er
    from ray_tracing_octrees_amd import hip
    g = G["utm_blocks_1p3"]
    ctx.voxelize_mesh(g["xyz"], g["tris"], g["voxel"])
    centre = (g["min"] + np.float32(g["vs"]) * np.asarray(g["dims"], np.float32) * np.float32(0.5)).astype(np.float32)
    b = hip.make_brushes([centre], 8 * float(g["vs"]), er.SPHERE, er.CARVE)
    edited, changed = er.apply(g["grid"], b, g["min"], g["vs"])
    assert changed > 0 and ctx.edit_voxels(b) == changed
    assert np.array_equal(ctx.download_voxels(), edited)
    _same_context(ctx, ctx2, edited, g["min"], g["vs"], "edited after voxelize")


@gpu
@pytest.mark.parametrize("voxel", [10.0, 5.0, 2.5])
def test_gpu_downtown(ctx, voxel):
    """About 50 k triangles of a synthetic city plus one ground quad, against the numpy rule."""
    xyz, tris = vr.downtown()
    grid, dims, gmin, vs, pairs = vr.voxelize(xyz, tris, voxel)
    r = ctx.voxelize_mesh(xyz, tris, voxel)
    _check_result(r, dims, gmin, vs, grid)
    assert r.pairs == pairs
    assert np.array_equal(ctx.download_voxels(), grid), voxel


@gpu
def test_gpu_voxelize_errors_leave_the_context_untouched(ctx):
    from ray_tracing_octrees_amd import hip
    g = G["utm_blocks_10"]
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.voxelize_mesh(g["xyz"], g["tris"], g["voxel"])
    nodes, vox, info = ctx.download_nodes(), ctx.download_voxels(), bytes(ctx.info())
    f = hip.make_frame(np.eye(4, dtype=np.float32), [0, 0, 0], W / H, FOV, W, H)
    img = ctx.render_host(f)
    xyz, tris = g["xyz"], g["tris"]
    far = xyz.copy()
    far[0] = [1e14, 0.0, 0.0]
    bad = [
        lambda: ctx.voxelize_mesh(xyz, np.where(tris == 3, len(xyz), tris), 1.0),            # row index out of range
        lambda: ctx.voxelize_mesh(xyz, np.where(tris == 3, -1, tris), 1.0),
        lambda: ctx.voxelize_mesh(xyz, tris, 0.0),
        lambda: ctx.voxelize_mesh(xyz, tris, np.nan),
        lambda: ctx.voxelize_mesh(xyz, tris, 1.0, recenter=3),
        lambda: ctx.voxelize_mesh(xyz, tris, 1.0, grid=((0, 4, 4), (0, 0, 0), 1.0)),
        lambda: ctx.voxelize_mesh(xyz, tris, 1.0, grid=((4, 4, 4), (np.inf, 0, 0), 1.0)),
        lambda: ctx.voxelize_mesh(xyz, tris, 1.0, grid=((4, 4, 4), (0, 0, 0), -1.0)),
        lambda: ctx.voxelize_mesh(xyz, tris, 1.0, grid=((1 << 21, 4, 4), (0, 0, 0), 1.0)),         # above the size limit
        lambda: ctx.voxelize_mesh(xyz, tris, 1.0, grid=((64, 64, 64), xyz.min(0) - 1e12, 1.0)),   # int casts overflow
        lambda: ctx.voxelize_mesh(far, tris, 1e-6),                                                # AUTO grid too large
        lambda: ctx.voxelize_mesh(xyz, np.zeros((0, 3), np.int32), 1.0),                           # AUTO with no face: empty
        lambda: ctx.voxelize_mesh(np.full((3, 3), np.nan), [[0, 1, 2]], 1.0),                      # no finite row: empty
    ]
    for i, call in enumerate(bad):
        try:
            call()
            raise AssertionError(f"case {i} was accepted")
        except hip.RtoError as e:
            assert e.code == hip.RTO_E_INVALID, (i, e)
    L = hip.load()
    p = hip.VoxelizeParams()
    p.voxel_size = 1.0
    assert L.rto_voxelize_mesh(ctx._h, None, 3, None, 0, C.byref(p), None) == hip.RTO_E_INVALID
    assert L.rto_voxelize_mesh(ctx._h, None, -1, None, 0, C.byref(p), None) == hip.RTO_E_INVALID
    assert L.rto_voxelize_mesh(ctx._h, None, 0, None, 0, None, None) == hip.RTO_E_INVALID
    p.mode = 7
    assert L.rto_voxelize_mesh(ctx._h, xyz.ctypes.data, len(xyz), tris.ctypes.data, len(tris), C.byref(p), None) == hip.RTO_E_INVALID
    assert ctx.download_nodes().tobytes() == nodes.tobytes()
    assert np.array_equal(ctx.download_voxels(), vox) and bytes(ctx.info()) == info
    assert ctx.render_host(f).tobytes() == img.tobytes()
