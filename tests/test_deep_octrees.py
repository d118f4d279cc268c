"""Octrees of depth 11 to 20 -- the range the library accepts but no other scene reaches -- against the oracle and the
float64 reference of the box path (ref64.Octree64.trace_boxes).

At depth 19 and 20 a walk that descends through child 7 at every level holds 7 d + 1 = 134 / 141 stack entries: more
than the 128 of the reference's shader.  The spine scenes of deep_scenes.py are built so that their first camera's rays
do.  The thin scenes are dense grids of the same depths for the builders."""
from __future__ import annotations

import numpy as np
import pytest

import deep_scenes as ds
import ref64
from conftest import assert_bit_exact, partition_row_map

W, H = 48, 40
FOV = 45.0


def _frames(orc, s):
    out = []
    S = ref64.Octree64(s.nodes, s.min, s.voxel)
    for name, view, pos in s.cameras(orc):
        rd = orc.generate_rays(view, pos, W / H, FOV, W, H).reshape(-1, 3)
        first, closest = ref64.render_boxes64(S, pos, rd)
        out.append((name, view, pos, first, closest))
    return out


def check_boxes(ref, frame, what, d):
    """Robust pixels equal float64 (hit / miss, and the Lambert term within its float32 bound); the others are bounded."""
    v = frame.reshape(-1, 4)[:, 0].astype(np.float64)
    rob = ref["robust"]
    n = len(v)
    bound = 0.1 if d <= 12 else 0.95               # deeper, a voxel spans fewer float32 steps of the coordinates
    assert (~rob).sum() <= bound * n, f"{what}: {int((~rob).sum())} of {n} pixels non-robust"
    bad = rob & ((v > 0.05) != ref["hit"])
    assert not bad.any(), f"{what}: {int(bad.sum())} robust pixels with another hit / miss than float64, e.g. {np.nonzero(bad)[0][:5]}"
    m = rob & ref["hit"]
    err = np.abs(v - 0.1 - ref["shade"])
    bad = m & (err > ref["tol"] + 1e-6)
    assert not bad.any(), f"{what}: {int(bad.sum())} robust hit pixels off float64's n.l (max {err[bad].max():.3g})"


# ---------------------------------------------------------------- CPU
def test_numpy_builder_matches_the_oracle_builder(orc):
    rng = np.random.default_rng(7)
    for t in range(24):
        dims = tuple(int(v) for v in rng.integers(1, 19, 3))
        data = (rng.random(dims[::-1]) < rng.choice([0.05, 0.5, 0.95])).astype(np.uint8)
        if t % 4 == 0:
            data[:] = t % 8 == 0
        g = orc.Grid(dims, np.zeros(3, np.float32), np.float32(1), data)
        z, y, x = np.nonzero(data)
        assert ds.build_octree(np.stack([x, y, z], 1), dims).tobytes() == orc.build_flat_octree(g).tobytes(), f"{dims}"
    cube = ds.build_octree(np.zeros((0, 3)), (32, 32, 32), [(8, 0, 16, 8)])
    z, y, x = np.meshgrid(np.arange(16, 24), np.arange(8), np.arange(8, 16), indexing="ij")
    assert cube.tobytes() == ds.build_octree(np.stack([x.ravel(), y.ravel(), z.ravel()], 1), (32, 32, 32)).tobytes()


@pytest.mark.parametrize("d", ds.DEPTHS + (21,))
def test_host_builder_matches_numpy_builder_on_deep_grids(d):
    import ray_tracing_octrees_amd as rto

    s = ds.scene("far", d, "thin")
    root = rto.createOctreeFromVoxelGrid(rto.VoxelGrid.from_array(s.data, s.min, s.voxel))
    try:
        got = root.flatten()
    finally:
        rto.freeOctree(root)
    assert got.tobytes() == s.nodes.tobytes()
    assert s.nodes["size"][0] == 1 << d


@pytest.mark.parametrize("kind", ds.KINDS)
@pytest.mark.parametrize("d", ds.DEPTHS)
def test_oracle_equals_float64_on_deep_scenes(orc, d, kind):
    s = ds.scene(kind, d)
    for name, view, pos, first, closest in _frames(orc, s):
        img, st = orc.render(s.nodes, s.min, s.voxel, view, pos, W / H, FOV, W, H)
        cimg, cst = orc.render_closest(s.nodes, s.min, s.voxel, view, pos, W / H, FOV, W, H)
        assert st["overflow"] == 0 and cst["overflow"] == 0
        check_boxes(first, img, f"d {d} {kind} {name} first hit", d)
        check_boxes(closest, cimg, f"d {d} {kind} {name} closest hit", d)
        assert st["max_stack"] == first["need"].max(), f"d {d} {kind} {name}: oracle's stack {st['max_stack']} vs float64"
        if name == "near0":
            assert first["hit"].sum() > 0 and closest["hit"].sum() > 0


@pytest.mark.parametrize("d", ds.DEPTHS)
def test_stack_need_of_deep_scenes(orc, d):
    """The spine scene's first camera drives rays down the child-7 spine: 7 d + 1 entries, above 128 from depth 19 on;
    the oracle walks them with its 141 entries and reports the same maximum."""
    s = ds.scene("frac", d)
    assert ds.stack_need(s.nodes) == 7 * d + 1 <= ds.STACK_CAP
    name, view, pos = s.cameras(orc)[0]
    for render in (orc.render, orc.render_closest):
        _, st = render(s.nodes, s.min, s.voxel, view, pos, W / H, FOV, W, H)
        assert st["max_stack"] == 7 * d + 1 and st["overflow"] == 0
        assert (st["max_stack"] > 128) == (d >= 19)


def test_oracle_stops_a_walk_at_its_stack_capacity(orc):
    """A depth-21 spine needs 148 entries: the oracle counts the rays it cannot walk instead of writing past its stack."""
    N = 1 << 21
    corner = ds._ball((N - 2.0, N - 2.0, N - 2.0), 2.6)
    corner = corner[(corner < N).all(1) & ~(corner == N - 1).all(1)]
    nodes = ds.build_octree(corner, (N, N, N))
    assert ds.stack_need(nodes) == 7 * 21 + 1
    gmin, vs = np.full(3, -0.5, np.float32), np.float32(2.0 ** -21)
    cam = orc.Camera(0.7, 0.5, float(np.float32(9 * vs)))
    cam.set_target(*[float(v) for v in (gmin + (N - 1.5) * vs).astype(np.float32)])
    for render in (orc.render, orc.render_closest):
        _, st = render(nodes, gmin, vs, cam.get_view(), cam.get_pos(), W / H, FOV, W, H)
        assert st["overflow"] > 0 and st["max_stack"] <= ds.STACK_CAP


# ---------------------------------------------------------------- GPU
def _deep_params():
    return [pytest.param(d, marks=pytest.mark.gpu) for d in ds.DEPTHS]


@pytest.mark.parametrize("d", _deep_params())
def test_kernels_equal_oracle_and_float64_on_deep_scenes(ctx, orc, d):
    import ray_tracing_octrees_amd as rto
    from ray_tracing_octrees_amd import hip
    from test_gpu_parity import KERNELS

    torch = pytest.importorskip("torch")
    for kind in ds.KINDS:
        s = ds.scene(kind, d)
        ctx.set_kernel(rto.KERNEL_AUTO)
        ctx.upload_octree(s.nodes, s.min, s.voxel)
        assert ctx.info().canonical == 1 and ctx.info().depth == d
        for name, view, pos, first, closest in _frames(orc, s):
            what = f"d {d} {kind} {name}"
            f = rto.make_frame(view, pos, W / H, FOV, W, H)
            want, st = orc.render(s.nodes, s.min, s.voxel, view, pos, W / H, FOV, W, H)
            steps = orc.render_steps(s.nodes, s.min, s.voxel, view, pos, W / H, FOV, W, H)
            check_boxes(first, want, what, d)
            for kname, kernel in KERNELS:
                ctx.set_kernel(kernel)
                assert_bit_exact(ctx.render_host(f), want, f"{what} {kname}")
                np.testing.assert_array_equal(ctx.render_steps(f), steps, err_msg=f"{what} {kname}")
                gs = ctx.frame_stats(f)
                assert (gs["pops"], gs["hits"], gs["capped"]) == (st["pops"], st["hits"], st["capped"]), f"{what} {kname}"
            ctx.set_kernel(rto.KERNEL_AUTO)
            exact, _ = ctx.debug_set_exact_grid(True)
            assert bool(exact) == (kind != "tenth"), f"{what}: exact-grid proof"
            if exact:
                ctx.debug_set_exact_grid(False)
                try:
                    assert_bit_exact(ctx.render_host(f), want, f"{what}: general child test on an exact grid")
                    np.testing.assert_array_equal(ctx.render_steps(f), steps)
                finally:
                    ctx.debug_set_exact_grid(True)
            # batch kernel, 3-way partition
            arr = hip.Context.frame_array([f, f])
            out = torch.full((2, H, W, 4), 7.0, dtype=torch.float32, device="cuda")
            ctx.render_batch_device(arr, out.data_ptr(), out.stride(0) * 4, None, False, 0)
            torch.cuda.synchronize()
            for i in range(2):
                assert_bit_exact(out[i].cpu().numpy(), want, f"{what} batched frame {i}")
            part = hip.Partition(3, 1, 16)
            rows = ctx.partition_rows(f, part)
            pb = torch.full((rows, W, 4), 7.0, dtype=torch.float32, device="cuda")
            ctx.render_device(f, pb.data_ptr(), part)
            torch.cuda.synchronize()
            assert_bit_exact(pb.cpu().numpy(), want[partition_row_map(H, 3, 1, 16)], f"{what} part 1/3")
            # closest hit: the three kernels agree with the oracle and with float64's nearest-box rule
            cwant, cst = orc.render_closest(s.nodes, s.min, s.voxel, view, pos, W / H, FOV, W, H)
            check_boxes(closest, cwant, f"{what} closest", d)
            for kname, kernel in (("near first", rto.KERNEL_AUTO), ("pop order", rto.KERNEL_PACKED_V1), ("node by node", rto.KERNEL_GENERIC)):
                ctx.set_kernel(kernel)
                assert_bit_exact(ctx.render_closest_host(f), cwant, f"{what} closest hit, {kname}")
            ctx.set_kernel(rto.KERNEL_AUTO)
            # nearest-hit mode: its LDS frames (4 KB per level and workgroup) fit the 64 KB it allows up to depth 16
            if d <= 16:
                nrgba, nt = orc.render_skip(s.nodes, s.min, s.voxel, view, pos, W / H, FOV, W, H)
                grgba, gt_ = ctx.render_skip_host(f)
                assert gt_.tobytes() == nt.tobytes(), f"{what}: nearest-hit distances"
                assert_bit_exact(grgba, nrgba, f"{what} nearest-hit colours")
            else:
                with pytest.raises(rto.RtoError) as e:
                    ctx.render_skip_host(f)
                assert e.value.code == hip.RTO_E_UNSUPPORTED


@pytest.mark.parametrize("d", _deep_params())
def test_gpu_builds_and_triangles_on_deep_grids(ctx, orc, d):
    """rto_build_octree (both forms) and the GPU leaf-triangle build against the host arrays; the lean, packed and generic
    triangle kernels with shadows against the oracle."""
    import ray_tracing_octrees_amd as rto

    s = ds.scene("far", d, "thin")
    g = orc.Grid(s.dims, s.min, s.voxel, s.data)
    tris, off = orc.build_leaf_triangles(g, s.nodes)
    assert len(tris) > 0
    for level_by_level in (False, True):
        ctx.set_kernel(rto.KERNEL_AUTO)
        ctx.debug_set_build_path(level_by_level)
        ctx.build_octree(s.data, s.min, s.voxel)
        assert ctx.download_nodes().tobytes() == s.nodes.tobytes(), f"d {d} build (level by level: {level_by_level})"
        ctx.build_leaf_triangles(s.data)
        gt, go = ctx.download_leaf_triangles()
        assert go.tobytes() == np.asarray(off, np.int32).tobytes() and gt.tobytes() == np.ascontiguousarray(tris, np.float32).reshape(-1, 12).tobytes()
    ctx.debug_set_build_path(False)
    for name, view, pos in s.cameras(orc):
        f = rto.make_frame(view, pos, W / H, FOV, W, H)
        want, wst = orc.render_triangles(s.nodes, tris, off, s.min, s.voxel, view, pos, W / H, FOV, W, H, shadow=True)
        assert wst["overflow"] == 0
        for kname, kernel in (("lean", rto.KERNEL_AUTO), ("packed", rto.KERNEL_PACKED_V3), ("generic", rto.KERNEL_GENERIC)):
            ctx.set_kernel(kernel)
            got, gs = ctx.render_triangles_host(f, shadow=True, stats=True)
            assert_bit_exact(got, want, f"d {d} {name} triangles {kname}")
            assert (gs["pops"], gs["hits"]) == (wst["pops"], wst["hits"]), f"d {d} {name} triangles {kname}"
    ctx.set_kernel(rto.KERNEL_AUTO)


@pytest.mark.gpu
def test_upload_refuses_arrays_beyond_the_stack_contract(ctx, orc):
    import ray_tracing_octrees_amd as rto
    from ray_tracing_octrees_amd import hip

    gmin, vs = np.zeros(3, np.float32), np.float32(1.0)

    def refused(nodes, code):
        with pytest.raises(rto.RtoError) as e:
            ctx.upload_octree(nodes, gmin, vs)
        assert e.value.code == code

    # depth 21: the canonical thin grid, and the C++ class on the same grid
    s = ds.scene("far", 21, "thin")
    refused(s.nodes, hip.RTO_E_UNSUPPORTED)
    grid = rto.VoxelGrid.from_array(s.data, s.min, s.voxel)
    root = rto.createOctreeFromVoxelGrid(grid)
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    rt.setOctree(root, grid)
    cam = rto.Camera(0.5, 0.7, 1.8)
    rt.renderSceneComputeWithCulling(cam, 32, 24, 32 / 24, 45.0, True)
    assert rt.framebuffer() is None and "20 levels" in rt.lastError
    rto.freeOctree(root)
    # a non-canonical chain whose walk needs 7 * 21 + 1 entries although every node is 1 voxel
    n = 8 * 21 + 1
    chain = np.zeros(n, rto.NODE_DTYPE)
    chain["size"] = 1
    chain["isLeaf"] = chain["isUniform"] = 1
    chain["child"] = -1
    for lvl in range(21):
        p = 0 if lvl == 0 else 8 * lvl
        chain["isLeaf"][p] = chain["isUniform"][p] = 0
        chain["child"][p] = 8 * lvl + 1 + np.arange(8)
    assert ds.stack_need(chain) == 7 * 21 + 1
    refused(chain, hip.RTO_E_UNSUPPORTED)
    short = chain[: 8 * 20 + 1].copy()                           # one level less: 141 entries, accepted (generic kernel)
    short["isLeaf"][8 * 20] = short["isUniform"][8 * 20] = 1
    short["child"][8 * 20] = -1
    ctx.upload_octree(short, gmin, vs)
    assert ctx.info().canonical == 0
    bad = short.copy()
    bad["child"][0, 3] = len(bad)
    refused(bad, hip.RTO_E_INVALID)
    bad["child"][0, 3] = 0                                       # a cycle
    refused(bad, hip.RTO_E_UNSUPPORTED)
