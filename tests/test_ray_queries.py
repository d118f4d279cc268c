"""Ray queries (rto_query_*, Context.query_*, RayTracerBVH::intersectRays / pick): caller-supplied rays and pixel picks on the
octree.  CPU: the float32 statement of the acceptance rule (tests/query_ref.py) against the oracle's renders and float64; the
ABI's layout; the built assembly of the k_query_* kernels.  GPU: every mode against those statements, bit for bit."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import deep_scenes as ds
import query_ref as q
import ref64
from conftest import SPHERE_CAM, make_camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOV = 45.0
MODES = (q.FIRST, q.CLOSEST, q.ANY)
VGPR_BUDGET = 72            # 7 waves per SIMD (512 / 7 = 73, allocated by 8)


def _hits_equal(got, want, what, mask_only=False):
    """Records equal field by field (t bitwise); mask_only: the hit / miss mask alone (ANY's leaf is unspecified)."""
    gh, wh = got["node"] >= 0, want["node"] >= 0
    bad = np.nonzero(gh != wh)[0]
    assert not len(bad), f"{what}: {len(bad)} rays differ in hit / miss, e.g. {bad[:5]}: got {got[bad[:3]]} want {want[bad[:3]]}"
    if mask_only:
        return
    neq = (got.view(np.int32).reshape(-1, 8) != want.view(np.int32).reshape(-1, 8)).any(1)
    bad = np.nonzero(neq)[0]
    assert not len(bad), f"{what}: {len(bad)} records differ, e.g. rays {bad[:5]}: got {got[bad[:3]]} want {want[bad[:3]]}"


def _pixel_rays(orc, view, pos, W, H):
    return orc.generate_rays(view, pos, W / H, FOV, W, H).reshape(-1, 3)


# ================================================================ CPU
@pytest.mark.parametrize("scene,cam", [("sphere64", SPHERE_CAM), ("sphere64", (0.3, 0.2, 0.1)), ("calgary", "calgary_oblique")])
def test_float32_statement_gives_the_oracle_frames(orc, scenes, camera, scene, cam):
    """query_ref.query32 on generate_rays with (0, 1e30): FIRST's hit mask is orc.render's and CLOSEST's orc.render_closest's, and
    shading the returned (leaf, t) with the oracle's shade_store formula gives their pixels bit for bit."""
    s = scenes(scene)
    view, pos = camera(cam) if isinstance(cam, str) else make_camera(orc, *cam)
    W, H = 80, 60
    T = q.Tree32(s.nodes, s.min, s.voxel)
    rd = _pixel_rays(orc, view, pos, W, H)
    r = q.query32(T, pos, rd)
    first, _ = orc.render(s.nodes, s.min, s.voxel, view, pos, W / H, FOV, W, H)
    closest, _ = orc.render_closest(s.nodes, s.min, s.voxel, view, pos, W / H, FOV, W, H)
    for mode, img in ((q.FIRST, first), (q.CLOSEST, closest)):
        want = img.reshape(-1, 4)
        assert ((r[mode]["node"] >= 0) == (want[:, 0] > 0.05)).all()
        got = q.shade32(T, pos, rd, r[mode])
        assert got.tobytes() == want.tobytes(), f"mode {mode}: {int((got != want).any(1).sum())} pixels"
    assert ((r[q.FIRST]["node"] >= 0).sum() > 0)


def test_float32_statement_against_float64_on_robust_pixel_rays(orc, scenes):
    """query32 with (0, 1e30) against Octree64.trace_boxes: robust rays agree in hit and leaf for FIRST and CLOSEST."""
    s = scenes("sphere64")
    S = ref64.Octree64(s.nodes, s.min, s.voxel)
    T = q.Tree32(s.nodes, s.min, s.voxel)
    for cam in (SPHERE_CAM, (0.3, 0.2, 0.1), (1.2, 2.0, 0.9)):
        view, pos = make_camera(orc, *cam)
        rd = _pixel_rays(orc, view, pos, 64, 48)
        first, closest = ref64.render_boxes64(S, pos, rd)
        r = q.query32(T, pos, rd)
        for mode, ref in ((q.FIRST, first), (q.CLOSEST, closest)):
            rob = ref["robust"]
            assert rob.mean() > 0.95
            assert ((r[mode]["node"] >= 0) == ref["hit"])[rob].all()
            assert (r[mode]["node"] == ref["leaf"])[rob].all()


@pytest.mark.parametrize("scene,seed", [("sphere64", 1), ("odd", 2), ("calgary", 3)])
def test_float32_statement_against_float64_with_windows(scenes, scene, seed):
    """Seeded rays of every kind with [t_min, t_max] windows: query32 against Octree64Q (Octree64 extended by a windowed rule).
    Robust rays agree in hit (all modes) and leaf (FIRST, CLOSEST); the non-robust share stays small; t agrees within float32."""
    s = scenes(scene)
    T = q.Tree32(s.nodes, s.min, s.voxel)
    o, d, tmn, tmx = q.seeded_rays(T, 2048, seed)
    r = q.query32(T, o, d, tmn, tmx)
    w = q.Octree64Q(s.nodes, s.min, s.voxel).trace_windows(o.astype(np.float64), d.astype(np.float64), tmn, tmx)
    for mode in MODES:
        rob = w[mode]["robust"]
        assert rob.mean() > 0.75, (mode, rob.mean())
        assert ((r[mode]["node"] >= 0) == w[mode]["hit"])[rob].all(), mode
        if mode != q.ANY:
            assert (r[mode]["node"] == w[mode]["leaf"])[rob].all(), mode
    c = w[q.CLOSEST]
    h = c["robust"] & c["hit"]
    assert np.allclose(r[q.CLOSEST]["t"][h], c["t"][h], rtol=1e-4, atol=1e-5 * float(np.abs(s.min).max() + 1))
    # windows do what they say
    assert (r[q.CLOSEST]["node"] >= 0).any() and (r[q.CLOSEST]["node"] < 0).any()
    hit = r[q.CLOSEST]["node"] >= 0
    assert (r[q.CLOSEST]["t"][hit] <= tmx[hit]).all() and (r[q.CLOSEST]["t"][hit] >= np.maximum(tmn[hit], 0)).all()
    assert (r[q.CLOSEST]["node"][-7:-1] == -1).all()                 # NaN rays and t_min > t_max


def test_query_structs_are_32_bytes():
    from ray_tracing_octrees_amd import hip
    assert C.sizeof(hip.Ray) == 32 and C.sizeof(hip.Hit) == 32
    assert hip.RAY_DTYPE.itemsize == 32 and hip.HIT_DTYPE.itemsize == 32
    assert hip.HIT_DTYPE == q.HIT_DTYPE
    assert (hip.QUERY_FIRST, hip.QUERY_CLOSEST, hip.QUERY_ANY) == (0, 1, 2)
    hdr = open(os.path.join(ROOT, "include", "rto_hip.h")).read()
    for name, v in (("RTO_QUERY_FIRST", 0), ("RTO_QUERY_CLOSEST", 1), ("RTO_QUERY_ANY", 2)):
        assert re.search(rf"#define {name}\s+{v}\b", hdr)
    for sym in ("rto_query_rays_device", "rto_query_rays_host", "rto_query_pixels_device", "rto_query_pixels_host"):
        assert sym in hip.SYMBOLS


def test_query_kernels_keep_their_budgets():
    """The built assembly (the product's flags): every k_query_* kernel without scratch instructions, VGPR spills or v_mfma, and
    within the VGPR budget DESIGN.md section 10 states."""
    import test_isa_contract as isa
    asm = isa.built_asm()
    if asm is None:
        pytest.skip("no hipcc in this environment")
    meta = isa.kernel_meta(asm)
    names = [k for k in meta if "k_query_" in k]
    assert len(names) == 12, names                                    # {desc, nodes} x {FIRST, CLOSEST, ANY} x {rays, pixels}
    for k in names:
        m = meta[k]
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (k, m)
        assert m["vgpr"] <= VGPR_BUDGET, (k, m)
        ins = isa.body(asm, k[len("_ZN3rto"):])
        assert not any(t.startswith(("scratch_", "buffer_load", "buffer_store")) or "v_mfma" in t for t in ins), k


# ================================================================ GPU
gpu = pytest.mark.gpu


def _rto():
    import ray_tracing_octrees_amd as rto
    return rto


def _all_pixels(W, H):
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([x.ravel(), y.ravel()], 1).astype(np.int32)


def _upload(ctx, s, kernel=None):
    rto = _rto()
    ctx.set_kernel(rto.KERNEL_AUTO if kernel is None else kernel)
    ctx.upload_octree(s.nodes, s.min, s.voxel)


@gpu
@pytest.mark.parametrize("scene,cam,W,H", [("sphere64", SPHERE_CAM, 160, 120), ("sphere64", (0.3, 0.2, 0.1), 128, 96),
                                           ("sphere256", SPHERE_CAM, 320, 240), ("sphere256", (0.3, 0.2, 0.1), 256, 160),
                                           ("calgary", "calgary_default", 260, 260), ("calgary", "calgary_oblique", 320, 180)])
def test_pixel_queries_reproduce_the_renders(ctx, orc, scenes, camera, scene, cam, W, H):
    """Every pixel of a frame: FIRST gives rto_render_host's hits, CLOSEST rto_render_closest_host's, ANY CLOSEST's mask; shading
    (leaf, t) in numpy gives both frames bit for bit; query_rays on orc.generate_rays gives query_pixels' records bit for bit."""
    rto = _rto()
    s = scenes(scene)
    _upload(ctx, s)
    view, pos = camera(cam) if isinstance(cam, str) else make_camera(orc, *cam)
    f = rto.make_frame(view, pos, W / H, FOV, W, H)
    T = q.Tree32(s.nodes, s.min, s.voxel)
    rd = _pixel_rays(orc, view, pos, W, H)
    xy = _all_pixels(W, H)
    got = {m: ctx.query_pixels(f, xy, m) for m in MODES}
    frames = {q.FIRST: ctx.render_host(f), q.CLOSEST: ctx.render_closest_host(f)}
    for m, img in frames.items():
        want = img.reshape(-1, 4)
        assert ((got[m]["node"] >= 0) == (want[:, 0] > 0.05)).all(), f"mode {m}: hit mask"
        sh = q.shade32(T, pos, rd, got[m])
        assert sh.tobytes() == want.tobytes(), f"mode {m}: {int((sh != want).any(1).sum())} pixels shade differently"
    _hits_equal(got[q.ANY], got[q.CLOSEST], "ANY vs CLOSEST", mask_only=True)
    for m in MODES:
        byrays = ctx.query_rays(np.broadcast_to(pos, rd.shape), rd, 0.0, 1e30, m)
        _hits_equal(byrays, got[m], f"mode {m}: query_rays vs query_pixels", mask_only=(m == q.ANY))
    if scene == "sphere64":
        want = q.query32(T, pos, rd)
        for m in MODES:
            _hits_equal(got[m], want[m], f"mode {m}: vs query32", mask_only=(m == q.ANY))


@gpu
@pytest.mark.parametrize("scene,seed", [("sphere64", 11), ("odd", 12), ("calgary", 13), ("sphere256", 14)])
def test_seeded_rays_match_the_float32_statement(ctx, scenes, scene, seed):
    """Arbitrary rays of every kind (outside / inside / inside solid leaves, axis-aligned, zero components, grazing, t_max and t_min
    windows, NaN and t_min > t_max) in every mode: bit for bit the records of query32, on the descriptor kernel and the node-by-node
    kernel; against float64 on its robust rays."""
    rto = _rto()
    s = scenes(scene)
    T = q.Tree32(s.nodes, s.min, s.voxel)
    o, d, tmn, tmx = q.seeded_rays(T, 4096, seed)
    want = q.query32(T, o, d, tmn, tmx)
    w64 = q.Octree64Q(s.nodes, s.min, s.voxel).trace_windows(o.astype(np.float64), d.astype(np.float64), tmn, tmx)
    for kernel in (rto.KERNEL_AUTO, rto.KERNEL_GENERIC):
        _upload(ctx, s, kernel)
        for m in MODES:
            got = ctx.query_rays(o, d, tmn, tmx, m)
            _hits_equal(got, want[m], f"kernel {kernel} mode {m}", mask_only=(m == q.ANY))
            rob = w64[m]["robust"]
            assert ((got["node"] >= 0) == w64[m]["hit"])[rob].all()
            assert rob.mean() > 0.75
            if m == q.ANY:
                # ANY's leaf: some accepted one -- it is a solid leaf that the ray's CLOSEST record does not beat by the rule
                h = got["node"] >= 0
                assert (s.nodes["isSolid"][got["node"][h]] == 1).all()
                assert (got["t"][h] <= tmx[h]).all()
    ctx.set_kernel(rto.KERNEL_AUTO)


@gpu
@pytest.mark.parametrize("kind,d", [("frac", 11), ("far", 16), ("tenth", 19), ("frac", 20)])
def test_deep_octrees_every_mode_against_float64(ctx, orc, kind, d):
    """Depth 11-20 trees (tests/deep_scenes.py): pixel rays of the scene's cameras and seeded rays, every mode, both kernels:
    robust rays agree with float64, and the two kernels agree with each other bit for bit."""
    rto = _rto()
    s = ds.scene(kind, d)
    Q = q.Octree64Q(s.nodes, s.min, s.voxel)
    T = q.Tree32(s.nodes, s.min, s.voxel)
    W, H = 48, 40
    rays = []
    for _, view, pos in s.cameras(orc):
        rd = _pixel_rays(orc, view, pos, W, H)
        rays.append((np.broadcast_to(pos, rd.shape).astype(np.float32), rd, np.zeros(len(rd), np.float32), np.full(len(rd), 1e30, np.float32)))
    rays.append(q.seeded_rays(T, 1024, d))
    o, dd, tmn, tmx = (np.concatenate(x) for x in zip(*rays))
    w = Q.trace_windows(o.astype(np.float64), dd.astype(np.float64), tmn, tmx)
    res = {}
    for kernel in (rto.KERNEL_AUTO, rto.KERNEL_GENERIC):
        _upload(ctx, s, kernel)
        for m in MODES:
            res[kernel, m] = got = ctx.query_rays(o, dd, tmn, tmx, m)
            rob = w[m]["robust"]
            assert (~rob).mean() <= (0.1 if d <= 12 else 0.6), (kind, d, m, (~rob).mean())     # deeper, a voxel spans fewer float32 steps
            assert ((got["node"] >= 0) == w[m]["hit"])[rob].all(), (kind, d, m)
            if m != q.ANY:
                assert (got["node"] == w[m]["leaf"])[rob].all(), (kind, d, m)
    for m in MODES:
        _hits_equal(res[rto.KERNEL_AUTO, m], res[rto.KERNEL_GENERIC, m], f"{kind}{d} mode {m}: descriptor vs node kernel",
                    mask_only=(m == q.ANY))
    ctx.set_kernel(rto.KERNEL_AUTO)


def _permuted(nodes, rng):
    """The same tree under another numbering: root kept at 0, every other node moved, child indices remapped."""
    n = len(nodes)
    perm = np.concatenate([[0], 1 + rng.permutation(n - 1)])          # new index of old node i = perm[i]
    out = np.zeros_like(nodes)
    out[perm] = nodes
    ch = out["child"]
    out["child"] = np.where(ch >= 0, perm[np.maximum(ch, 0)], -1)
    return out, perm


@gpu
def test_same_records_on_canonical_permuted_and_gpu_built_arrays(ctx, scenes):
    """The same rays give the same records up to the node mapping on: the canonical array, a non-canonical numbering of it, and the
    octree rto_build_octree makes, where `node` indexes rto_download_nodes and that node's x/y/z/size and isSolid agree."""
    s = scenes("sphere64")
    T = q.Tree32(s.nodes, s.min, s.voxel)
    o, d, tmn, tmx = q.seeded_rays(T, 4096, 21)
    _upload(ctx, s)
    base = {m: ctx.query_rays(o, d, tmn, tmx, m) for m in MODES}
    assert ctx.info().canonical == 1
    perm_nodes, perm = _permuted(s.nodes, np.random.default_rng(5))
    ctx.upload_octree(perm_nodes, s.min, s.voxel)
    assert ctx.info().canonical == 0
    for m in MODES:
        got = ctx.query_rays(o, d, tmn, tmx, m)
        mapped = base[m].copy()
        h = mapped["node"] >= 0
        mapped["node"][h] = perm[mapped["node"][h]]
        _hits_equal(got, mapped, f"mode {m}: permuted array", mask_only=(m == q.ANY))
    ctx.build_octree(s.grid.data, s.min, s.voxel)
    built = ctx.download_nodes()
    assert built.tobytes() == s.nodes.tobytes()
    for m in MODES:
        got = ctx.query_rays(o, d, tmn, tmx, m)
        _hits_equal(got, base[m], f"mode {m}: rto_build_octree's tree", mask_only=(m == q.ANY))
        h = got["node"] >= 0
        nd = built[got["node"][h]]
        assert (nd["x"] == got["x"][h]).all() and (nd["y"] == got["y"][h]).all() and (nd["z"] == got["z"][h]).all()
        assert (nd["size"] == got["size"][h]).all() and (nd["isSolid"] == 1).all()


@gpu
def test_records_ignore_the_frustum(ctx, orc, scenes):
    """rto_update_frustum(enable=1) with a camera that culls most nodes changes no record: queries see the whole octree."""
    s = scenes("sphere64")
    _upload(ctx, s)
    T = q.Tree32(s.nodes, s.min, s.voxel)
    o, d, tmn, tmx = q.seeded_rays(T, 4096, 31)
    xy = _all_pixels(64, 48)
    view, pos = make_camera(orc, *SPHERE_CAM)
    rto = _rto()
    f = rto.make_frame(view, pos, 64 / 48, FOV, 64, 48)
    before = {m: (ctx.query_rays(o, d, tmn, tmx, m), ctx.query_pixels(f, xy, m)) for m in MODES}
    # a narrow camera looking away from most of the volume, margin-free planes (the reference's margin keeps everything)
    planes = np.array([[1, 0, 0, 0.45], [-1, 0, 0, -0.40], [0, 1, 0, 0.5], [0, -1, 0, 0.5], [0, 0, 1, 0.5], [0, 0, -1, 0.5]], np.float32)
    ctx.debug_update_frustum_planes(planes, 0.0)
    assert ctx.info().culling_active == 1 and ctx.info().visible_nodes < len(s.nodes) // 4
    for m in MODES:
        _hits_equal(ctx.query_rays(o, d, tmn, tmx, m), before[m][0], f"mode {m}: rays after a frustum update")
        _hits_equal(ctx.query_pixels(f, xy, m), before[m][1], f"mode {m}: pixels after a frustum update")
    ctx.update_frustum(view, FOV, 64 / 48, enable=False)


@gpu
def test_sizes_streams_and_errors(ctx, orc, scenes):
    """n of 0, 1, 63, 65 and 2^22; device queries on a caller's stream ordered after an upload; the error codes."""
    torch = pytest.importorskip("torch")
    rto = _rto()
    from ray_tracing_octrees_amd import hip
    s = scenes("sphere64")
    T = q.Tree32(s.nodes, s.min, s.voxel)
    o, d, tmn, tmx = q.seeded_rays(T, 4096, 41)
    rays = hip.make_rays(o, d, tmn, tmx)
    _upload(ctx, s)
    full = ctx.query_ray_records(rays, q.CLOSEST)
    for n in (1, 63, 65):
        _hits_equal(ctx.query_ray_records(rays[:n], q.CLOSEST), full[:n], f"n = {n}")
    assert len(ctx.query_ray_records(rays[:0], q.CLOSEST)) == 0
    big = np.resize(rays, 1 << 22)
    got = ctx.query_ray_records(big, q.FIRST)
    ref = ctx.query_ray_records(rays, q.FIRST)
    _hits_equal(got, np.resize(ref, 1 << 22), "n = 2^22")
    # device form on a non-default stream, right behind an upload of another scene and back
    other = torch.cuda.Stream()
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda")
    d_hits = torch.zeros(len(rays) * 32, dtype=torch.uint8, device="cuda")
    ctx.upload_octree(scenes("odd").nodes, scenes("odd").min, scenes("odd").voxel)
    _upload(ctx, s)
    torch.cuda.synchronize()
    ctx.query_rays_device(q.CLOSEST, d_rays.data_ptr(), len(rays), d_hits.data_ptr(), other.cuda_stream)
    other.synchronize()
    _hits_equal(d_hits.cpu().numpy().view(hip.HIT_DTYPE), full, "device form on a caller's stream")
    xy = torch.from_numpy(_all_pixels(32, 24)).to("cuda")
    view, pos = make_camera(orc, *SPHERE_CAM)
    f = rto.make_frame(view, pos, 32 / 24, FOV, 32, 24)
    d_ph = torch.zeros(32 * 24 * 32, dtype=torch.uint8, device="cuda")
    ctx.query_pixels_device(q.FIRST, f, xy.data_ptr(), 32 * 24, d_ph.data_ptr(), other.cuda_stream)
    other.synchronize()
    _hits_equal(d_ph.cpu().numpy().view(hip.HIT_DTYPE), ctx.query_pixels(f, _all_pixels(32, 24), q.FIRST), "pixels, device form")
    # pixels outside the frame: misses, not errors
    out = ctx.query_pixels(f, np.array([[-1, 0], [0, -1], [32, 0], [0, 24], [5, 5]], np.int32), q.FIRST)
    assert (out["node"][:4] == -1).all() and (out["t"][:4] == np.float32(1e30)).all()
    # error codes
    L = ctx._L
    hits = np.zeros(4, hip.HIT_DTYPE)
    assert L.rto_query_rays_host(ctx._h, 7, rays.ctypes.data, 4, hits.ctypes.data) == hip.RTO_E_INVALID
    assert L.rto_query_rays_host(ctx._h, 1, None, 4, hits.ctypes.data) == hip.RTO_E_INVALID
    assert L.rto_query_rays_host(ctx._h, 1, rays.ctypes.data, 4, None) == hip.RTO_E_INVALID
    assert L.rto_query_rays_host(ctx._h, 1, None, 0, None) == hip.RTO_OK
    assert L.rto_query_rays_device(ctx._h, 1, None, 4, d_hits.data_ptr(), None) == hip.RTO_E_INVALID
    assert L.rto_query_pixels_host(ctx._h, 3, C.byref(f), xy.data_ptr(), 4, hits.ctypes.data) == hip.RTO_E_INVALID
    assert L.rto_query_pixels_host(ctx._h, 0, C.byref(f), None, 4, hits.ctypes.data) == hip.RTO_E_INVALID
    fresh = rto.Context(0)
    try:
        with pytest.raises(hip.RtoError) as e:
            fresh.query_rays(o[:4], d[:4])
        assert e.value.code == hip.RTO_E_NO_OCTREE
        with pytest.raises(hip.RtoError) as e:
            fresh.query_pixels(f, _all_pixels(4, 4))
        assert e.value.code == hip.RTO_E_NO_OCTREE
    finally:
        fresh.close()


@gpu
def test_drop_in_class_intersect_rays_and_pick(orc, scenes):
    """RayTracerBVH::intersectRays equals the C ABI; pick at sampled pixels hits exactly where renderSceneCompute's frame is lit, and
    the frame's pixel is the shade of the picked leaf."""
    rto = _rto()
    W, H = 96, 72
    grid = rto.VoxelGrid.test_sphere(64)
    root = rto.createOctreeFromVoxelGrid(grid)
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    rt.setOctree(root, grid)
    s = scenes("sphere64")
    T = q.Tree32(s.nodes, s.min, s.voxel)
    o, d, tmn, tmx = q.seeded_rays(T, 2048, 51, windows_too=False)
    ctx = rto.Context(0)
    try:
        ctx.upload_octree(s.nodes, s.min, s.voxel)
        for m in MODES:
            got = rt.intersectRays(o, d, m, 0.0, 1e30)
            _hits_equal(got, ctx.query_rays(o, d, 0.0, 1e30, m), f"intersectRays mode {m}", mask_only=(m == q.ANY))
        got = rt.intersectRays(o, d, q.CLOSEST, 0.05, 0.9)
        _hits_equal(got, ctx.query_rays(o, d, 0.05, 0.9, q.CLOSEST), "intersectRays with a window")
    finally:
        ctx.close()
    cam = rto.Camera(*SPHERE_CAM)
    rt.renderSceneCompute(cam, W, H, W / H, FOV)
    img = rt.framebuffer()
    assert img is not None
    rd = _pixel_rays(orc, cam.getView(), cam.getPos(), W, H)
    rng = np.random.default_rng(3)
    pix = np.concatenate([rng.integers(0, [W, H], (300, 2)), [[W // 2, H // 2], [0, 0], [W - 1, H - 1]]])
    lit = 0
    for px, py in pix:
        h = rt.pick(cam, int(px), int(py), W, H, W / H, FOV)
        want = img[py, px]
        assert (h is not None) == bool(want[0] > 0.05), (px, py)
        if h is not None:
            lit += 1
            rec = np.array([h], q.HIT_DTYPE)
            sh = q.shade32(T, cam.getPos(), rd[py * W + px][None, :], rec)[0]
            assert sh.tobytes() == want.tobytes(), (px, py)
    assert lit > 20
    rto.freeOctree(root)
