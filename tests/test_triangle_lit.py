"""The lit render of the triangle surface (rto_render_lit_triangles_*, Context.render_lit_triangles_*,
RayTracerBVH::renderSurfaceLit): the triangle render's frame with a shadow ray and ambient occlusion per hit pixel.  CPU: the
float32 statement (tests/tri_lit_ref.py) against the oracle's triangle frames, the tangent frame, float64 and an analytic scene;
exports and the built assembly of the k_trilit_* kernels.  GPU: frames and visibility against that statement, bit for bit."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import deep_scenes as ds
import lit_ref as lr
import query_ref as q
import ref64
import tri_lit_ref as tl
import tri_query_ref as tq
from conftest import SPHERE_CAM, make_camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOV = 45.0
VGPR_BUDGET = 80            # k_triq_desc's budget, 6 waves per SIMD
SETTINGS = ((0, 0), (1, 0), (0, 1), (1, 8), (1, 64), (1, 3), (0, 5), (1, 48))      # K = 3, 5, 48: a hit's AO rays straddle waves
LIGHTS = ((-1.0, -1.0, -1.0), (0.3, -0.8, 0.45), (0.0, -1.0, 0.0))   # the renders' light, an oblique one, an axis-aligned one
SYMS = ("rto_render_lit_triangles_device", "rto_render_lit_triangles_host")
EXCLUDED_CAP = 1e-3         # the issue's: FIRST / ANY disagreement on at most 0.1 % of the shadow-casting pixels


def _hip():
    from ray_tracing_octrees_amd import hip
    return hip


def _table():
    return _hip().ao_directions()


def _rays(orc, view, pos, W, H, fov=FOV):
    return orc.generate_rays(view, pos, W / H, fov, W, H).reshape(-1, 3)


def _tq_scene(orc, name):
    import test_triangle_queries as ttq
    return ttq._scene(orc, name)


def _camera(orc, s, name):
    """(view, pos) of an orbit camera aimed at the grid's centre: "outside", "axis" (theta = phi = 0) or "inside" (the outside
    camera's view from the grid's centre: inside the surface for the closed scenes)."""
    centre = s.min.astype(np.float64) + np.array(s.grid.dims, np.float64) * float(s.voxel) / 2
    R = float(np.float32(1.6 * float(np.array(s.grid.dims).max()) * float(s.voxel)))
    th, ph = (0.0, 0.0) if name == "axis" else (0.6, 0.45)
    cam = orc.Camera(th, ph, R)
    cam.set_target(*[float(v) for v in centre.astype(np.float32)])
    view, pos = cam.get_view(), cam.get_pos()
    if name == "inside":
        pos = (centre + np.array([0.013, -0.021, 0.017]) * float(s.voxel)).astype(np.float32)
    return view, pos


def _excluded(casts, f, a):
    """Pixels whose shadow ray has different FIRST and ANY verdicts, and their share of the shadow-casting pixels."""
    ex = casts & (f != a)
    return ex, ex.sum() / max(1, int(casts.sum()))


# ================================================================ CPU
@pytest.mark.parametrize("name", ["sphere32", "two_blobs", "shell_window", "eye_inside", "far200", "terraces"])
def test_statement_without_terms_is_the_oracle_frame(orc, name):
    """tri_lit_ref with shadow off and K = 0 (default light) is orc.render_triangles' frame bit for bit; with the shadow ray alone
    it is the oracle's shadowed frame on every pixel whose shadow ray has the same verdict under FIRST and ANY, and those are all
    but at most 0.1 % of the casting pixels.  Counted here: 0 excluded pixels in every one of the six scenes."""
    g, nodes, tris, off, view, pos, W, H, fov, _ = _tq_scene(orc, name)
    T = q.Tree32(nodes, g.min, g.voxel_size)
    rd = _rays(orc, view, pos, W, H, fov)
    first = tq.query_tri32(T, tris, off, pos, rd)[tq.FIRST]
    img, vis = tl.tri_lit_frame(T, tris, off, g.voxel_size, pos, rd, W, H, _table(), shadow=False, K=0, first=first)
    plain, _ = orc.render_triangles(nodes, tris, off, g.min, g.voxel_size, view, pos, W / H, fov, W, H, shadow=False)
    assert img.tobytes() == plain.reshape(H, W, 4).tobytes()
    assert set(np.unique(vis)) <= {-1, 0} and (vis == 0).sum() > 50
    assert ((vis >= 0).ravel() == (first["tri"] >= 0)).all()
    img, vis = tl.tri_lit_frame(T, tris, off, g.voxel_size, pos, rd, W, H, _table(), shadow=True, K=0, first=first)
    dark, _ = orc.render_triangles(nodes, tris, off, g.min, g.voxel_size, view, pos, W / H, fov, W, H, shadow=True)
    hit, f, a = tl.shadow_verdicts(T, tris, off, g.voxel_size, pos, rd, first=first)
    casts = hit & (tq.lambert(first) > 0)
    ex, share = _excluded(casts, f, a)
    print(f"{name}: {int(ex.sum())} of {int(casts.sum())} shadow-casting pixels excluded (FIRST != ANY)")
    assert share <= EXCLUDED_CAP, (name, int(ex.sum()), int(casts.sum()))
    same = (img.reshape(-1, 4).view(np.uint32) == dark.reshape(-1, 4).view(np.uint32)).all(1)
    assert same[~ex].all(), f"{name}: {int((~same[~ex]).sum())} pixels differ from the oracle's shadowed frame"
    assert ((vis.ravel() >= 256) == (casts & a)).all()


def _mc_normals(orc):
    g = orc.test_sphere_grid(64)
    nodes = orc.build_flat_octree(g)
    tris, _ = orc.build_leaf_triangles(g, nodes)
    return np.asarray(tris, np.float32).reshape(-1, 12)[:, 9:12]


def test_tangent_frame_is_orthonormal(orc):
    """For the 64 table entries x (axis-aligned normals, both signs of z, n.z = +-0, seeded unit normals, the Marching-Cubes normals
    of sphere64, each also negated): U, V, n are orthonormal to 1e-6 and dir . n = z' to 1e-6, in float64 arithmetic on the float32
    values.  The tolerances bound a dozen float32 roundings (2^-24 each) of unit-size values; they are not measurements."""
    rng = np.random.default_rng(17)
    axes = np.float32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    zero_z = np.float32([[1, 0, 0.0], [1, 0, -0.0], [0.6, 0.8, 0.0], [0.6, -0.8, -0.0]])
    v = rng.normal(size=(2000, 3))
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    near = np.float32([[1e-4, 0, -1], [0, 1e-4, -1], [1e-3, 1e-3, 1], [3e-4, -2e-4, -1]])
    near = (near / np.linalg.norm(near.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    mc = _mc_normals(orc)
    mc = mc[rng.choice(len(mc), 4000, replace=False)]
    n = np.concatenate([axes, zero_z, v, near, mc, -mc]).astype(np.float32)
    assert (np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1) < 1e-6).all()
    assert (np.signbit(n[:, 2]) & (n[:, 2] == 0)).any()                  # a -0 is among them
    Uv, Vv = tl.tangent_frame(n)
    assert np.isfinite(Uv).all() and np.isfinite(Vv).all()
    u, v_, m = Uv.astype(np.float64), Vv.astype(np.float64), n.astype(np.float64)
    dot = lambda a, b: (a * b).sum(-1)                                   # noqa: E731
    for a, b, want in ((u, u, 1), (v_, v_, 1), (u, v_, 0), (u, m, 0), (v_, m, 0)):
        assert np.abs(dot(a, b) - want).max() <= 1e-6
    T = _table()
    for bits in (0, 64, 128, 192):
        h = np.full(len(n), bits, np.uint32)
        dirs = tl.ao_dirs(T, h, n, 64)                                   # every table entry, in order
        assert np.isfinite(dirs).all()
        dn = (dirs.astype(np.float64) * m[:, None, :]).sum(-1)
        assert np.abs(dn - T[None, :, 2].astype(np.float64)).max() <= 1e-6


@pytest.mark.parametrize("name", ["sphere32", "two_blobs"])
def test_statement_against_float64_on_robust_rays(orc, name):
    """tri_lit_ref's decisions against float64 (ref64.TriScene64): primary hits agree with trace_dfs on robust rays; every
    shadow and AO verdict agrees with any_hits where float64 calls it sure (a hit beyond float32's error, and for AO every
    candidate well inside the window) or impossible (no candidate pair inside the window); the decided share is large."""
    g, nodes, tris, off, view, pos, W, H, fov, _ = _tq_scene(orc, name)
    T = q.Tree32(nodes, g.min, g.voxel_size)
    S = ref64.TriScene64(nodes, tris, off, g.min, g.voxel_size)
    W, H = 48, 36
    rd = _rays(orc, view, pos, W, H, fov)
    yy, xx = np.mgrid[0:H, 0:W]
    rays = {}
    radius = float(np.float32(4 * float(g.voxel_size)))
    tl.tri_lit32(T, tris, off, g.voxel_size, pos, rd, xx.ravel(), yy.ravel(), _table(), light_dir=(0.3, -0.8, 0.45), shadow=True, K=8,
                 radius=radius, seed=5, rays_out=rays)
    o64 = np.broadcast_to(np.asarray(pos, np.float64), rd.shape).copy()
    ref = S.trace_dfs(o64, rd.astype(np.float64))
    first = rays["first"]
    assert ((first["tri"] >= 0) == ref["hit"])[ref["hit_robust"]].all()
    assert (first["tri"] == ref["tri"])[ref["robust"]].all() and ref["robust"].mean() > 0.9
    for kind, tmax in (("shadow", np.inf), ("ao", radius)):
        o, d, got = rays[kind][:3]
        pr, _, t, sure = S.any_hits(o.astype(np.float64), d.astype(np.float64))
        inwin = (t > 0) & (t <= tmax * (1 + 1e-4))
        possible = np.zeros(len(d), bool); possible[pr[inwin]] = True
        deep = np.ones(len(d), bool)                                   # every candidate pair well inside the window
        deep[pr[~((t > 0) & (t <= tmax * (1 - 1e-4)))]] = False
        sure_hit, sure_miss = sure & deep, ~possible
        assert (sure_hit | sure_miss).mean() > 0.8, (kind, (sure_hit | sure_miss).mean())
        assert got[sure_hit].all() and not got[sure_miss].any(), kind
    assert rays["ao"][2].any() and (~rays["ao"][2]).any() and rays["shadow"][2].any()


def _floor_pillar(orc):
    """A 32^3 grid (voxel 1, origin 0): a floor slab y in [0, 2) and a pillar x, z in [14, 18), y in [2, 20); its octree and the
    Marching-Cubes leaf triangles the host's LocalMC builds."""
    data = np.zeros((32, 32, 32), np.uint8)            # (z, y, x)
    data[:, 0:2, :] = 1
    data[14:18, 2:20, 14:18] = 1
    g = orc.Grid((32, 32, 32), np.zeros(3, np.float32), np.float32(1.0), data)
    from ray_tracing_octrees_amd import host
    hg = host.VoxelGrid.from_array(data, g.min, g.voxel_size)
    root = host.createOctreeFromVoxelGrid(hg)
    nodes = root.flatten()
    tris, off = host.buildLeafTriangles(hg, nodes)                  # the C++ host builder: LocalMC per leaf, no GPU
    host.freeOctree(root)
    return g, nodes, tris, off


def test_shadow_and_ao_of_a_pillar_on_a_floor(orc):
    """Rays straight down onto the floor's Marching-Cubes surface, light from above at an angle: the shadowed floor points are
    those the pillar's analytic shadow covers (away from its edge by a voxel: the surface lies half a voxel inside the boxes);
    AO is 1 on the open floor far from the pillar and below 1 beside it."""
    g, nodes, tris, off = _floor_pillar(orc)
    T = q.Tree32(nodes, g.min, g.voxel_size)
    tris = np.asarray(tris, np.float32).reshape(-1, 12)
    light = (0.5, -1.0, 0.3)                            # travels down, towards +x and +z: shadows fall towards -x, -z
    xs, zs = np.meshgrid(np.arange(2.25, 30, 0.5), np.arange(2.25, 30, 0.5))
    px, pz = xs.ravel(), zs.ravel()
    keep = ~((px > 12.5) & (px < 19.5) & (pz > 12.5) & (pz < 19.5))          # the pillar's top, and its foot, is not open floor
    px, pz = px[keep], pz[keep]
    o = np.stack([px, np.full_like(px, 30.0), pz], 1).astype(np.float32)
    d = np.broadcast_to(np.float32([0, -1, 0]), o.shape).copy()
    ix, iz = np.floor(px).astype(int), np.floor(pz).astype(int)
    rays = {}
    rgba, vis = tl.tri_lit32(T, tris, off, g.voxel_size, o, d, ix, iz, _table(), light_dir=light, shadow=True, K=16, radius=4.0,
                             seed=3, rays_out=rays)
    assert (vis >= 0).all()
    first = rays["first"]
    fy = 30.0 - first["t"].astype(np.float64)            # the floor's surface height where each ray lands
    assert (np.abs(fy - fy[0]) < 1e-3).all() and 1.0 <= fy[0] <= 2.0
    assert (first["ny"] > 0.99).all()                    # flat floor, normal up
    # analytic: from (px, fy, pz) along (-0.5, 1, -0.3) u the pillar's surface is x, z in [14 -+ 0.5, 18 +- 0.5], y up to 20 -+ 0.5
    def overlap(margin):
        top = 19.5 - fy[0]
        lo = np.maximum.reduce([np.zeros_like(px), 2 * (px - 18) - margin, (pz - 18) / 0.3 - margin])
        hi = np.minimum.reduce([np.full_like(px, top), 2 * (px - 14) + margin, (pz - 14) / 0.3 + margin])
        return hi - lo
    inside, outside = overlap(-2.5) > 0, overlap(2.5) < 0
    shadowed = vis >= 256
    assert inside.sum() > 50 and outside.sum() > 1000
    assert shadowed[inside].all() and not shadowed[outside].any()
    assert (rgba[shadowed, 0] < rgba[~shadowed, 0].min()).all()         # a shadowed floor point is darker than every lit one
    _, vis64 = tl.tri_lit32(T, tris, off, g.voxel_size, o, d, ix, iz, _table(), light_dir=light, shadow=False, K=64, radius=4.0,
                            seed=3, first=first)
    occ = vis64 & 255
    dist = np.maximum(np.maximum(14 - px, px - 18), np.maximum(14 - pz, pz - 18))          # Chebyshev distance to the pillar
    far, corner = dist > 5.01, dist < 2.0
    assert far.sum() > 100 and corner.sum() > 10
    assert (occ[far] == 0).all() and (occ[corner] > 0).all()                              # A = 1 far away, A < 1 in the corner
    assert (vis64 < 256).all() and ((vis & 255)[far] == 0).all()


def test_exports_and_signatures():
    """The two entry points are declared with the stated signatures, listed in SYMBOLS, bound with matching argtypes and exported by
    the built library; rto_lighting is reused as it is (32 bytes)."""
    hip = _hip()
    hdr = open(os.path.join(ROOT, "include", "rto_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert ("int rto_render_lit_triangles_device(rto_context* ctx, const rto_frame* frame, const rto_lighting* lighting, void* d_rgba, "
            "int32_t* d_vis , void* hip_stream);") in flat
    assert ("int rto_render_lit_triangles_host(rto_context* ctx, const rto_frame* frame, const rto_lighting* lighting, float* host_rgba, "
            "int32_t* host_vis );") in flat
    assert C.sizeof(hip.Lighting) == 32
    lib = C.CDLL(os.path.join(ROOT, "ray_tracing_octrees_amd", "librto_hip.so"))
    for s in SYMS:
        assert s in hip.SYMBOLS and hasattr(lib, s), s
    L = hip.load()
    assert len(L.rto_render_lit_triangles_device.argtypes) == 6 and len(L.rto_render_lit_triangles_host.argtypes) == 5
    assert hasattr(hip.Context, "render_lit_triangles_host") and hasattr(hip.Context, "render_lit_triangles_device")
    from ray_tracing_octrees_amd import host
    assert hasattr(host.RayTracerBVH, "renderSurfaceLit")


def test_trilit_kernels_keep_their_budgets():
    """The built assembly (the product's flags): the two k_trilit_* kernels without scratch instructions, spills or v_mfma, within
    80 VGPRs; the lit, box-query and triangle-query kernels are all still there."""
    import test_isa_contract as isa
    asm = isa.built_asm()
    if asm is None:
        pytest.fail("no hipcc: the budget cannot be checked")
    meta = isa.kernel_meta(asm)
    names = [k for k in meta if "k_trilit_" in k]
    assert len(names) == 2, names
    assert len([k for k in meta if "k_lit_" in k]) == 2
    assert len([k for k in meta if "k_query_" in k]) == 12 and len([k for k in meta if "k_triq_" in k]) == 12
    for k in names:
        m = meta[k]
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (k, m)
        assert m["vgpr"] <= VGPR_BUDGET, (k, m)
        ins = isa.body(asm, k[len("_ZN3rto"):].split("E")[0])
        assert not any(t.startswith(("scratch_", "buffer_load", "buffer_store")) or "v_mfma" in t for t in ins), k
        assert not any("v_writelane" in t or "v_readlane" in t for t in ins), k          # no scalar register parked in a vector lane


# ================================================================ GPU
gpu = pytest.mark.gpu


def _rto():
    import ray_tracing_octrees_amd as rto
    return rto


def _light(light=(-1.0, -1.0, -1.0), shadow=0, K=0, radius=1.0, seed=0):
    return _hip().make_lighting(light, bool(shadow), K, radius, seed)


def _equal(got, want, what):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape, what
    neq = (g.view(np.uint32) != w.view(np.uint32)).reshape(g.shape[0], g.shape[1], -1).any(-1)
    assert not neq.any(), f"{what}: {int(neq.sum())} pixels differ, e.g. {np.argwhere(neq)[:4].tolist()}"


def _resident(ctx, s):
    """Upload the scene's octree, build its leaf triangles on the GPU, and return them."""
    rto = _rto()
    ctx.set_kernel(rto.KERNEL_AUTO)
    ctx.upload_octree(s.nodes, s.min, s.voxel)
    ctx.build_leaf_triangles(s.grid.data)
    tris, off = ctx.download_leaf_triangles()
    return np.asarray(tris, np.float32).reshape(-1, 12), off


def _check(ctx, T, tris, off, voxel, f, pos, rd, W, H, light, sh, K, radius, seed, what, first=None):
    img, vis = ctx.render_lit_triangles_host(f, _light(light, sh, K, radius, seed), vis=True)
    want, wvis = tl.tri_lit_frame(T, tris, off, voxel, pos, rd, W, H, _table(), light_dir=light, shadow=sh, K=K, radius=radius, seed=seed,
                                  first=first)
    _equal(img, want, what)
    assert (vis == wvis).all(), f"{what}: visibility differs at {int((vis != wvis).sum())} pixels"
    return vis


@gpu
@pytest.mark.parametrize("scene", ["sphere64", "odd", "calgary"])
@pytest.mark.parametrize("cam", ["outside", "inside", "axis"])
def test_frames_match_the_statement(ctx, orc, scenes, scene, cam):
    """RGBA and visibility bit for bit against tri_lit_ref, triangles from rto_build_leaf_triangles: every (shadow, K) setting
    under each of the three lights, and two seeds wherever AO runs (the seed enters nothing else)."""
    rto = _rto()
    s = scenes(scene)
    tris, off = _resident(ctx, s)
    T = q.Tree32(s.nodes, s.min, s.voxel)
    view, pos = _camera(orc, s, cam)
    W, H = 32, 24
    f = rto.make_frame(view, pos, W / H, FOV, W, H)
    rd = _rays(orc, view, pos, W, H)
    first = tq.query_tri32(T, tris, off, pos, rd)[tq.FIRST]
    radius = float(np.float32(4 * float(s.voxel)))
    hits = occluded = 0
    for light in LIGHTS:
        for sh, K in SETTINGS:
            for seed in ((0, 0x9E3779B9) if K else (0,)):
                vis = _check(ctx, T, tris, off, s.voxel, f, pos, rd, W, H, light, sh, K, radius, seed,
                             f"{scene}/{cam} light {light} shadow {sh} K {K} seed {seed}", first)
                hits += int((vis >= 0).sum())
                occluded += int((vis > 0).sum())
    assert hits > 0 and occluded > 0


@gpu
def test_a_frame_smaller_than_one_tile(ctx, orc, scenes):
    """sphere64 at 5 x 3, every (shadow, K) setting bit for bit against tri_lit_ref: the frame is part of one 8x8 tile, so three
    of its workgroup's four waves lie behind the last tile, and with at most 15 hits the shadow rays fill part of one wave and the
    AO rays start at the padding alone (ray 64, or 0 without the shadow term)."""
    rto = _rto()
    s = scenes("sphere64")
    tris, off = _resident(ctx, s)
    T = q.Tree32(s.nodes, s.min, s.voxel)
    view, pos = make_camera(orc, 0.6, 0.45, 1.0)                    # nine of the fifteen pixels hit
    W, H = 5, 3
    f = rto.make_frame(view, pos, W / H, FOV, W, H)
    rd = _rays(orc, view, pos, W, H)
    first = tq.query_tri32(T, tris, off, pos, rd)[tq.FIRST]
    radius = float(np.float32(4 * float(s.voxel)))
    hits = occluded = 0
    for sh, K in SETTINGS:
        vis = _check(ctx, T, tris, off, s.voxel, f, pos, rd, W, H, LIGHTS[1], sh, K, radius, 0x9E3779B9, f"5x3 shadow {sh} K {K}", first)
        hits += int((vis >= 0).sum())
        occluded += int((vis > 0).sum())
    assert hits == 9 * len(SETTINGS) and occluded > 0


def _identity_case(ctx, orc, g, view, pos, W, H, sample):
    """(0, 0) is rto_render_triangles(shadow = 0) on the whole frame; (1, 0) is its shadowed frame on the sampled pixels whose shadow
    ray has one verdict under FIRST and ANY in tri_query_ref.  Returns (excluded, casting) of the sample."""
    rto = _rto()
    ctx.set_kernel(rto.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    ctx.build_leaf_triangles()
    f = rto.make_frame(view, pos, W / H, FOV, W, H)
    img, vis = ctx.render_lit_triangles_host(f, _light(), vis=True)
    plain = ctx.render_triangles_host(f, shadow=False)
    _equal(img, plain, "no terms vs render_triangles(shadow=0)")
    assert ((vis >= 0) == (plain[..., 0] > 0.05)).all() and (vis >= 0).any()
    img, vis = ctx.render_lit_triangles_host(f, _light(shadow=1), vis=True)
    dark = ctx.render_triangles_host(f, shadow=True)
    nodes = ctx.download_nodes()
    tris, off = ctx.download_leaf_triangles()
    T = q.Tree32(nodes, g.min, g.voxel_size)
    rd = _rays(orc, view, pos, W, H)[sample]
    hit, fv, av = tl.shadow_verdicts(T, tris, off, g.voxel_size, pos, rd)
    first = tq.query_tri32(T, tris, off, pos, rd)[tq.FIRST]
    casts = hit & (tq.lambert(first) > 0)
    ex, share = _excluded(casts, fv, av)
    print(f"{W}x{H}: {int(ex.sum())} of {int(casts.sum())} sampled shadow-casting pixels excluded (FIRST != ANY)")
    assert casts.sum() > 1000 and share <= EXCLUDED_CAP, (int(ex.sum()), int(casts.sum()))
    got, want = img.reshape(-1, 4)[sample], dark.reshape(-1, 4)[sample]
    same = (got.view(np.uint32) == want.view(np.uint32)).all(1)
    assert same[~ex].all(), f"{int((~same[~ex]).sum())} sampled pixels differ from render_triangles(shadow=1)"
    assert ((vis.reshape(-1)[sample] >= 256) == (casts & av)).all()
    # off the sample the two frames may differ only where a shadow ray decides differently: a lit and a shadowed colour of one hit
    diff = (img.view(np.uint32) != dark.view(np.uint32)).any(-1)
    assert diff.mean() <= EXCLUDED_CAP, diff.mean()
    return int(ex.sum()), int(casts.sum())


@gpu
def test_identities_at_1080p(ctx, orc):
    """sphere 256^3 at 1920x1080: the two identities; the FIRST / ANY exclusion computed from tri_query_ref on a seeded sample of
    32,768 pixels.  Counted on the CPU for this scene and sample before the GPU test was written: 0 of 4,389 casting pixels
    excluded (none of them blocked: the shell does not shadow its lit side; test_identities_on_scenes_with_shadows has blocked ones)."""
    g = orc.test_sphere_grid(256)
    view, pos = make_camera(orc, *SPHERE_CAM)
    W, H = 1920, 1080
    sample = np.sort(np.random.default_rng(31).choice(W * H, 1 << 15, replace=False))
    _identity_case(ctx, orc, g, view, pos, W, H, sample)


@gpu
def test_identities_at_config5_size(ctx, orc):
    """Config 5's size (512^3 shell, 3840x2160, the default camera): the two identities, the exclusion on a seeded sample of 32,768
    pixels.  Counted on the CPU for this scene and sample before the GPU test was written: 0 of 4,337 casting pixels excluded."""
    g = orc.test_sphere_grid(512)
    view, pos = make_camera(orc, *SPHERE_CAM)
    W, H = 3840, 2160
    sample = np.sort(np.random.default_rng(32).choice(W * H, 1 << 15, replace=False))
    _identity_case(ctx, orc, g, view, pos, W, H, sample)


@gpu
@pytest.mark.parametrize("name", ["shell_window", "terraces"])
def test_identities_on_scenes_with_shadows(ctx, orc, name):
    """The two identities on whole frames of scenes whose shadow rays are blocked (uploaded triangles): 0 of 2,940 and 0 of 6,186
    casting pixels excluded, counted by test_statement_without_terms_is_the_oracle_frame."""
    rto = _rto()
    g, nodes, tris, off, view, pos, W, H, fov, _ = _tq_scene(orc, name)
    ctx.set_kernel(rto.KERNEL_AUTO)
    ctx.upload_octree(nodes, g.min, g.voxel_size)
    ctx.upload_leaf_triangles(tris, off)
    f = rto.make_frame(view, pos, W / H, fov, W, H)
    _equal(ctx.render_lit_triangles_host(f, _light()), ctx.render_triangles_host(f, shadow=False), f"{name}: no terms")
    T = q.Tree32(nodes, g.min, g.voxel_size)
    rd = _rays(orc, view, pos, W, H, fov)
    first = tq.query_tri32(T, tris, off, pos, rd)[tq.FIRST]
    hit, fv, av = tl.shadow_verdicts(T, tris, off, g.voxel_size, pos, rd, first=first)
    casts = hit & (tq.lambert(first) > 0)
    ex, share = _excluded(casts, fv, av)
    assert share <= EXCLUDED_CAP and (casts & av).sum() > 20
    img, vis = ctx.render_lit_triangles_host(f, _light(shadow=1), vis=True)
    dark = ctx.render_triangles_host(f, shadow=True)
    same = (img.reshape(-1, 4).view(np.uint32) == dark.reshape(-1, 4).view(np.uint32)).all(1)
    assert same[~ex].all(), f"{name}: {int((~same[~ex]).sum())} pixels differ from render_triangles(shadow=1)"
    assert ((vis.ravel() >= 256) == (casts & av)).all()


@gpu
@pytest.mark.parametrize("K", [8, 5])
def test_config5_lit_frame_on_a_seeded_sample(ctx, orc, K):
    """Config 5 (512^3, 3840x2160) with the shadow ray and K = 8 or 5 (hits straddling waves): a seeded sample of 65,536 draws (the
    distinct pixels among them, more than 60,000) equals tri_lit_ref bit for bit."""
    rto = _rto()
    g = orc.test_sphere_grid(512)
    ctx.set_kernel(rto.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    ctx.build_leaf_triangles()
    nodes = ctx.download_nodes()
    tris, off = ctx.download_leaf_triangles()
    W, H = 3840, 2160
    view, pos = make_camera(orc, *SPHERE_CAM)
    f = rto.make_frame(view, pos, W / H, FOV, W, H)
    radius = float(np.float32(4 * float(g.voxel_size)))
    img, vis = ctx.render_lit_triangles_host(f, _light(shadow=1, K=K, radius=radius, seed=11), vis=True)
    rng = np.random.default_rng(2025)
    lit_rows = np.nonzero((vis >= 0).any(1))[0]
    pick = rng.choice(W * H, 1 << 16, replace=False)
    pick[: 1 << 14] = (rng.choice(lit_rows, 1 << 14) * W + rng.integers(0, W, 1 << 14))     # a quarter from rows with geometry
    pick = np.unique(pick)                                            # the two draws may overlap: a few pixels fewer than 65,536
    assert len(pick) > 60000
    x, y = pick % W, pick // W
    rd = _rays(orc, view, pos, W, H)[pick]
    want, wvis = tl.tri_lit32(q.Tree32(nodes, g.min, g.voxel_size), tris, off, g.voxel_size, pos, rd, x, y, _table(), shadow=1, K=K,
                              radius=radius, seed=11)
    got = img.reshape(-1, 4)[pick]
    assert got.tobytes() == want.tobytes(), f"{int((got != want).any(1).sum())} of {len(pick)} pixels differ"
    assert (vis.reshape(-1)[pick] == wvis).all()
    assert ((wvis & 255) > 0).sum() > 100 and (wvis >= 0).sum() > 5000


@gpu
def test_uploaded_normals_that_are_not_unit_zero_or_not_finite(ctx, orc):
    """rto_upload_leaf_triangles with stored normals scaled, zeroed, made infinite or NaN on triangles the pixel rays hit: frames
    equal the statement (a secondary ray with a non-finite component is a miss).  Ordinary input of the ABI, checked once."""
    rto = _rto()
    g, nodes, tris, off, view, pos, W, H, fov, _ = _tq_scene(orc, "sphere32")
    tris = np.asarray(tris, np.float32).reshape(-1, 12).copy()
    T = q.Tree32(nodes, g.min, g.voxel_size)
    W, H = 40, 30
    rd = _rays(orc, view, pos, W, H, fov)
    hit = np.unique(tq.query_tri32(T, tris, off, pos, rd)[tq.FIRST]["tri"])
    hit = hit[hit >= 0]
    assert len(hit) > 60
    kinds = np.arange(len(hit)) % 6
    tris[hit[kinds == 0], 9:12] *= np.float32(3.5)
    tris[hit[kinds == 1], 9:12] *= np.float32(1e-3)
    tris[hit[kinds == 2], 9:12] = 0.0
    tris[hit[kinds == 3], 9] = np.inf
    tris[hit[kinds == 4], 10] = np.nan
    tris[hit[kinds == 5], 9:12] *= np.float32(1e30)
    ctx.set_kernel(rto.KERNEL_AUTO)
    ctx.upload_octree(nodes, g.min, g.voxel_size)
    ctx.upload_leaf_triangles(tris, off)
    f = rto.make_frame(view, pos, W / H, fov, W, H)
    radius = float(np.float32(4 * float(g.voxel_size)))
    for light, sh, K, seed in ((LIGHTS[0], 1, 8, 0), (LIGHTS[1], 1, 5, 3), (LIGHTS[2], 0, 64, 1), (LIGHTS[1], 1, 0, 0)):
        vis = _check(ctx, T, tris, off, g.voxel_size, f, pos, rd, W, H, light, sh, K, radius, seed, f"odd normals {light} {sh} {K}")
        assert (vis >= 0).sum() > 100


@gpu
@pytest.mark.parametrize("kind,d", [("far", 12), ("frac", 19), ("tenth", 20)])
def test_deep_octrees_with_spine_triangles(ctx, orc, kind, d):
    """Depth 12-20 spine trees with test_triangle_queries' uploaded triangles: every camera of the scene, shadow and K = 8."""
    import test_triangle_queries as ttq
    rto = _rto()
    s = ds.scene(kind, d, "spine")
    ctx.set_kernel(rto.KERNEL_AUTO)
    ctx.upload_octree(s.nodes, s.min, s.voxel)
    tris, off = ttq._spine_triangles(s)
    ctx.upload_leaf_triangles(tris, off)
    T = q.Tree32(s.nodes, s.min, s.voxel)
    W, H = 32, 24
    radius = float(np.float32(4 * float(s.voxel)))
    lit = 0
    for name, view, pos in s.cameras(orc):
        f = rto.make_frame(view, pos, W / H, FOV, W, H)
        vis = _check(ctx, T, tris, off, s.voxel, f, pos, _rays(orc, view, pos, W, H), W, H, (0.3, -0.8, 0.45), 1, 8, radius, 1,
                     f"{kind}{d} {name}")
        lit += int((vis >= 0).sum())
    assert lit > 0


@gpu
def test_deep_thin_octree(ctx, orc):
    """A depth-11 thin scene with the triangles rto_build_leaf_triangles makes of it."""
    rto = _rto()
    s = ds.scene("frac", 11, "thin")
    ctx.set_kernel(rto.KERNEL_AUTO)
    ctx.upload_octree(s.nodes, s.min, s.voxel)
    ctx.build_leaf_triangles(s.data)
    tris, off = ctx.download_leaf_triangles()
    T = q.Tree32(s.nodes, s.min, s.voxel)
    W, H = 32, 24
    radius = float(np.float32(4 * float(s.voxel)))
    lit = 0
    for name, view, pos in s.cameras(orc):
        f = rto.make_frame(view, pos, W / H, FOV, W, H)
        vis = _check(ctx, T, tris, off, s.voxel, f, pos, _rays(orc, view, pos, W, H), W, H, (0.3, -0.8, 0.45), 1, 5, radius, 1,
                     f"frac11 thin {name}")
        lit += int((vis >= 0).sum())
    assert lit > 0


@gpu
def test_a_tree_that_is_one_leaf_owns_no_triangles(ctx, orc):
    """A single-leaf tree with an (empty) triangle set resident: every pixel is a miss under every setting."""
    rto = _rto()
    hip = _hip()
    gmin, vs = np.float32([-1.0, -1.0, -1.0]), np.float32(0.25)
    solid = np.zeros(1, hip.NODE_DTYPE)
    solid["size"], solid["isLeaf"], solid["isUniform"], solid["isSolid"], solid["child"] = 8, 1, 1, 1, -1
    ctx.upload_octree(solid, gmin, vs)
    ctx.upload_leaf_triangles(np.zeros((0, 12), np.float32), np.zeros(2, np.int32))
    cam = orc.Camera(0.6, 0.45, 6.0)
    cam.set_target(0.0, 0.0, 0.0)
    W, H = 40, 30
    f = rto.make_frame(cam.get_view(), cam.get_pos(), W / H, FOV, W, H)
    for sh, K in ((0, 0), (1, 8), (0, 5)):
        img, vis = ctx.render_lit_triangles_host(f, _light((0.3, -0.8, 0.45), sh, K, 0.5, 9), vis=True)
        assert (vis == -1).all() and (img == np.float32([0, 0, 0, 1])).all()


@gpu
def test_carving_the_occluder_lights_its_shadow(ctx, orc):
    """Floor and pillar built on the GPU with triangles resident; a box brush carves the pillar away: the frames before and after
    equal tri_lit_ref on the downloaded tree and triangles, and pixels that were in shadow are lit."""
    rto = _rto()
    hip = _hip()
    g, _, _, _ = _floor_pillar(orc)
    ctx.set_kernel(rto.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    ctx.build_leaf_triangles()
    cam = orc.Camera(0.9, 0.9, 60.0)
    cam.set_target(16.0, 2.0, 16.0)
    view, pos = cam.get_view(), cam.get_pos()
    W, H = 64, 48
    f = rto.make_frame(view, pos, W / H, FOV, W, H)
    rd = _rays(orc, view, pos, W, H)
    light = (0.5, -1.0, 0.3)

    def frame(what):
        tris, off = ctx.download_leaf_triangles()
        T = q.Tree32(ctx.download_nodes(), g.min, g.voxel_size)
        return _check(ctx, T, tris, off, g.voxel_size, f, pos, rd, W, H, light, 1, 4, 3.0, 2, what)

    vb = frame("before the edit")
    changed = ctx.edit_voxels(hip.make_brushes([[16.0, 11.0, 16.0]], [[3.0, 9.5, 3.0]], hip.BRUSH_BOX, hip.EDIT_CARVE))
    assert changed > 0
    va = frame("after the edit")
    assert ((vb >= 256) & (va >= 0) & (va < 256)).sum() > 5


@gpu
def test_voxelized_mesh_is_lit(ctx, orc):
    """rto_voxelize_mesh + rto_build_leaf_triangles: the lit frame of the new scene equals the statement."""
    rto = _rto()
    hip = _hip()
    # a closed box mesh of 12 triangles, voxelized on a fixed 32^3 grid
    lo, hi = 6.3, 25.6
    v = np.array([[x, y, z] for z in (lo, hi) for y in (lo, hi) for x in (lo, hi)], np.float64)
    faces = np.array([[0, 1, 3], [0, 3, 2], [4, 7, 5], [4, 6, 7], [0, 5, 1], [0, 4, 5], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                      [1, 5, 7], [1, 7, 3]], np.int32)
    res = ctx.voxelize_mesh(v, faces, 1.0, grid=((32, 32, 32), (0.0, 0.0, 0.0), 1.0), triangles=True)
    assert res.filled > 0
    nodes = ctx.download_nodes()
    tris, off = ctx.download_leaf_triangles()
    assert len(tris) > 0
    gmin, vs = np.asarray(res.grid_min, np.float32), np.float32(res.voxel_size)
    T = q.Tree32(nodes, gmin, vs)
    cam = orc.Camera(0.6, 0.45, 70.0)
    cam.set_target(16.0, 16.0, 16.0)
    view, pos = cam.get_view(), cam.get_pos()
    W, H = 48, 36
    f = rto.make_frame(view, pos, W / H, FOV, W, H)
    vis = _check(ctx, T, tris, off, vs, f, pos, _rays(orc, view, pos, W, H), W, H, (0.3, -0.8, 0.45), 1, 8, 4.0, 6, "voxelized mesh")
    assert (vis >= 0).sum() > 100


@gpu
def test_same_seed_same_bytes_and_device_form(ctx, orc, scenes):
    """Two frames with the same seed are identical bytes; the device form on a caller's stream, with and without the visibility
    buffer, gives the host form's bytes; another seed changes some AO pixels and no shadow verdict."""
    torch = pytest.importorskip("torch")
    rto = _rto()
    s = scenes("sphere64")
    _resident(ctx, s)
    W, H = 320, 180
    view, pos = make_camera(orc, *SPHERE_CAM)
    f = rto.make_frame(view, pos, W / H, FOV, W, H)
    radius = float(np.float32(4 * float(s.voxel)))
    L = _light((0.3, -0.8, 0.45), 1, 8, radius, 7)
    a, va = ctx.render_lit_triangles_host(f, L, vis=True)
    b, vb = ctx.render_lit_triangles_host(f, L, vis=True)
    assert a.tobytes() == b.tobytes() and va.tobytes() == vb.tobytes()
    other = torch.cuda.Stream()
    d_rgba = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
    d_vis = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.render_lit_triangles_device(f, L, d_rgba.data_ptr(), d_vis.data_ptr(), other.cuda_stream)
    other.synchronize()
    assert d_rgba.cpu().numpy().tobytes() == a.tobytes() and d_vis.cpu().numpy().tobytes() == va.tobytes()
    d_rgba.zero_()
    torch.cuda.synchronize()
    ctx.render_lit_triangles_device(f, L, d_rgba.data_ptr(), 0, other.cuda_stream)
    other.synchronize()
    assert d_rgba.cpu().numpy().tobytes() == a.tobytes()
    c, vc = ctx.render_lit_triangles_host(f, _light((0.3, -0.8, 0.45), 1, 8, radius, 8), vis=True)
    assert ((vc & 255) != (va & 255)).any() and ((vc >= 256) == (va >= 256)).all()
    # the box lit render shares the work buffers: a frame of it in between changes nothing
    ctx.render_lit_host(f, L)
    assert ctx.render_lit_triangles_host(f, L).tobytes() == a.tobytes()


@gpu
def test_error_codes(ctx, orc, scenes):
    """RTO_E_INVALID for every bad argument of the lit render's list, RTO_E_NO_OCTREE on a fresh context and with an octree but no
    triangles, RTO_E_UNSUPPORTED for a non-canonical array; a refused call leaves the next frame unchanged."""
    torch = pytest.importorskip("torch")
    rto = _rto()
    hip = _hip()
    s = scenes("sphere64")
    tris, off = _resident(ctx, s)
    view, pos = make_camera(orc, *SPHERE_CAM)
    f = rto.make_frame(view, pos, 4 / 3, FOV, 32, 24)
    good = _light((-1.0, -1.0, -1.0), 1, 4, 0.05, 0)
    ref = ctx.render_lit_triangles_host(f, good)
    Lib, h = ctx._L, ctx._h
    out = np.zeros((24, 32, 4), np.float32)

    def rc(L, frame=f, buf=out):
        return Lib.rto_render_lit_triangles_host(h, C.byref(frame) if frame is not None else None, C.byref(L) if L is not None else None,
                                                 buf.ctypes.data if buf is not None else None, None)

    assert rc(good) == hip.RTO_OK
    assert rc(None) == hip.RTO_E_INVALID
    assert rc(good, frame=None) == hip.RTO_E_INVALID
    assert rc(good, buf=None) == hip.RTO_E_INVALID
    bad = []
    for field, value in (("ao_samples", -1), ("ao_samples", 65), ("reserved", 1)):
        L = _light((-1.0, -1.0, -1.0), 1, 4, 0.05, 0)
        setattr(L, field, value)
        bad.append(L)
    for radius in (0.0, -1.0, float("inf"), float("nan")):
        bad.append(_light((-1.0, -1.0, -1.0), 0, 4, radius, 0))
    for light in ((0.0, 0.0, 0.0), (float("nan"), -1.0, 0.0), (float("inf"), -1.0, 0.0), (1e-30, 0.0, 0.0)):
        bad.append(_light(light, 1, 0, 1.0, 0))
    for L in bad:
        assert rc(L) == hip.RTO_E_INVALID, (list(L.light_dir), L.shadow, L.ao_samples, L.ao_radius, L.reserved)
        assert ctx.render_lit_triangles_host(f, good).tobytes() == ref.tobytes()
    assert rc(_light((-1.0, -1.0, -1.0), 1, 0, float("nan"), 0)) == hip.RTO_OK          # K = 0: the radius is not used
    d_rgba = torch.zeros(32 * 24 * 4 + 4, dtype=torch.float32, device="cuda")
    d_vis = torch.zeros(32 * 24 + 1, dtype=torch.int32, device="cuda")
    dev = Lib.rto_render_lit_triangles_device
    assert dev(h, C.byref(f), C.byref(good), C.c_void_p(d_rgba.data_ptr() + 4), None, None) == hip.RTO_E_INVALID
    assert dev(h, C.byref(f), C.byref(good), C.c_void_p(d_rgba.data_ptr()), C.c_void_p(d_vis.data_ptr() + 2), None) == hip.RTO_E_INVALID
    assert dev(h, C.byref(f), C.byref(good), None, None, None) == hip.RTO_E_INVALID
    for W, H, K in ((65536, 65536, 0), (8192, 8192, 64), (46341, 46341, 1)):       # the lit render's 32-bit ray-index limits
        big = rto.make_frame(view, pos, W / H, FOV, W, H)
        assert rc(_light((-1.0, -1.0, -1.0), 1, K, 0.05, 0), frame=big) == hip.RTO_E_INVALID, (W, H, K)
        assert dev(h, C.byref(big), C.byref(_light((-1.0, -1.0, -1.0), 1, K, 0.05, 0)), C.c_void_p(d_rgba.data_ptr()), None, None) \
            == hip.RTO_E_INVALID, (W, H, K)
    assert rc(good, frame=rto.make_frame(view, pos, 4 / 3, FOV, 0, 24)) == hip.RTO_E_INVALID
    assert ctx.render_lit_triangles_host(f, good).tobytes() == ref.tobytes()
    # an octree without triangles: a new upload frees them; the box lit render still answers; triangles back: the frame is back
    ctx.upload_octree(s.nodes, s.min, s.voxel)
    with pytest.raises(hip.RtoError) as e:
        ctx.render_lit_triangles_host(f, good)
    assert e.value.code == hip.RTO_E_NO_OCTREE
    assert ctx.render_lit_host(f, good).shape == (24, 32, 4)
    ctx.upload_leaf_triangles(tris, off)
    assert ctx.render_lit_triangles_host(f, good).tobytes() == ref.tobytes()
    fresh = rto.Context(0)
    try:
        with pytest.raises(hip.RtoError) as e:
            fresh.render_lit_triangles_host(f, good)
        assert e.value.code == hip.RTO_E_NO_OCTREE
        import test_triangle_queries as ttq
        pn, ptris, poff = ttq._permuted(s.nodes, tris, off, np.random.default_rng(5))
        fresh.upload_octree(pn, s.min, s.voxel)
        fresh.upload_leaf_triangles(ptris, poff)
        assert fresh.info().canonical == 0
        with pytest.raises(hip.RtoError) as e:
            fresh.render_lit_triangles_host(f, good)
        assert e.value.code == hip.RTO_E_UNSUPPORTED
        assert len(fresh.query_triangle_pixels(f, np.zeros((1, 2), np.int32), tq.FIRST)) == 1       # the context is still usable
    finally:
        fresh.close()


@gpu
def test_drop_in_render_surface_lit(orc):
    """RayTracerBVH::renderSurfaceLit through host.py fills framebuffer() with the C ABI's lit triangle frame; without triangles
    resident it fails the way pickSurface does (no frame, lastError set)."""
    rto = _rto()
    W, H = 96, 72
    grid = rto.VoxelGrid.test_sphere(64)
    root = rto.createOctreeFromVoxelGrid(grid)
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    rt.setOctree(root, grid)
    cam = rto.Camera(*SPHERE_CAM)
    rt.renderSurfaceLit(cam, W, H, W / H, FOV, lightDir=(0.3, -0.8, 0.45), shadow=True, aoSamples=8, aoRadius=0.05, seed=4)
    assert rt.framebuffer() is None and "triangles" in rt.lastError
    rt.buildLeafTriangles()
    rt.renderSurfaceLit(cam, W, H, W / H, FOV, lightDir=(0.3, -0.8, 0.45), shadow=True, aoSamples=8, aoRadius=0.05, seed=4)
    img = rt.framebuffer()
    assert img is not None and img.shape == (H, W, 4)
    ctx = rto.Context(0)
    try:
        og = orc.test_sphere_grid(64)
        ctx.upload_octree(orc.build_flat_octree(og), og.min, og.voxel_size)
        ctx.build_leaf_triangles(og.data)
        f = rto.make_frame(cam.getView(), cam.getPos(), W / H, FOV, W, H)
        want = ctx.render_lit_triangles_host(f, _light((0.3, -0.8, 0.45), 1, 8, 0.05, 4))
    finally:
        ctx.close()
    assert img.tobytes() == want.tobytes() and (img[..., 0] > 0.05).any()
    rt.renderSurfaceLit(cam, W, H, W / H, FOV, shadow=False, aoSamples=0)
    lit0 = rt.framebuffer()
    rt.renderSceneTriangles(cam, W, H, W / H, FOV, False)
    assert lit0.tobytes() == rt.framebuffer().tobytes()
    rto.freeOctree(root)
