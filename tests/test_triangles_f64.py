"""Config 5 (leaf triangles + shadow ray) against a float64 reference of its rules (tests/ref64.py).

The bit-exact parity tests pin the kernels to the oracle, and the oracle to nothing upstream for this path: the two
were written together, in float32.  Here both are held to float64 on the pixels whose every decision lies beyond
float32's error (`robust`), with the share of the others bounded so the mask cannot hide a real fault.  The CPU tests
check the oracle; the GPU tests check the kernels directly, with no oracle involved."""
from __future__ import annotations

import numpy as np
import pytest

import ref64

LIT_TOL = 1e-5


# ---------------------------------------------------------------- scenes
def _grid(orc, data, gmin, voxel):
    dz, dy, dx = data.shape
    return orc.Grid((dx, dy, dz), np.asarray(gmin, np.float32), np.float32(voxel), np.ascontiguousarray(data, np.uint8))


def _ball(dim, centre, r, inner=None):
    z, y, x = np.meshgrid(*(np.arange(dim) + 0.5,) * 3, indexing="ij")
    d2 = (x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2
    m = d2 <= r * r
    if inner is not None:
        m &= d2 > inner * inner
    return m.astype(np.uint8)


def _cam(orc, theta, phi, r, target=None):
    c = orc.Camera(theta, phi, r)
    if target is not None:
        c.set_target(*[float(v) for v in target])
    return c.get_view(), c.get_pos()


def _sphere(orc, dim):
    return orc.test_sphere_grid(dim)


def _rescaled(orc, dim, gmin, voxel):
    """sphere `dim` moved to another origin and voxel size; camera at the grid's centre"""
    g = orc.test_sphere_grid(dim)
    g = _grid(orc, g.data, gmin, voxel)
    return g, np.asarray(gmin, np.float64) + 0.5 * dim * float(voxel)


# name -> (grid, (view, pos), W, H, fov, bound on the non-robust share, why)
def make_case(orc, name):
    if name in ("sphere16", "sphere32", "sphere64"):
        return _sphere(orc, int(name[6:])), _cam(orc, 0.5, 0.7, 1.8), 96, 96, 45.0, 0.02, "the shipped sphere camera"
    if name == "far200":
        return _sphere(orc, 64), _cam(orc, 0.5, 0.7, 200.0), 96, 96, 0.4, 0.08, "telephoto: hit point far from the eye"
    if name == "far5000":
        # float32's own uncertainty in ro - v0 (half an ulp of 5000) is ~1 % of a pixel here: many pixels sit on a
        # decision edge whatever the kernel does
        return _sphere(orc, 64), _cam(orc, 0.5, 0.7, 5000.0), 96, 96, 0.016, 0.30, "telephoto at 5000"
    if name == "shell_window":
        d = 48
        data = _ball(d, (24, 24, 24), 21, inner=17)
        data[:, :, 38:] = 0                                   # a window in the +x side: the inside and its shadows show
        return _grid(orc, data, (-0.5, -0.5, -0.5), 1.0 / d), _cam(orc, 0.25, 1.3, 1.7), 96, 96, 45.0, 0.02, "config 5's hollow shell, open"
    if name == "two_blobs":
        d = 40
        data = np.maximum(_ball(d, (12, 20, 20), 8), _ball(d, (28, 22, 19), 8))
        return _grid(orc, data, (-20, -20, -20), 1.0), _cam(orc, 0.15, -1.45, 90.0), 64, 64, 30.0, 0.02, "DFS-first-leaf vs nearest"
    if name == "box_axis":
        d = 24
        data = np.zeros((d, d, d), np.uint8)
        data[6:18, 6:18, 6:18] = 1
        return _grid(orc, data, (-12, -12, -12), 1.0), _cam(orc, 0.0, 0.0, 40.0), 80, 80, 45.0, 0.03, "planar faces seen along z"
    if name == "voxel_2^-12":
        g, c = _rescaled(orc, 32, (-0.5, -0.5, -0.5), 2.0 ** -12)
        return g, _cam(orc, 0.5, 0.7, 32 * 2.0 ** -12 * 1.8, c), 96, 96, 45.0, 0.02, "tiny voxels far from the origin"
    if name == "voxel_2^-8":
        g, c = _rescaled(orc, 32, (-0.5, -0.5, -0.5), 2.0 ** -8)
        return g, _cam(orc, 0.5, 0.7, 32 * 2.0 ** -8 * 1.8, c), 96, 96, 45.0, 0.02, "small voxels"
    if name == "voxel_10_calgary":
        g, c = _rescaled(orc, 32, (-2125.0, -1215.0, -150.0), 10.0)
        return g, _cam(orc, 0.5, 0.7, 320 * 1.8, c), 96, 96, 45.0, 0.02, "large voxels at the Calgary origin"
    if name == "eye_inside":
        d = 32
        data = _ball(d, (16, 16, 16), 14)
        return _grid(orc, data, (-0.5, -0.5, -0.5), 1.0 / d), _cam(orc, 0.3, 0.4, 0.11, (0.0, 0.0, 0.0)), 80, 80, 90.0, 0.02, \
            "eye in the solid: triangles behind it (t < 0) must not count"
    if name == "terraces":
        # steps falling away from the light (1, 1, 1): shadow rays skim concave creases, where the size of the offset
        # along the normal decides the verdict.  Axis-aligned faces put many shadow edges exactly on pixel decisions,
        # hence the wide bound
        d = 24
        z, y, x = np.meshgrid(np.arange(d), np.arange(d), np.arange(d), indexing="ij")
        data = (y < 4 + x // 3 + z // 5).astype(np.uint8)
        return _grid(orc, data, (-12, -12, -12), 1.0), _cam(orc, 0.6, -2.2, 30.0), 160, 160, 45.0, 0.25, "contact shadows in creases"
    if name.startswith("random"):
        from test_gpu_parity import _random_grid
        seed = int(name[6:])
        rng = np.random.default_rng(1000 + seed)
        g = _random_grid(orc, rng)
        ext = float(np.float32(max(g.dims)) * g.voxel_size)
        centre = g.min + 0.5 * np.array(g.dims, np.float32) * g.voxel_size
        radius = ext * rng.uniform(1.2, 4.0)
        return g, _cam(orc, float(rng.uniform(0, 6.28)), float(rng.uniform(-1.4, 1.4)), radius, centre), 80, 64, 45.0, 0.03, \
            "the fuzz test's grids"
    raise KeyError(name)


CPU_CASES = ["sphere16", "sphere32", "sphere64", "shell_window", "two_blobs", "box_axis", "voxel_2^-12", "voxel_2^-8",
             "voxel_10_calgary", "eye_inside", "terraces", "far200", "far5000"] + [f"random{i}" for i in range(4)]


class Case:
    def __init__(self, orc, name, spec=None, sample=None):
        g, (view, pos), W, H, fov, bound, why = spec or make_case(orc, name)
        self.name, self.grid, self.view, self.pos, self.W, self.H, self.fov, self.bound = name, g, view, pos, W, H, fov, bound
        self.nodes = orc.build_flat_octree(g)
        self.tris, self.off = orc.build_leaf_triangles(g, self.nodes)
        self.rd = orc.generate_rays(view, pos, W / H, fov, W, H).reshape(-1, 3)
        self.pix = np.arange(W * H) if sample is None else np.sort(np.random.default_rng(5).choice(W * H, sample, replace=False))
        self.rd = self.rd[self.pix]
        self.S = ref64.TriScene64(self.nodes, self.tris, self.off, g.min, g.voxel_size)
        self.ref = ref64.render64(self.S, pos, self.rd)
        o = np.broadcast_to(pos.astype(np.float64), self.rd.shape)
        self.bf_ray, self.bf_tri, self.bf_t, self.bf_sure = self.S.any_hits(np.ascontiguousarray(o), self.rd.astype(np.float64))


_cache = {}


def case(orc, name):
    if name not in _cache:
        _cache[name] = Case(orc, name)
    return _cache[name]


def check_frame(c: Case, frame, shadow, what, hits=None):
    """frame (H, W, 4) float32 from the renderer under test; hits: its per-frame hit count, when it gives one."""
    r = c.ref
    rgba = frame.reshape(-1, 4)[c.pix].astype(np.float64)
    got_hit = rgba[:, 0] > 0.05                               # miss (0,0,0,1); a hit is at least the ambient 0.1
    val = rgba[:, 0] - 0.1
    rob, hrob = r["robust"], r["hit_robust"]
    n = len(val)
    assert (~rob).sum() <= c.bound * n, f"{what}: {int((~rob).sum())} of {n} pixels non-robust (bound {c.bound:.0%})"
    # hit / miss
    bad = hrob & (got_hit != r["hit"])
    assert not bad.any(), f"{what}: {int(bad.sum())} robust pixels with another hit/miss than float64, e.g. {np.nonzero(bad)[0][:5]}"
    if hits is not None:
        assert abs(int(hits) - int(r["hit"].sum())) <= int((~hrob).sum()), f"{what}: hits {hits} vs float64 {int(r['hit'].sum())}"
    # the Lambert term, and with it the shadow verdict
    want = r["value"] if shadow else r["shade"]
    m = rob & r["hit"]
    err = np.abs(val - want)
    bad = m & (err > LIT_TOL)
    assert not bad.any(), (f"{what}: {int(bad.sum())} robust hit pixels off float64's n.l "
                           f"(max {err[bad].max():.3g}), e.g. {np.nonzero(bad)[0][:5]}")
    if shadow:
        lit = m & (r["shade"] > LIT_TOL)
        bad = lit & ((val < LIT_TOL) != r["shadowed"])
        assert not bad.any(), (f"{what}: {int(bad.sum())} robust pixels with another shadow verdict than float64 "
                               f"({int((bad & r['shadowed']).sum())} lit where float64 is shadowed)")
    # order-independent: a ray that surely hits some triangle is a hit ...
    bad = c.bf_sure & ~got_hit
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels miss although float64 hits a triangle beyond doubt (leak)"
    # ... and a hit's shade is that of a triangle the ray really hits
    L = ref64.LIGHT
    n_ = c.S.nrm[c.bf_tri]
    n_ = np.where((ref64._dot(n_, c.rd[c.bf_ray].astype(np.float64)) > 0)[:, None], -n_, n_)
    cand = np.maximum(0.0, ref64._dot(n_, L))
    ok = np.zeros(n, bool)
    close = np.abs(cand - val[c.bf_ray]) <= LIT_TOL
    ok[c.bf_ray[close]] = True
    need = got_hit & (val > LIT_TOL) & hrob
    bad = need & ~ok
    assert not bad.any(), f"{what}: {int(bad.sum())} hit pixels shaded like no triangle their ray hits, e.g. {np.nonzero(bad)[0][:5]}"


def _oracle(orc, c: Case, shadow):
    return orc.render_triangles(c.nodes, c.tris, c.off, c.grid.min, c.grid.voxel_size, c.view, c.pos, c.W / c.H, c.fov, c.W, c.H,
                                shadow=shadow)


# ---------------------------------------------------------------- CPU: the oracle against float64
@pytest.mark.parametrize("name", CPU_CASES)
def test_oracle_equals_float64(orc, name):
    c = case(orc, name)
    assert c.ref["hit"].sum() > 0, f"{name}: the scene must be seen"
    for shadow in (False, True):
        frame, st = _oracle(orc, c, shadow)
        check_frame(c, frame, shadow, f"oracle {name} shadow={shadow}", hits=st["hits"])


def test_far_camera_shadows_are_lit_where_float64_is(orc):
    """Shadow acne grew with the camera's distance (the origin p + n bias had the rounding error of ro + rd t, which
    grows with t): a sphere seen from r = 200 and 5000 must shadow the same pixels as from nearby."""
    for name in ("far200", "far5000"):
        c = case(orc, name)
        frame, _ = _oracle(orc, c, True)
        val = frame.reshape(-1, 4)[:, 0].astype(np.float64) - 0.1
        lit64 = c.ref["robust"] & c.ref["hit"] & (c.ref["shade"] > LIT_TOL) & ~c.ref["shadowed"]
        assert lit64.sum() > 150
        dark = lit64 & (val < LIT_TOL)
        assert not dark.any(), f"{name}: {int(dark.sum())} of {int(lit64.sum())} lit pixels shadowed"


def test_two_blobs_pin_the_first_leaf_rule(orc):
    """The primary hit is the first leaf in pop order (children 7..0) with any triangle hit, not the nearest surface:
    on two blobs that overlap on screen some pixels show the farther blob, and the oracle follows that rule."""
    c = case(orc, "two_blobs")
    r = c.ref
    near_t = np.full(len(c.rd), np.inf)
    np.minimum.at(near_t, c.bf_ray, c.bf_t)
    farther = r["robust"] & r["hit"] & (r["t"] > near_t + 1.0)           # a voxel or more behind the nearest surface
    assert int(farther.sum()) == 396, int(farther.sum())    # of ~530 hits: the blob on the +x side is popped first
    frame, _ = _oracle(orc, c, False)
    val = frame.reshape(-1, 4)[:, 0].astype(np.float64) - 0.1
    np.testing.assert_allclose(val[farther], r["shade"][farther], atol=LIT_TOL)


def test_triangles_lie_inside_their_leaves(orc):
    """any_hits prunes by leaf boxes: sound only if every triangle lies in its own leaf's closed box (up to the
    rounding of the vertices' own coordinates, which _inside's margin covers)."""
    for name in ("sphere32", "shell_window", "voxel_10_calgary", "random1"):
        c = case(orc, name)
        owner = np.repeat(np.arange(len(c.nodes)), np.diff(c.off))
        v = c.tris[:, :9].reshape(-1, 3, 3).astype(np.float64)
        lo, hi = c.S.bmin[owner][:, None, :], c.S.bmax[owner][:, None, :]
        tol = 4 * ref64.EPS * c.S.bmag[owner][:, None, None]
        assert ((v >= lo - tol) & (v <= hi + tol)).all(), name


# ---------------------------------------------------------------- GPU: the kernels against float64, no oracle involved
GPU_CASES = CPU_CASES
TRI_KERNELS = (("lean", "KERNEL_AUTO"), ("packed_v3", "KERNEL_PACKED_V3"), ("generic", "KERNEL_GENERIC"))


def _upload(ctx, c):
    import ray_tracing_octrees_amd as rto
    ctx.set_kernel(rto.KERNEL_AUTO)
    ctx.upload_octree(c.nodes, c.grid.min, c.grid.voxel_size)
    ctx.upload_leaf_triangles(c.tris, c.off)
    return rto.make_frame(c.view, c.pos, c.W / c.H, c.fov, c.W, c.H)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_CASES)
def test_kernels_equal_float64(ctx, orc, name):
    """Every triangle kernel, shadow on and off, both forms of the exact-grid child test, and the batched kernel."""
    import ray_tracing_octrees_amd as rto
    from ray_tracing_octrees_amd import hip
    torch = pytest.importorskip("torch")
    c = case(orc, name)
    f = _upload(ctx, c)
    try:
        for kname, kattr in TRI_KERNELS:
            ctx.set_kernel(getattr(rto, kattr))
            for shadow in (False, True):
                got, gs = ctx.render_triangles_host(f, shadow=shadow, stats=True)
                check_frame(c, got, shadow, f"{name} {kname} shadow={shadow}", hits=gs["hits"])
                check_frame(c, ctx.render_triangles_host(f, shadow=shadow), shadow, f"{name} {kname} shadow={shadow} (colour only)")
        ctx.set_kernel(rto.KERNEL_AUTO)
        if ctx.debug_set_exact_grid(True)[1]:                  # an exact grid: the general child test must agree as well
            ctx.debug_set_exact_grid(False)
            try:
                for shadow in (False, True):
                    check_frame(c, ctx.render_triangles_host(f, shadow=shadow), shadow, f"{name} lean, general child test, shadow={shadow}")
            finally:
                ctx.debug_set_exact_grid(True)
        arr = hip.Context.frame_array([f, f, f])
        out = torch.full((3, c.H, c.W, 4), 7.0, dtype=torch.float32, device="cuda")
        for shadow in (False, True):
            ctx.render_triangles_batch_device(arr, out.data_ptr(), out.stride(0) * 4, shadow, None, False, 0)
            torch.cuda.synchronize()
            for i in range(3):
                check_frame(c, out[i].cpu().numpy(), shadow, f"{name} batched frame {i} shadow={shadow}")
    finally:
        ctx.set_kernel(rto.KERNEL_AUTO)


@pytest.mark.gpu
def test_config5_sized_frame_equals_float64_on_a_sample(ctx, orc):
    """Config 5's size: the 512^3 shell, 3840x2160, the default camera; float64 on a fixed sample of 2^16 pixels."""
    import ray_tracing_octrees_amd as rto
    spec = (orc.test_sphere_grid(512), _cam(orc, 0.5, 0.7, 1.8), 3840, 2160, 45.0, 0.02, "config 5")
    c = Case(orc, "config5", spec=spec, sample=1 << 16)
    f = _upload(ctx, c)
    for kname, kattr in TRI_KERNELS:
        ctx.set_kernel(getattr(rto, kattr))
        check_frame(c, ctx.render_triangles_host(f, shadow=True), True, f"config 5 4K {kname}")
    ctx.set_kernel(rto.KERNEL_AUTO)
