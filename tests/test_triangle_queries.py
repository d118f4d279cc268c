"""Triangle queries (rto_query_triangles_*, rto_query_triangle_pixels_*, Context.query_triangle*, RayTracerBVH::intersectTriangles /
pickSurface): caller rays and pixel picks against the resident leaf triangles.  CPU: the float32 statement (tests/tri_query_ref.py)
against the oracle's triangle frames and float64 (tests/ref64.py); the ABI's layout and exports; the built assembly of the k_triq_*
kernels.  GPU: every mode against the statement and the renders, bit for bit, on both kernels."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import deep_scenes as ds
import query_ref as q
import ref64
import tri_query_ref as tq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (tq.FIRST, tq.CLOSEST, tq.ANY)
DESC_VGPR_BUDGET = 80       # 6 waves per SIMD (512 / 80), what the LDS stack allows up to depth 8
NODES_VGPR_BUDGET = 64      # one wave per workgroup, 36 KB of LDS: 4 workgroups per CU; registers are not what limits it
SYMS = ("rto_query_triangles_device", "rto_query_triangles_host", "rto_query_triangle_pixels_device", "rto_query_triangle_pixels_host")


def _recs_equal(got, want, what, mask_only=False):
    """Records equal in every field, bitwise; mask_only: the hit / miss mask alone (ANY's triangle is unspecified)."""
    gh, wh = got["tri"] >= 0, want["tri"] >= 0
    bad = np.nonzero(gh != wh)[0]
    assert not len(bad), f"{what}: {len(bad)} rays differ in hit / miss, e.g. {bad[:5]}: got {got[bad[:3]]} want {want[bad[:3]]}"
    if mask_only:
        return
    neq = (got.view(np.int32).reshape(-1, 8) != want.view(np.int32).reshape(-1, 8)).any(1)
    bad = np.nonzero(neq)[0]
    assert not len(bad), f"{what}: {len(bad)} records differ, e.g. rays {bad[:5]}: got {got[bad[:3]]} want {want[bad[:3]]}"


def _any_is_accepted(got, o, d, tmn, tmx, tris, off, what):
    """ANY's record: a triangle of the leaf it names, hit by the ray inside the window, with the fields Moeller-Trumbore gives."""
    h = np.nonzero(got["tri"] >= 0)[0]
    k, leaf = got["tri"][h], got["node"][h]
    assert ((off[leaf] <= k) & (k < off[leaf + 1])).all(), what
    ok, t, u, v = tq.ray_triangle(np.broadcast_to(o, d.shape)[h], d[h], tris[k])
    assert ok.all(), what
    assert (t.view(np.int32) == got["t"][h].view(np.int32)).all() and (u == got["u"][h]).all() and (v == got["v"][h]).all(), what
    assert ((got["t"][h] >= tmn[h]) & (got["t"][h] <= tmx[h])).all(), what


def _scene(orc, name):
    import test_triangles_f64 as tf
    g, (view, pos), W, H, fov, bound, _ = tf.make_case(orc, name)
    nodes = orc.build_flat_octree(g)
    tris, off = orc.build_leaf_triangles(g, nodes)
    return g, nodes, tris, off, view, pos, W, H, fov, bound


# ================================================================ CPU
@pytest.mark.parametrize("name", ["sphere32", "two_blobs", "shell_window", "eye_inside", "far200", "terraces"])
def test_statement_first_gives_the_oracle_frames(orc, name):
    """FIRST on every pixel ray with (0, 1e30), shaded, is orc_render_triangles' frame bit for bit with shadows off; with shadows on,
    FIRST on the shadow rays derived from the records decides the shadowed pixels, again bit for bit."""
    g, nodes, tris, off, view, pos, W, H, fov, _ = _scene(orc, name)
    T = q.Tree32(nodes, g.min, g.voxel_size)
    rd = orc.generate_rays(view, pos, W / H, fov, W, H).reshape(-1, 3)
    first = tq.query_tri32(T, tris, off, pos, rd)[tq.FIRST]
    assert (first["tri"] >= 0).sum() > 50
    plain, _ = orc.render_triangles(nodes, tris, off, g.min, g.voxel_size, view, pos, W / H, fov, W, H, shadow=False)
    got = tq.shade(first)
    assert got.tobytes() == plain.reshape(-1, 4).tobytes(), f"{int((got != plain.reshape(-1, 4)).any(1).sum())} pixels"
    so, sd = tq.shadow_rays(pos, rd, first, tris, g.voxel_size)
    h = first["tri"] >= 0
    sh = tq.query_tri32(T, tris, off, so[h], sd[h])[tq.FIRST]
    shadowed = np.zeros(len(rd), bool)
    shadowed[np.nonzero(h)[0]] = sh["tri"] >= 0
    dark, _ = orc.render_triangles(nodes, tris, off, g.min, g.voxel_size, view, pos, W / H, fov, W, H, shadow=True)
    got = tq.shade(first, shadowed)
    assert got.tobytes() == dark.reshape(-1, 4).tobytes(), f"{int((got != dark.reshape(-1, 4)).any(1).sum())} pixels"


@pytest.mark.parametrize("name", ["sphere32", "two_blobs", "shell_window", "eye_inside", "voxel_10_calgary"])
def test_statement_against_float64(orc, name):
    """FIRST against TriScene64.trace_dfs and CLOSEST / ANY against any_hits: robust rays agree in hit and triangle, every CLOSEST
    hit is a pair float64 may call a hit, every sure hit is a hit; the non-robust share stays within the scene's bound."""
    g, nodes, tris, off, view, pos, W, H, fov, bound = _scene(orc, name)
    T = q.Tree32(nodes, g.min, g.voxel_size)
    S = ref64.TriScene64(nodes, tris, off, g.min, g.voxel_size)
    rd = orc.generate_rays(view, pos, W / H, fov, W, H).reshape(-1, 3)
    # pixel rays and rays from random points around the scene to random points inside it
    rng = np.random.default_rng(7)
    lo, hi = T.bmin[0].astype(np.float64), T.bmax[0].astype(np.float64)
    o2 = (lo + (hi - lo) * rng.uniform(-0.5, 1.5, (2048, 3))).astype(np.float32)
    d2 = ((lo + (hi - lo) * rng.random((2048, 3))) - o2).astype(np.float32)
    o = np.concatenate([np.broadcast_to(pos, rd.shape).astype(np.float32), o2])
    d = np.concatenate([rd, d2])
    r = tq.query_tri32(T, tris, off, o, d)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    ref = S.trace_dfs(o64, d64)
    rob = ref["robust"]
    assert (~rob).mean() <= bound, (~rob).mean()
    f = r[tq.FIRST]
    assert ((f["tri"] >= 0) == ref["hit"])[ref["hit_robust"]].all()
    assert (f["tri"] == ref["tri"])[rob].all()
    pr, pk, _, sure = S.any_hits(o64, d64)
    c = r[tq.CLOSEST]
    assert (c["tri"] >= 0)[sure].all(), "a sure hit is a miss"
    pairs = set(zip(pr.tolist(), pk.tolist()))
    h = np.nonzero(c["tri"] >= 0)[0]
    assert all((int(i), int(c["tri"][i])) in pairs for i in h), "CLOSEST returned a triangle float64 does not hit"
    hitters = np.zeros(len(d), bool); hitters[pr] = True
    assert not ((c["tri"] >= 0) & ~hitters).any()
    assert ((~sure) & hitters).mean() <= bound
    # CLOSEST is never behind FIRST, and the least t any hit pair has (within float32's error of t)
    both = (f["tri"] >= 0)
    assert (c["t"][both] <= f["t"][both]).all()


def test_statement_windows_and_invalid_rays(orc):
    """Windows decide which triangles count: a t_max short of the nearest surface gives a miss, a t_min past it moves CLOSEST to a
    farther surface, the window [t, t] keeps it; NaN inputs and t_min > t_max miss in every mode."""
    g, nodes, tris, off, view, pos, W, H, fov, _ = _scene(orc, "shell_window")
    T = q.Tree32(nodes, g.min, g.voxel_size)
    rd = orc.generate_rays(view, pos, W / H, fov, W, H).reshape(-1, 3)
    base = tq.query_tri32(T, tris, off, pos, rd)[tq.CLOSEST]
    h = base["tri"] >= 0
    short = tq.query_tri32(T, tris, off, pos, rd, 0.0, base["t"] * np.float32(0.999))[tq.CLOSEST]
    assert (short["tri"] < 0)[h].all()
    past = tq.query_tri32(T, tris, off, pos, rd, base["t"] * np.float32(1.0001), 1e30)[tq.CLOSEST]
    assert ((past["t"] > base["t"]) | (past["tri"] < 0))[h].all() and (past["tri"] >= 0)[h].mean() > 0.5
    exact = tq.query_tri32(T, tris, off, pos, rd, base["t"], base["t"])[tq.CLOSEST]
    assert (exact["tri"] == base["tri"])[h].all()
    o = np.broadcast_to(pos, (6, 3)).astype(np.float32).copy()
    d = rd[:6].copy()
    tmn = np.zeros(6, np.float32); tmx = np.full(6, 1e30, np.float32)
    o[0, 0] = np.nan; d[1, 2] = np.nan; tmn[2] = np.nan; tmx[3] = np.nan; tmn[4], tmx[4] = 2.0, 1.0
    r = tq.query_tri32(T, tris, off, o, d, tmn, tmx)
    for m in MODES:
        assert (r[m]["tri"][:5] == -1).all() and (r[m]["t"][:5] == tq.MISS_T).all()


def test_tri_hit_layout_and_exports():
    """rto_tri_hit is 32 bytes in the header's field order; TRI_HIT_DTYPE and hip.TriHit match it; the four entry points are declared,
    listed in SYMBOLS and exported by the built library."""
    from ray_tracing_octrees_amd import hip
    assert hip.TRI_HIT_DTYPE.itemsize == 32 and C.sizeof(hip.TriHit) == 32
    assert hip.TRI_HIT_DTYPE == tq.TRI_HIT_DTYPE
    assert [f[0] for f in hip.TriHit._fields_] == list(hip.TRI_HIT_DTYPE.names)
    hdr = open(os.path.join(ROOT, "include", "rto_hip.h")).read()
    m = re.search(r"typedef struct rto_tri_hit \{(.*?)\} rto_tri_hit;", hdr, re.S)
    assert m, "rto_tri_hit is not declared"
    fields = re.findall(r"^\s*(float|int32_t)\s+([^;]+);", m.group(1), re.M)
    names = [n.strip() for _, decl in fields for n in decl.split(",")]
    assert names == ["t", "tri", "node", "u", "v", "nx", "ny", "nz"], names
    lib = C.CDLL(os.path.join(ROOT, "ray_tracing_octrees_amd", "librto_hip.so"))
    for s in SYMS:
        assert re.search(rf"\bint\s+{s}\(", hdr), s
        assert s in hip.SYMBOLS, s
        assert hasattr(lib, s), s


def test_triangle_query_kernels_keep_their_budgets():
    """The built assembly (the product's flags): the 12 k_triq_* kernels without scratch instructions, spills or v_mfma; the
    descriptor kernels within DESIGN.md section 10's VGPR budget."""
    import test_isa_contract as isa
    asm = isa.built_asm()
    if asm is None:
        pytest.fail("no hipcc: the budget cannot be checked")
    meta = isa.kernel_meta(asm)
    names = [k for k in meta if "k_triq_" in k]
    assert len(names) == 12, names                                    # {desc, nodes} x {FIRST, CLOSEST, ANY} x {rays, pixels}
    assert len([k for k in meta if "k_query_" in k]) == 12            # the box queries' kernels untouched
    for k in names:
        m = meta[k]
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (k, m)
        assert m["vgpr"] <= (DESC_VGPR_BUDGET if "k_triq_desc" in k else NODES_VGPR_BUDGET), (k, m)
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


def _upload(ctx, nodes, gmin, voxel, tris, off, kernel=None):
    rto = _rto()
    ctx.set_kernel(rto.KERNEL_AUTO if kernel is None else kernel)
    ctx.upload_octree(nodes, gmin, voxel)
    ctx.upload_leaf_triangles(tris, off)


def _check_frame_by_queries(ctx, f, pos, rd, xy, tris, voxel, what, want_first=None):
    """The render's frames (shadow off / on) from FIRST pixel records and FIRST on the derived shadow rays; returns the records."""
    first = ctx.query_triangle_pixels(f, xy, tq.FIRST)
    if want_first is not None:
        _recs_equal(first, want_first, f"{what}: FIRST pixel records vs the statement")
    plain = ctx.render_triangles_host(f, shadow=False).reshape(-1, 4)[xy[:, 1] * f.width + xy[:, 0]]
    got = tq.shade(first)
    bad = (got != plain).any(1)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels shade differently from the frame (shadow off)"
    h = first["tri"] >= 0
    assert h.sum() > 0, what
    so, sd = tq.shadow_rays(pos, rd, first, tris, voxel)
    sh = ctx.query_triangles(so[h], sd[h], 0.0, 1e30, tq.FIRST)
    shadowed = np.zeros(len(xy), bool)
    shadowed[np.nonzero(h)[0]] = sh["tri"] >= 0
    dark = ctx.render_triangles_host(f, shadow=True).reshape(-1, 4)[xy[:, 1] * f.width + xy[:, 0]]
    got = tq.shade(first, shadowed)
    bad = (got != dark).any(1)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ from the shadowed frame"
    return first


@gpu
@pytest.mark.parametrize("name", ["sphere64", "two_blobs", "shell_window", "eye_inside", "far200", "terraces"])
def test_pixel_queries_reproduce_the_triangle_render(ctx, orc, name):
    """FIRST on every pixel is rto_render_triangles' hit: shaded, the frame bit for bit (shadow off); with FIRST on the shadow rays,
    the shadowed frame bit for bit.  Both kernels, against the float32 statement in every field; query_triangles on the oracle's
    pixel rays gives the same records; ANY's mask is CLOSEST's."""
    rto = _rto()
    g, nodes, tris, off, view, pos, W, H, fov, _ = _scene(orc, name)
    T = q.Tree32(nodes, g.min, g.voxel_size)
    rd = orc.generate_rays(view, pos, W / H, fov, W, H).reshape(-1, 3)
    want = tq.query_tri32(T, tris, off, pos, rd)
    xy = _all_pixels(W, H)
    f = rto.make_frame(view, pos, W / H, fov, W, H)
    for kernel in (rto.KERNEL_AUTO, rto.KERNEL_GENERIC):
        _upload(ctx, nodes, g.min, g.voxel_size, tris, off, kernel)
        what = f"{name} kernel {kernel}"
        _check_frame_by_queries(ctx, f, pos, rd, xy, tris, g.voxel_size, what, want[tq.FIRST])
        for m in MODES:
            got = ctx.query_triangle_pixels(f, xy, m)
            _recs_equal(got, want[m], f"{what} mode {m}", mask_only=(m == tq.ANY))
            byrays = ctx.query_triangles(np.broadcast_to(pos, rd.shape), rd, 0.0, 1e30, m)
            _recs_equal(byrays, got, f"{what} mode {m}: rays vs pixels", mask_only=(m == tq.ANY))
    ctx.set_kernel(rto.KERNEL_AUTO)


@gpu
def test_config5_sized_pixel_queries_reproduce_the_render(ctx, orc):
    """Config 5's size: the 512^3 shell at 3840x2160, the default camera, on a seeded sample of 2^20 pixels: the frame (shadow off
    and on) from FIRST records, on the descriptor kernel."""
    rto = _rto()
    g = orc.test_sphere_grid(512)
    nodes = orc.build_flat_octree(g)
    cam = orc.Camera(0.5, 0.7, 1.8)
    view, pos = cam.get_view(), cam.get_pos()
    W, H = 3840, 2160
    ctx.set_kernel(rto.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    ctx.build_leaf_triangles()
    tris, _ = ctx.download_leaf_triangles()
    pix = np.sort(np.random.default_rng(55).choice(W * H, 1 << 20, replace=False))
    xy = np.stack([pix % W, pix // W], 1).astype(np.int32)
    rd = orc.generate_rays(view, pos, W / H, 45.0, W, H).reshape(-1, 3)[pix]
    f = rto.make_frame(view, pos, W / H, 45.0, W, H)
    first = _check_frame_by_queries(ctx, f, pos, rd, xy, tris, g.voxel_size, "config 5 4K")
    assert (first["tri"] >= 0).mean() > 0.1


def _seeded(T, tris, off, n, seed):
    """query_ref's seeded rays (outside, inside, inside solid leaves, axis-aligned, zero components, grazing, NaN, t_min > t_max) with
    windows placed around the nearest triangle: t_max short of it, t_min past it, a window around it."""
    o, d, tmn, tmx = q.seeded_rays(T, n, seed, windows_too=False)
    rng = np.random.default_rng(seed + 100)
    base = tq.query_tri32(T, tris, off, o, d)[tq.CLOSEST]
    ht = np.where(base["tri"] >= 0, base["t"], np.float32(1.0)).astype(np.float32)
    w = rng.integers(0, 4, n)
    w[n - 8:] = 0                                                      # leave the invalid rays at the end as they are
    tmx = np.where(w == 1, ht * rng.uniform(0.3, 0.999, n).astype(np.float32), tmx).astype(np.float32)
    tmn = np.where(w == 2, ht * rng.uniform(1.0001, 1.5, n).astype(np.float32), tmn).astype(np.float32)
    tmn = np.where(w == 3, ht * np.float32(0.9), tmn).astype(np.float32)
    tmx = np.where(w == 3, ht * np.float32(1.2), tmx).astype(np.float32)
    tmn[(rng.random(n) < 0.03) & (w == 0)] = np.float32(-1.0)
    return o, d, tmn, tmx


def _permuted(nodes, tris, off, rng):
    """The same tree under another numbering (root kept at 0), its triangles regrouped to follow the new numbering."""
    n = len(nodes)
    perm = np.concatenate([[0], 1 + rng.permutation(n - 1)])          # new index of old node i = perm[i]
    out = np.zeros_like(nodes)
    out[perm] = nodes
    ch = out["child"]
    out["child"] = np.where(ch >= 0, perm[np.maximum(ch, 0)], -1)
    old = np.argsort(perm)                                             # old index of new node j
    cnt = np.diff(off)[old]
    noff = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    ntris = np.concatenate([tris[off[i]:off[i + 1]] for i in old] + [np.zeros((0, 12), np.float32)])
    return out, ntris, noff


@gpu
@pytest.mark.parametrize("name,seed", [("sphere32", 11), ("two_blobs", 12), ("shell_window", 13), ("voxel_10_calgary", 14)])
def test_seeded_rays_match_the_statement_on_every_array(ctx, orc, name, seed):
    """Seeded rays with windows, NaN inputs, zero direction components and origins inside the solid, every mode, bit for bit the
    statement's records: the descriptor kernel on the canonical array, the node-by-node kernel under RTO_KERNEL_GENERIC and on a
    permuted (non-canonical) array, and the descriptor kernel on the octree and triangles the GPU builds."""
    rto = _rto()
    g, nodes, tris, off, *_ = _scene(orc, name)
    T = q.Tree32(nodes, g.min, g.voxel_size)
    o, d, tmn, tmx = _seeded(T, tris, off, 4096, seed)
    want = tq.query_tri32(T, tris, off, o, d, tmn, tmx)
    assert (want[tq.CLOSEST]["tri"] >= 0).mean() > 0.1

    def check(what, tr, of, remap=None):
        for m in MODES:
            got = ctx.query_triangles(o, d, tmn, tmx, m)
            w = want[m] if remap is None else remap(want[m])
            _recs_equal(got, w, f"{name} {what} mode {m}", mask_only=(m == tq.ANY))
            if m == tq.ANY:
                _any_is_accepted(got, o, d, tmn, tmx, tr, of, f"{name} {what} ANY")

    for kernel in (rto.KERNEL_AUTO, rto.KERNEL_GENERIC):
        _upload(ctx, nodes, g.min, g.voxel_size, tris, off, kernel)
        assert ctx.info().canonical == 1
        check(f"kernel {kernel}", tris, off)
    pn, ptris, poff = _permuted(nodes, tris, off, np.random.default_rng(seed))
    _upload(ctx, pn, g.min, g.voxel_size, ptris, poff)
    assert ctx.info().canonical == 0
    Tp = q.Tree32(pn, g.min, g.voxel_size)
    wp = tq.query_tri32(Tp, ptris, poff, o, d, tmn, tmx)
    for m in MODES:
        got = ctx.query_triangles(o, d, tmn, tmx, m)
        _recs_equal(got, wp[m], f"{name} permuted mode {m}", mask_only=(m == tq.ANY))
        # FIRST picks the same triangle under any numbering (CLOSEST's ties between leaves go to the lowest index, which moves)
        h = got["tri"] >= 0
        if m == tq.FIRST:
            assert (ptris[got["tri"][h]] == tris[want[m]["tri"][h]]).all()
    ctx.set_kernel(rto.KERNEL_AUTO)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    ctx.build_leaf_triangles()
    bn = ctx.download_nodes()
    btris, boff = ctx.download_leaf_triangles()
    Tb = q.Tree32(bn, g.min, g.voxel_size)
    wb = tq.query_tri32(Tb, btris, boff, o, d, tmn, tmx)
    for m in MODES:
        got = ctx.query_triangles(o, d, tmn, tmx, m)
        _recs_equal(got, wb[m], f"{name} GPU-built mode {m}", mask_only=(m == tq.ANY))


def _grazing(T, tris, off, n, seed):
    """Rays aimed at triangle vertices, and at midpoints of triangle edges, that lie on a face the owning leaf shares with a
    neighbour (an interior face plane of its box), from directions spread over the sphere and nearly inside that plane."""
    rng = np.random.default_rng(seed)
    owner = np.repeat(np.arange(len(off) - 1), np.diff(off))
    v = tris[:, :9].reshape(-1, 3, 3)
    lo, hi = T.bmin[owner][:, None, :], T.bmax[owner][:, None, :]
    inner = ((v == lo) & (lo > T.bmin[0])) | ((v == hi) & (hi < T.bmax[0]))          # (tri, vertex, axis)
    pts, axes = [], []
    for a in range(3):
        tv = np.nonzero(inner[:, :, a])
        pts.append(v[tv[0], tv[1]]); axes.append(np.full(len(tv[0]), a))
        for i, j in ((0, 1), (1, 2), (2, 0)):
            e = np.nonzero(inner[:, i, a] & inner[:, j, a] & (v[:, i, a] == v[:, j, a]))[0]
            pts.append(0.5 * (v[e, i].astype(np.float64) + v[e, j])); axes.append(np.full(len(e), a))
    pts, axes = np.concatenate(pts), np.concatenate(axes)
    assert len(pts) > 10, "the scene has no triangle vertices on shared leaf faces"
    k = rng.integers(0, len(pts), n)
    p, ax = pts[k].astype(np.float64), axes[k]
    dd = rng.normal(size=(n, 3))
    flat = rng.random(n) < 0.5
    dd[np.nonzero(flat)[0], ax[flat]] = rng.choice([0.0, 1e-6, -1e-6], int(flat.sum()))
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    ext = float(T.bmax[0].max() - T.bmin[0].min())
    o = (p - dd * ext * rng.uniform(0.05, 1.0, (n, 1))).astype(np.float32)
    return o, dd.astype(np.float32)


@gpu
@pytest.mark.parametrize("name", ["box_axis", "sphere32", "two_blobs"])
def test_grazing_rays_on_shared_leaf_faces(ctx, orc, name):
    """Rays at vertices and edges lying on faces two leaves share -- where a triangle's float t can come out in front of its own
    leaf's float tNear -- every mode, both kernels, bit for bit the statement (CLOSEST's exhaustive rule)."""
    rto = _rto()
    g, nodes, tris, off, *_ = _scene(orc, name)
    T = q.Tree32(nodes, g.min, g.voxel_size)
    o, d = _grazing(T, tris, off, 4096, 3)
    want = tq.query_tri32(T, tris, off, o, d)
    assert (want[tq.CLOSEST]["tri"] >= 0).mean() > 0.5
    for kernel in (rto.KERNEL_AUTO, rto.KERNEL_GENERIC):
        _upload(ctx, nodes, g.min, g.voxel_size, tris, off, kernel)
        for m in MODES:
            got = ctx.query_triangles(o, d, 0.0, 1e30, m)
            _recs_equal(got, want[m], f"{name} kernel {kernel} mode {m}", mask_only=(m == tq.ANY))
    ctx.set_kernel(rto.KERNEL_AUTO)


def _spine_triangles(s):
    """A few triangles per solid leaf of a spine scene, inside its box: two on the -x face, one across the box's diagonal."""
    g0, vs = s.min.astype(np.float32), np.float32(s.voxel)
    sol = np.nonzero((s.nodes["isSolid"] == 1) & ((s.nodes["isLeaf"] == 1) | (s.nodes["isUniform"] == 1)))[0]
    xyz = np.stack([s.nodes["x"], s.nodes["y"], s.nodes["z"]], 1)[sol].astype(np.float32)
    lo = (g0 + xyz * vs).astype(np.float32)
    hi = (lo + (s.nodes["size"][sol].astype(np.float32) * vs)[:, None]).astype(np.float32)
    c = lambda a, b, cc: np.stack([a[:, 0], b[:, 1], cc[:, 2]], 1)         # noqa: E731
    quads = [(lo, c(lo, hi, lo), c(lo, lo, hi)), (c(lo, hi, hi), c(lo, lo, hi), c(lo, hi, lo)), (c(lo, lo, lo), c(hi, hi, lo), hi)]
    t = np.zeros((len(sol), 3, 12), np.float32)
    for i, (a, b, cc) in enumerate(quads):
        e1, e2 = (b - a).astype(np.float64), (cc - a).astype(np.float64)
        nrm = np.cross(e1, e2)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        t[:, i] = np.concatenate([a, b, cc, nrm.astype(np.float32)], 1)
    cnt = np.zeros(len(s.nodes), np.int64)
    cnt[sol] = 3
    return t.reshape(-1, 12), np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)


@gpu
@pytest.mark.parametrize("kind,d,geometry", [("frac", 11, "thin"), ("tenth", 16, "thin"), ("far", 12, "spine"),
                                             ("frac", 19, "spine"), ("tenth", 20, "spine")])
def test_deep_octrees_against_float64(ctx, orc, kind, d, geometry):
    """Depth 11-20 trees: "thin" scenes with rto_build_leaf_triangles, "spine" scenes (2^20 voxels a side at depth 20, 134- and
    141-entry walks) with a few uploaded triangles per solid leaf.  Pixel rays of the scene's cameras and seeded rays: FIRST agrees
    with TriScene64.trace_dfs on robust rays, both kernels agree with each other and with the statement bit for bit."""
    rto = _rto()
    s = ds.scene(kind, d, geometry)
    ctx.set_kernel(rto.KERNEL_AUTO)
    ctx.upload_octree(s.nodes, s.min, s.voxel)
    if geometry == "thin":
        ctx.build_leaf_triangles(s.data)
        tris, off = ctx.download_leaf_triangles()
    else:
        tris, off = _spine_triangles(s)
        ctx.upload_leaf_triangles(tris, off)
    assert len(tris) > 0
    T = q.Tree32(s.nodes, s.min, s.voxel)
    W, H = 48, 40
    rays = []
    for _, view, pos in s.cameras(orc):
        rd = orc.generate_rays(view, pos, W / H, 45.0, W, H).reshape(-1, 3)
        rays.append((np.broadcast_to(pos, rd.shape).astype(np.float32), rd))
    so, sd, _, _ = q.seeded_rays(T, 1024, d, windows_too=False)
    rays.append((so, sd))
    o, dd = (np.concatenate(x) for x in zip(*rays))
    want = tq.query_tri32(T, tris, off, o, dd)
    S = ref64.TriScene64(s.nodes, tris, off, s.min, s.voxel)
    # float64 on rays without NaN and without a zero direction component: for an origin on a box plane, the float32 slab test's
    # 0 * inf = NaN has no float64 counterpart (those rays are held to the statement above all the same)
    ok = ~np.isnan(o).any(1) & ~np.isnan(dd).any(1) & (dd != 0).all(1)
    ref = S.trace_dfs(o[ok].astype(np.float64), dd[ok].astype(np.float64))
    res = {}
    for kernel in (rto.KERNEL_AUTO, rto.KERNEL_GENERIC):
        ctx.set_kernel(kernel)
        for m in MODES:
            res[kernel, m] = got = ctx.query_triangles(o, dd, 0.0, 1e30, m)
            _recs_equal(got, want[m], f"{kind}{d} {geometry} kernel {kernel} mode {m}", mask_only=(m == tq.ANY))
        g = res[kernel, tq.FIRST][ok]
        rob = ref["robust"]
        assert (~rob).mean() <= 0.6, (~rob).mean()
        assert ((g["tri"] >= 0) == ref["hit"])[ref["hit_robust"]].all()
        assert (g["tri"] == ref["tri"])[rob].all()
    assert (want[tq.CLOSEST]["tri"] >= 0).sum() > 20
    ctx.set_kernel(rto.KERNEL_AUTO)


@gpu
def test_frustum_streams_sizes_and_errors(ctx, orc):
    """A frustum update in force (and switched off again) changes no record; the device forms on a caller's stream; n = 0, 1, 65;
    misaligned buffers, unknown modes and NULL buffers; RTO_E_NO_OCTREE on a fresh context, after a new octree upload (triangles
    freed), and a valid answer again once triangles are uploaded."""
    torch = pytest.importorskip("torch")
    rto = _rto()
    from ray_tracing_octrees_amd import hip
    g, nodes, tris, off, view, pos, W, H, fov, _ = _scene(orc, "sphere32")
    T = q.Tree32(nodes, g.min, g.voxel_size)
    o, d, tmn, tmx = _seeded(T, tris, off, 2048, 61)
    rays = hip.make_rays(o, d, tmn, tmx)
    _upload(ctx, nodes, g.min, g.voxel_size, tris, off)
    f = rto.make_frame(view, pos, W / H, fov, W, H)
    xy = _all_pixels(W, H)
    before = {m: (ctx.query_triangle_records(rays, m), ctx.query_triangle_pixels(f, xy, m)) for m in MODES}
    planes = np.array([[1, 0, 0, 0.45], [-1, 0, 0, -0.40], [0, 1, 0, 0.5], [0, -1, 0, 0.5], [0, 0, 1, 0.5], [0, 0, -1, 0.5]], np.float32)
    ctx.debug_update_frustum_planes(planes, 0.0)
    assert ctx.info().culling_active == 1 and ctx.info().visible_nodes < len(nodes) // 2
    for phase in ("culling on", "culling off"):
        for m in MODES:
            _recs_equal(ctx.query_triangle_records(rays, m), before[m][0], f"mode {m}: rays, {phase}")
            _recs_equal(ctx.query_triangle_pixels(f, xy, m), before[m][1], f"mode {m}: pixels, {phase}")
        ctx.update_frustum(view, fov, W / H, enable=False)
    full = before[tq.CLOSEST][0]
    for n in (1, 65):
        _recs_equal(ctx.query_triangle_records(rays[:n], tq.CLOSEST), full[:n], f"n = {n}")
    assert len(ctx.query_triangle_records(rays[:0], tq.CLOSEST)) == 0
    # device forms on a non-default stream
    other = torch.cuda.Stream()
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda")
    d_hits = torch.zeros(len(rays) * 32 + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.query_triangles_device(tq.CLOSEST, d_rays.data_ptr(), len(rays), d_hits.data_ptr(), other.cuda_stream)
    other.synchronize()
    _recs_equal(d_hits[:len(rays) * 32].cpu().numpy().view(tq.TRI_HIT_DTYPE), full, "device form on a caller's stream")
    d_xy = torch.from_numpy(xy).to("cuda")
    d_ph = torch.zeros(len(xy) * 32, dtype=torch.uint8, device="cuda")
    ctx.query_triangle_pixels_device(tq.FIRST, f, d_xy.data_ptr(), len(xy), d_ph.data_ptr(), other.cuda_stream)
    other.synchronize()
    _recs_equal(d_ph.cpu().numpy().view(tq.TRI_HIT_DTYPE), before[tq.FIRST][1], "pixels, device form")
    out = ctx.query_triangle_pixels(f, np.array([[-1, 0], [0, -1], [W, 0], [0, H]], np.int32), tq.FIRST)
    assert (out["tri"] == -1).all() and (out["t"] == tq.MISS_T).all()
    # error codes
    L = ctx._L
    hits = np.zeros(4, tq.TRI_HIT_DTYPE)
    assert L.rto_query_triangles_host(ctx._h, 7, rays.ctypes.data, 4, hits.ctypes.data) == hip.RTO_E_INVALID
    assert L.rto_query_triangles_host(ctx._h, -1, rays.ctypes.data, 4, hits.ctypes.data) == hip.RTO_E_INVALID
    assert L.rto_query_triangles_host(ctx._h, 1, None, 4, hits.ctypes.data) == hip.RTO_E_INVALID
    assert L.rto_query_triangles_host(ctx._h, 1, rays.ctypes.data, 4, None) == hip.RTO_E_INVALID
    assert L.rto_query_triangles_host(ctx._h, 1, None, 0, None) == hip.RTO_OK
    assert L.rto_query_triangles_device(ctx._h, 1, C.c_void_p(d_rays.data_ptr() + 4), 4, C.c_void_p(d_hits.data_ptr()), None) == hip.RTO_E_INVALID
    assert L.rto_query_triangles_device(ctx._h, 1, C.c_void_p(d_rays.data_ptr()), 4, C.c_void_p(d_hits.data_ptr() + 8), None) == hip.RTO_E_INVALID
    assert L.rto_query_triangle_pixels_device(ctx._h, 0, C.byref(f), C.c_void_p(d_xy.data_ptr()), 4, C.c_void_p(d_ph.data_ptr() + 4), None) == hip.RTO_E_INVALID
    assert L.rto_query_triangle_pixels_host(ctx._h, 3, C.byref(f), xy.ctypes.data, 4, hits.ctypes.data) == hip.RTO_E_INVALID
    assert L.rto_query_triangle_pixels_host(ctx._h, 0, None, xy.ctypes.data, 4, hits.ctypes.data) == hip.RTO_E_INVALID
    # no triangles resident: a new octree frees them
    ctx.upload_octree(nodes, g.min, g.voxel_size)
    for call in (lambda: ctx.query_triangle_records(rays[:4], tq.CLOSEST), lambda: ctx.query_triangle_pixels(f, xy[:4], tq.FIRST)):
        with pytest.raises(hip.RtoError) as e:
            call()
        assert e.value.code == hip.RTO_E_NO_OCTREE
    assert len(ctx.query_rays(o[:4], d[:4])) == 4                     # the box queries still answer
    ctx.upload_leaf_triangles(tris, off)
    _recs_equal(ctx.query_triangle_records(rays, tq.CLOSEST), full, "after the triangles came back")
    fresh = rto.Context(0)
    try:
        with pytest.raises(hip.RtoError) as e:
            fresh.query_triangles(o[:4], d[:4])
        assert e.value.code == hip.RTO_E_NO_OCTREE
    finally:
        fresh.close()


@gpu
def test_drop_in_class_intersect_triangles_and_pick_surface(orc):
    """RayTracerBVH::intersectTriangles equals the C ABI's records, with the point o + d t; pickSurface at sampled pixels returns
    the triangle renderSceneTriangles shades there (the frame's pixel is its shade) and the point on the render's ray."""
    rto = _rto()
    W, H = 96, 72
    grid = rto.VoxelGrid.test_sphere(64)
    root = rto.createOctreeFromVoxelGrid(grid)
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    rt.setOctree(root, grid)
    rt.buildLeafTriangles()
    ctx = None
    try:
        ctx = rto.Context(0)
        og = orc.test_sphere_grid(64)
        nodes = orc.build_flat_octree(og)
        ctx.upload_octree(nodes, og.min, og.voxel_size)
        ctx.build_leaf_triangles(og.data)                             # the builder buildLeafTriangles runs
        T = q.Tree32(nodes, og.min, og.voxel_size)
        o, d, _, _ = q.seeded_rays(T, 2048, 71, windows_too=False)
        o, d = o[:-8], d[:-8]
        for m in MODES:
            got, pts = rt.intersectTriangles(o, d, m, 0.0, 1e30)
            want = ctx.query_triangles(o, d, 0.0, 1e30, m)
            _recs_equal(got, want, f"intersectTriangles mode {m}", mask_only=(m == tq.ANY))
            h = got["tri"] >= 0
            p = (o + (d * got["t"][:, None]).astype(np.float32)).astype(np.float32)
            assert (pts[h] == p[h]).all() and (pts[~h] == 0).all()
        got, _ = rt.intersectTriangles(o, d, tq.CLOSEST, 0.05, 0.9)
        _recs_equal(got, ctx.query_triangles(o, d, 0.05, 0.9, tq.CLOSEST), "intersectTriangles with a window")
    finally:
        if ctx is not None:
            ctx.close()
    cam = rto.Camera(0.5, 0.7, 1.8)
    rt.renderSceneTriangles(cam, W, H, W / H, 45.0, False)
    img = rt.framebuffer()
    assert img is not None
    rd = orc.generate_rays(cam.getView(), cam.getPos(), W / H, 45.0, W, H).reshape(-1, 3)
    pos = np.asarray(cam.getPos(), np.float32)
    rng = np.random.default_rng(3)
    pix = np.concatenate([rng.integers(0, [W, H], (300, 2)), [[W // 2, H // 2], [0, 0], [W - 1, H - 1]]])
    lit = 0
    for px, py in pix:
        r = rt.pickSurface(cam, int(px), int(py), W, H, W / H, 45.0)
        want = img[py, px]
        assert (r is not None) == bool(want[0] > 0.05), (px, py)
        if r is None:
            continue
        lit += 1
        h, point = r
        rec = np.array([h], tq.TRI_HIT_DTYPE)
        assert tq.shade(rec)[0].tobytes() == want.tobytes(), (px, py)
        dd = rd[py * W + px]
        assert (point == (pos + (dd * h["t"]).astype(np.float32)).astype(np.float32)).all(), (px, py)
    assert lit > 20
    assert rt.pickSurface(cam, -1, 0, W, H, W / H, 45.0) is None
    rto.freeOctree(root)
