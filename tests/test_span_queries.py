"""Span queries (rto_query_spans_*, Context.query_spans, RayTracerBVH::intersectSpans / pickSpan): the solid path length, the
leaf count and the entry / exit parameters of a ray through the octree.  CPU: the float32 statement of the rule (tests/span_ref.py)
against query_ref's CLOSEST and ANY, against hand arithmetic on a scene of slabs and against float64; the ABI's layout; the built
assembly of the k_span_* kernels.  GPU: the records against that statement, byte for byte."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import deep_scenes as ds
import query_ref as q
import ref64
import span_ref as sp
from conftest import SPHERE_CAM, make_camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOV = 45.0
VGPR_DESC, VGPR_NODES = 80, 64          # 6 waves per SIMD (512 / 6 = 85, allocated by 8) / 8 waves


def _spans_equal(got, want, what):
    neq = (got.view(np.int32).reshape(-1, 8) != want.view(np.int32).reshape(-1, 8)).any(1)
    bad = np.nonzero(neq)[0]
    assert not len(bad), f"{what}: {len(bad)} of {len(got)} records differ, e.g. rays {bad[:5]}: got {got[bad[:3]]} want {want[bad[:3]]}"


def _closest_part_equal(span, hit, what):
    """(t_enter, node, face) of span records against CLOSEST hit records, t bitwise."""
    for a, b in (("t_enter", "t"), ("node", "node"), ("face", "face")):
        bad = np.nonzero(span[a].view(np.int32) != hit[b].view(np.int32))[0]
        assert not len(bad), f"{what}: {a} differs from CLOSEST's {b} on {len(bad)} rays, e.g. {bad[:5]}: {span[bad[:3]]} {hit[bad[:3]]}"


def _pixel_rays(orc, view, pos, W, H):
    return orc.generate_rays(view, pos, W / H, FOV, W, H).reshape(-1, 3)


def _all_pixels(W, H):
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([x.ravel(), y.ravel()], 1).astype(np.int32)


_CACHE = {}


def _seeded(scenes, scene, n, seed):
    """(scene, Tree32, rays, span32 records) computed once per (scene, n, seed) and shared; callers leave them unchanged."""
    key = (scene, n, seed)
    if key not in _CACHE:
        s = scenes(scene)
        T = q.Tree32(s.nodes, s.min, s.voxel)
        rays = q.seeded_rays(T, n, seed)
        _CACHE[key] = (s, T, rays, sp.span32(T, *rays))
    return _CACHE[key]


def _slabs(orc):
    if "slabs" not in _CACHE:
        data, gmin, voxel = sp.slab_scene()
        g = orc.Grid((16, 16, 16), gmin, voxel, data)
        _CACHE["slabs"] = (g, orc.build_flat_octree(g))
    return _CACHE["slabs"]


def _column_leaves(nodes, ix, iy):
    """Solid leaves of the octree whose box holds the voxel column (ix, iy)."""
    leaf = ((nodes["isLeaf"] == 1) | (nodes["isUniform"] == 1)) & (nodes["isSolid"] == 1)
    return int((leaf & (nodes["x"] <= ix) & (ix < nodes["x"] + nodes["size"]) & (nodes["y"] <= iy) & (iy < nodes["y"] + nodes["size"])).sum())


VS = 2.0 ** -4
COL = (7, 5)                                                       # the voxel column of the axis rays
CX, CY = -0.5 + (COL[0] + 0.5) * VS, -0.5 + (COL[1] + 0.5) * VS
# (origin, direction, t_min, t_max) -> (length, t_enter, t_exit, leaves or None = the column's, face); all exact in float32.
# Along +z from z = -1 the slabs lie at t in [0.625, 0.6875], [0.8125, 0.9375], [1.0625, 1.375]; along -z from z = 1 the same
# intervals in the other order of slabs.
AXIS_CASES = [
    ((CX, CY, -1.0), (0, 0, 1), 0.0, 1e30, (8 * VS, 0.625, 1.375, None, 4)),
    ((CX, CY, 1.0), (0, 0, -1), 0.0, 1e30, (8 * VS, 0.625, 1.375, None, 5)),
    ((CX, CY, -1.0), (0, 0, 1), 0.0, 0.84375, (VS + 0.03125, 0.625, 0.84375, 2, 4)),        # ends inside the middle slab (voxel z = 5)
    ((CX, CY, -1.0), (0, 0, 1), 1.15625, 1e30, (1.375 - 1.15625, 1.15625, 1.375, 2, -1)),    # starts inside the leaf z = [10, 12)
    ((CX, CY, -1.0), (0, 0, 1), 0.7, 0.8, None),                                              # wholly in the first gap: a miss
]


def _check_axis_cases(records, nodes, what):
    for rec, (_, _, _, _, want) in zip(records, AXIS_CASES):
        if want is None:
            assert rec.tobytes() == sp.miss_records(1).tobytes(), (what, rec)
            continue
        length, t0, t1, leaves, face = want
        leaves = _column_leaves(nodes, *COL) if leaves is None else leaves
        assert (rec["length"], rec["t_enter"], rec["t_exit"], rec["leaves"], rec["face"]) == \
            (np.float32(length), np.float32(t0), np.float32(t1), leaves, face), (what, rec, want)


def _axis_rays():
    o = np.array([c[0] for c in AXIS_CASES], np.float32)
    d = np.array([c[1] for c in AXIS_CASES], np.float32)
    return o, d, np.array([c[2] for c in AXIS_CASES], np.float32), np.array([c[3] for c in AXIS_CASES], np.float32)


def _chords(T, n, seed):
    """Rays that start and end outside the root box and cross it, and their reversals: both end points on a lattice of float32
    numbers, so that the direction b - a and its negation are exact and the two rays are the same line.  Returns (a, b)."""
    rng = np.random.default_rng(seed)
    lo, hi = T.bmin[0].astype(np.float64), T.bmax[0].astype(np.float64)
    ext = float((hi - lo).max())
    h = 2.0 ** np.floor(np.log2(ext)) / 1024
    sl = np.nonzero(T.solid)[0]                                     # aimed at points of solid leaves: most chords meet some solid
    pick = sl[rng.integers(0, len(sl), n)]
    tgt = T.bmin[pick] + rng.random((n, 3)) * (T.bmax[pick].astype(np.float64) - T.bmin[pick])
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    a = np.round((tgt + u * ext * rng.uniform(1.8, 2.5, (n, 1))) / h) * h      # farther from the target than the box's diagonal
    b = np.round((tgt - u * ext * rng.uniform(1.8, 2.5, (n, 1))) / h) * h
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    assert (a32 == a).all() and (b32 == b).all() and ((b32 - a32).astype(np.float64) == b - a).all()
    return a32, b32


# ================================================================ CPU
@pytest.mark.parametrize("scene,seed", [("sphere64", 1), ("odd", 2), ("calgary", 3)])
def test_statement_agrees_with_closest_and_any(scenes, scene, seed):
    """span32's (t_enter, node, face) are query32's CLOSEST records bit for bit, leaves > 0 is its ANY mask; t_exit >= t_enter,
    length <= t_exit - t_enter up to the sum's rounding, and a miss is the miss record."""
    s, T, (o, d, tmn, tmx), span = _seeded(scenes, scene, 2048, seed)
    r = q.query32(T, o, d, tmn, tmx)
    _closest_part_equal(span, r[q.CLOSEST], scene)
    assert ((span["leaves"] > 0) == (r[q.ANY]["node"] >= 0)).all()
    hit = span["leaves"] > 0
    assert hit.any() and (~hit).any() and (span["leaves"][hit] > 1).any()
    assert span[~hit].tobytes() == sp.miss_records(int((~hit).sum())).tobytes()
    assert (span["t_exit"][hit] >= span["t_enter"][hit]).all() and (span["length"][hit] >= 0).all()
    width = (span["t_exit"][hit].astype(np.float64) - span["t_enter"][hit]) * (1 + span["leaves"][hit] * 2.0 ** -22)
    assert (span["length"][hit] <= width + 1e-30).all()
    assert (span["reserved"] == 0).all() and (span["leaves"][-7:-1] == 0).all()       # NaN rays and t_min > t_max


def test_slabs_by_hand(orc):
    """The scene of z-slabs 1, 2 and 5 voxels thick (exact grid): axis rays through a voxel centre give 8 voxels of solid exactly,
    the outer faces as t_enter / t_exit and the column's leaves; windows that end inside the middle slab, start inside a leaf and
    lie in a gap; an oblique ray's length is the axis length over |d.z| / |d| within the float64 bound."""
    g, nodes = _slabs(orc)
    assert _column_leaves(nodes, *COL) == 6                          # 1 + 2 voxels, then z = 9 and the size-2 leaves [10, 12), [12, 14)
    T = q.Tree32(nodes, g.min, g.voxel_size)
    _check_axis_cases(sp.span32(T, *_axis_rays()), nodes, "span32")
    dn = np.array([0.3, 0.2, 1.0]) / np.linalg.norm([0.3, 0.2, 1.0])
    o = np.array([[-0.2, -0.1, -1.0], [0.2, 0.15, 1.0]], np.float32)
    d = np.array([dn, -dn], np.float32)
    got = sp.span32(T, o, d)
    ref = sp.Octree64S(nodes, g.min, g.voxel_size).span_windows(o, d)
    d64 = d.astype(np.float64)
    norm = np.linalg.norm(d64, axis=1)                             # length is in units of d: times |d| it is a distance
    want = 8 * VS / (np.abs(d64[:, 2]) / norm)
    print("oblique:", got["length"] * norm, want, ref["length"] * norm, ref["tol"])
    assert (np.abs(ref["length"] * norm - want) <= 1e-12).all()
    assert (np.abs(got["length"] * norm - want) <= ref["tol"] * norm).all() and (ref["tol"] < 1e-4).all()
    assert (got["leaves"] >= 6).all()


@pytest.mark.parametrize("scene,seed", [("sphere64", 1), ("odd", 2), ("calgary", 3)])
def test_length_against_float64(scenes, scene, seed):
    """Every seeded ray, none excluded: |length32 - length64| <= the bound Octree64S.span_windows derives from ref64's slab error
    terms.  Two guards keep that bound from growing into an exclusion:
      * the rays whose bound carries a whole chord (`flat`: a zero direction component and the origin on a box plane) are at most
        the half of the grazing family that seeded_rays builds that way, n / 16, plus 1 % for sampling and for origins that land on
        a plane by chance -- and there are some, so the case is exercised;
      * on the other rays with solid on their way the median of tol / length is at most 32 K EPS M / voxel, M the largest
        coordinate of the root box.  A leaf's term is en + ef, each at most K EPS ((|box| + |o|) |1/d| + |t|) on the deciding axis;
        the seeded origins lie within 2 root extents of the centre and the rays' |t d| within 4, so en + ef <= 16 K EPS M |1/d|,
        while the chord of a leaf of s voxels is about s voxel |1/d|: a ratio of 16 K EPS M / (s voxel), doubled for the quarter of
        the rays whose window clips their chords.  (K EPS M / voxel itself is 8e-6, 1e-5 and 1.2e-4 on the three scenes: no
        first-order bound with ref64's K = 4 can be tighter than that.)"""
    s, T, (o, d, tmn, tmx), span = _seeded(scenes, scene, 2048, seed)
    ref = sp.Octree64S(s.nodes, s.min, s.voxel).span_windows(o, d, tmn, tmx)
    err = np.abs(span["length"].astype(np.float64) - ref["length"])
    bad = np.nonzero(~(err <= ref["tol"]))[0]
    print(scene, "max err", err.max(), "max err / tol", np.nanmax(err / np.maximum(ref["tol"], 1e-300)))
    assert not len(bad), (bad[:5], err[bad[:5]], ref["tol"][bad[:5]], span[bad[:5]])
    flat = ref["flat"]
    print(scene, "flat rays", int(flat.sum()), "of", len(flat), "max err off them", err[~flat].max())
    assert 0 < flat.sum() <= len(flat) // 16 + len(flat) // 100
    rest = (ref["length"] > 0) & ~flat
    M = float(np.abs(np.concatenate([T.bmin[0], T.bmax[0]])).max())
    rel = np.median(ref["tol"][rest] / ref["length"][rest])
    print(scene, "rays off the flat set with solid", int(rest.sum()), "median tol / length", rel, "cap", 32 * ref64.K * ref64.EPS * M / float(s.voxel))
    assert rest.sum() > 200 and rel <= 32 * ref64.K * ref64.EPS * M / float(s.voxel)


@pytest.mark.parametrize("scene,seed", [("sphere64", 4), ("odd", 5), ("calgary", 6)])
def test_reversed_rays_cross_the_same_leaves(scenes, scene, seed):
    """A ray from a to b, both outside the root box, and the ray from b to a (t in [0, 1] covers the box either way): the same
    number of leaves, and lengths within the two rays' summed float64 bounds."""
    s = scenes(scene)
    T = q.Tree32(s.nodes, s.min, s.voxel)
    a, b = _chords(T, 256, seed)
    fwd, rev = sp.span32(T, a, b - a), sp.span32(T, b, a - b)
    hit = fwd["leaves"] > 0
    assert hit.sum() > 100
    assert (fwd["leaves"] == rev["leaves"]).all(), np.nonzero(fwd["leaves"] != rev["leaves"])[0][:5]
    S = sp.Octree64S(s.nodes, s.min, s.voxel)
    tf, tr = S.span_windows(a, b - a)["tol"], S.span_windows(b, a - b)["tol"]
    assert (np.abs(fwd["length"].astype(np.float64) - rev["length"]) <= tf + tr).all()
    assert (fwd["t_exit"][hit] < 1).all() and (rev["t_exit"][hit] < 1).all()   # both end points are past the box


def test_span_structs_are_32_bytes():
    from ray_tracing_octrees_amd import hip
    assert C.sizeof(hip.Span) == 32 and hip.SPAN_DTYPE.itemsize == 32 and sp.SPAN_DTYPE.itemsize == 32
    assert hip.SPAN_DTYPE == sp.SPAN_DTYPE
    assert [f[0] for f in hip.Span._fields_] == list(hip.SPAN_DTYPE.names)
    hdr = open(os.path.join(ROOT, "include", "rto_hip.h")).read()
    assert re.search(r"typedef struct rto_span \{\s*/\* 32 bytes \*/", hdr)
    for sym, args in (("rto_query_spans_device", r"rto_context\* ctx, const rto_ray\* d_rays, int64_t n, rto_span\* d_spans, void\* hip_stream"),
                      ("rto_query_spans_host", r"rto_context\* ctx, const rto_ray\* rays, int64_t n, rto_span\* spans"),
                      ("rto_query_span_pixels_device", r"rto_context\* ctx, const rto_frame\* frame, const int32_t\* d_xy, int64_t n, rto_span\* d_spans,\s*void\* hip_stream"),
                      ("rto_query_span_pixels_host", r"rto_context\* ctx, const rto_frame\* frame, const int32_t\* xy, int64_t n, rto_span\* spans")):
        assert re.search(rf"int\s+{sym}\({args}\);", hdr), sym
        assert sym in hip.SYMBOLS and hasattr(hip.load(), sym)


def test_span_kernels_keep_their_budgets():
    """The built assembly (the product's flags): the four k_span_* kernels without scratch, spills or v_mfma; k_span_desc within 80
    VGPRs, k_span_nodes within 64."""
    import test_isa_contract as isa
    asm = isa.built_asm()
    if asm is None:
        pytest.skip("no hipcc in this environment")
    meta = isa.kernel_meta(asm)
    names = [k for k in meta if "k_span_" in k]
    assert len(names) == 4, names                                     # {desc, nodes} x {rays, pixels}
    assert not any("k_query_" in k or "k_triq_" in k for k in names)
    for k in names:
        m = meta[k]
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (k, m)
        assert m["vgpr"] <= (VGPR_DESC if "k_span_desc" in k else VGPR_NODES), (k, m)
        ins = isa.body(asm, k[len("_ZN3rto"):])
        assert not any(t.startswith(("scratch_", "buffer_load", "buffer_store")) or "v_mfma" in t for t in ins), k


# ================================================================ GPU
gpu = pytest.mark.gpu


def _rto():
    import ray_tracing_octrees_amd as rto
    return rto


def _upload(ctx, s, kernel=None):
    rto = _rto()
    ctx.set_kernel(rto.KERNEL_AUTO if kernel is None else kernel)
    ctx.upload_octree(s.nodes, s.min, s.voxel)


@gpu
@pytest.mark.parametrize("scene,seed", [("sphere64", 11), ("odd", 12), ("calgary", 13), ("sphere256", 14)])
def test_seeded_rays_match_the_float32_statement(ctx, scenes, scene, seed):
    """Rays of every kind (outside / inside / inside solid leaves, axis-aligned, zero components, grazing, windows, NaN, t_min >
    t_max): the records of span32 byte for byte on the descriptor kernel and on the node kernel, hence equal to each other, length
    included; the CLOSEST part is query_rays' CLOSEST record and leaves > 0 its ANY mask."""
    rto = _rto()
    s, T, (o, d, tmn, tmx), want = _seeded(scenes, scene, 4096, seed)
    assert (want["leaves"] > 1).sum() > 200
    for kernel in (rto.KERNEL_AUTO, rto.KERNEL_GENERIC):
        _upload(ctx, s, kernel)
        got = ctx.query_spans(o, d, tmn, tmx)
        _spans_equal(got, want, f"{scene} kernel {kernel}")
        _closest_part_equal(got, ctx.query_rays(o, d, tmn, tmx, q.CLOSEST), f"{scene} kernel {kernel}")
        assert ((got["leaves"] > 0) == (ctx.query_rays(o, d, tmn, tmx, q.ANY)["node"] >= 0)).all()
    ctx.set_kernel(rto.KERNEL_AUTO)


@gpu
@pytest.mark.parametrize("scene,cam", [("sphere64", SPHERE_CAM), ("sphere64", (0.3, 0.2, 0.1)), ("sphere64", (0.0, 0.0, 1.8)),
                                       ("calgary", "calgary_oblique")])
def test_pixel_spans(ctx, orc, scenes, camera, scene, cam):
    """Every pixel of a 96 x 96 frame (camera outside, inside a solid leaf, axis-aligned; calgary oblique): span32 on
    orc.generate_rays, query_spans on the same rays, and query_pixels' CLOSEST record in (t_enter, node, face)."""
    rto = _rto()
    s = scenes(scene)
    _upload(ctx, s)
    W = H = 96
    view, pos = camera(cam) if isinstance(cam, str) else make_camera(orc, *cam)
    f = rto.make_frame(view, pos, W / H, FOV, W, H)
    rd = _pixel_rays(orc, view, pos, W, H)
    xy = _all_pixels(W, H)
    got = ctx.query_span_pixels(f, xy)
    _spans_equal(got, sp.span32(q.Tree32(s.nodes, s.min, s.voxel), pos, rd), "pixels vs span32")
    _spans_equal(ctx.query_spans(np.broadcast_to(pos, rd.shape), rd), got, "query_spans vs query_span_pixels")
    _closest_part_equal(got, ctx.query_pixels(f, xy, q.CLOSEST), "pixels")
    assert (got["leaves"] > 0).sum() > 100
    out = ctx.query_span_pixels(f, np.array([[-1, 0], [0, -1], [W, 0], [0, H]], np.int32))
    assert out.tobytes() == sp.miss_records(4).tobytes()            # outside the frame: misses, not errors


@gpu
def test_sizes_streams_and_errors(ctx, orc, scenes):
    """n of 1, 63, 64, 65, 255, 257 and 0; a slice of a larger device buffer that does not start at its base; a caller's stream;
    misaligned buffers and the other error codes, each leaving the context usable."""
    torch = pytest.importorskip("torch")
    rto = _rto()
    from ray_tracing_octrees_amd import hip
    s, T, (o, d, tmn, tmx), want = _seeded(scenes, "sphere64", 4096, 11)
    rays = hip.make_rays(o, d, tmn, tmx)
    for kernel in (rto.KERNEL_AUTO, rto.KERNEL_GENERIC):
        _upload(ctx, s, kernel)
        for n in (1, 63, 64, 65, 255, 257):
            _spans_equal(ctx.query_span_records(rays[:n]), want[:n], f"kernel {kernel} n = {n}")
    _upload(ctx, s)
    assert len(ctx.query_span_records(rays[:0])) == 0
    other = torch.cuda.Stream()
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda")
    d_spans = torch.full((len(rays) * 32,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    first, n = 1000, 257                                            # records 1000 .. 1256 of both buffers
    ctx.query_spans_device(d_rays.data_ptr() + 32 * first, n, d_spans.data_ptr() + 32 * first, other.cuda_stream)
    other.synchronize()
    back = d_spans.cpu().numpy()
    _spans_equal(back[32 * first:32 * (first + n)].view(hip.SPAN_DTYPE), want[first:first + n], "slice on a caller's stream")
    assert (back[:32 * first] == 0xAB).all() and (back[32 * (first + n):] == 0xAB).all()
    view, pos = make_camera(orc, *SPHERE_CAM)
    f = rto.make_frame(view, pos, 32 / 24, FOV, 32, 24)
    xy = torch.from_numpy(_all_pixels(32, 24)).to("cuda")
    d_ps = torch.zeros(32 * 24 * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.query_span_pixels_device(f, xy.data_ptr(), 32 * 24, d_ps.data_ptr(), other.cuda_stream)
    other.synchronize()
    _spans_equal(d_ps.cpu().numpy().view(hip.SPAN_DTYPE), ctx.query_span_pixels(f, _all_pixels(32, 24)), "pixels, device form")
    # error codes; after each the context answers as before
    L = ctx._L
    out = np.zeros(4, hip.SPAN_DTYPE)
    vp = C.c_void_p
    bad = [L.rto_query_spans_host(ctx._h, None, 4, out.ctypes.data), L.rto_query_spans_host(ctx._h, rays.ctypes.data, 4, None),
           L.rto_query_spans_host(ctx._h, rays.ctypes.data, -1, out.ctypes.data),
           L.rto_query_spans_device(ctx._h, None, 4, vp(d_spans.data_ptr()), None),
           L.rto_query_spans_device(ctx._h, vp(d_rays.data_ptr() + 8), 4, vp(d_spans.data_ptr()), None),
           L.rto_query_spans_device(ctx._h, vp(d_rays.data_ptr()), 4, vp(d_spans.data_ptr() + 4), None),
           L.rto_query_span_pixels_device(ctx._h, C.byref(f), vp(xy.data_ptr()), 4, vp(d_ps.data_ptr() + 8), None),
           L.rto_query_span_pixels_host(ctx._h, None, xy.data_ptr(), 4, out.ctypes.data),
           L.rto_query_span_pixels_host(ctx._h, C.byref(f), None, 4, out.ctypes.data)]
    assert bad == [hip.RTO_E_INVALID] * len(bad), bad
    assert L.rto_query_spans_host(ctx._h, None, 0, None) == hip.RTO_OK
    _spans_equal(ctx.query_span_records(rays[:257]), want[:257], "after the refused calls")
    fresh = rto.Context(0)
    try:
        assert fresh._L.rto_query_spans_host(fresh._h, None, 0, None) == hip.RTO_OK              # n == 0 with nothing resident
        assert fresh._L.rto_query_span_pixels_device(fresh._h, None, None, 0, None, None) == hip.RTO_OK
        for call in (lambda: fresh.query_spans(o[:4], d[:4]), lambda: fresh.query_span_pixels(f, _all_pixels(4, 4))):
            with pytest.raises(hip.RtoError) as e:
                call()
            assert e.value.code == hip.RTO_E_NO_OCTREE
        fresh.upload_octree(s.nodes, s.min, s.voxel)
        _spans_equal(fresh.query_span_records(rays[:65]), want[:65], "a context that had refused")
    finally:
        fresh.close()


def _permuted(nodes, rng):
    """The same tree under another numbering: root kept at 0, every other node moved, child indices remapped (slots kept)."""
    n = len(nodes)
    perm = np.concatenate([[0], 1 + rng.permutation(n - 1)])          # new index of old node i = perm[i]
    out = np.zeros_like(nodes)
    out[perm] = nodes
    ch = out["child"]
    out["child"] = np.where(ch >= 0, perm[np.maximum(ch, 0)], -1)
    return out


@gpu
def test_permuted_gpu_built_and_one_leaf_arrays(ctx, scenes):
    """A non-canonical numbering of the tree and the tree rto_build_octree makes give the statement's records for that array; a
    one-leaf tree, solid (every ray through it: one leaf, its chord) and empty (misses)."""
    s, T, (o, d, tmn, tmx), want = _seeded(scenes, "sphere64", 4096, 11)
    perm_nodes = _permuted(s.nodes, np.random.default_rng(5))
    ctx.upload_octree(perm_nodes, s.min, s.voxel)
    assert ctx.info().canonical == 0
    _spans_equal(ctx.query_spans(o, d, tmn, tmx), sp.span32(q.Tree32(perm_nodes, s.min, s.voxel), o, d, tmn, tmx), "permuted array")
    ctx.build_octree(s.grid.data, s.min, s.voxel)
    assert ctx.download_nodes().tobytes() == s.nodes.tobytes()
    _spans_equal(ctx.query_spans(o, d, tmn, tmx), want, "rto_build_octree's tree")
    for solid in (1, 0):
        one = np.zeros(1, s.nodes.dtype)
        one["size"], one["isLeaf"], one["isUniform"], one["isSolid"], one["child"] = 64, 1, 1, solid, -1
        ctx.upload_octree(one, s.min, s.voxel)
        got = ctx.query_spans(o, d, tmn, tmx)
        _spans_equal(got, sp.span32(q.Tree32(one, s.min, s.voxel), o, d, tmn, tmx), f"one leaf, solid {solid}")
        assert (got["leaves"] <= solid).all() and (got["leaves"] > 0).any() == bool(solid)


def _slot_permuted(nodes, rng):
    """The same boxes with the child slots of every internal node shuffled: slot k no longer holds octant k."""
    out = nodes.copy()
    ch = out["child"]
    for i in np.nonzero((nodes["isLeaf"] == 0) & (nodes["isUniform"] == 0))[0]:
        ch[i] = ch[i][rng.permutation(8)]
    out["child"] = ch
    return out


def _edge_rays():
    """Rays in the slab scene that enter the first slab on their way exactly through the edge two of its leaves share (d = (+-1, 0,
    +-1), the entry point on a leaf boundary in x -- the top slab's leaves are 2 voxels wide --, t = 1 there, all exact): both
    leaves have tIn = 1, one of them with a chord of zero length."""
    o, d = [], []
    for ix in (4, 8, 10):
        for (z0, z1), sx, sz in ((sp.SLABS[0], 1, 1), (sp.SLABS[0], -1, 1), (sp.SLABS[2], 1, -1), (sp.SLABS[2], -1, -1)):
            zf = -0.5 + (z0 if sz > 0 else z1) * VS
            o.append((-0.5 + ix * VS - sx, CY, zf - sz))
            d.append((sx, 0, sz))
    return np.array(o, np.float32), np.array(d, np.float32)


@gpu
def test_ties_and_slot_permuted_arrays(ctx, orc, scenes):
    """Ties in tIn: rays through an edge two leaves share give span32's records and CLOSEST's (t, node, face) on both kernels.
    Then arrays whose child slots are not the octants of the children's boxes: the visit order, hence the sum, goes by slot and the
    tie in tIn by position, both as the rule says, so the records are span32's; t_enter is CLOSEST's t on every ray, and (node,
    face) are CLOSEST's wherever one leaf alone has the least tIn (the node-by-node CLOSEST query breaks ties by its pop order,
    which on such an array is not the order of positions: include/rto_hip.h says so)."""
    rto = _rto()
    g, slab_nodes = _slabs(orc)
    eo, ed = _edge_rays()
    for nodes, canonical in ((slab_nodes, 1), (_slot_permuted(slab_nodes, np.random.default_rng(9)), 0)):
        want, tie = sp.span32(q.Tree32(nodes, g.min, g.voxel_size), eo, ed, ties=True)
        assert tie.all() and (want["t_enter"] == 1).all()
        for kernel in (rto.KERNEL_AUTO, rto.KERNEL_GENERIC):
            ctx.set_kernel(kernel)
            ctx.upload_octree(nodes, g.min, g.voxel_size)
            assert ctx.info().canonical == canonical
            got = ctx.query_spans(eo, ed)
            _spans_equal(got, want, f"edge rays, canonical {canonical}, kernel {kernel}")
            if canonical:
                _closest_part_equal(got, ctx.query_rays(eo, ed, 0.0, 1e30, q.CLOSEST), f"edge rays, kernel {kernel}")
    ctx.set_kernel(rto.KERNEL_AUTO)
    s, T, (o, d, tmn, tmx), _ = _seeded(scenes, "sphere64", 4096, 11)
    nodes = _slot_permuted(s.nodes, np.random.default_rng(7))
    ctx.upload_octree(nodes, s.min, s.voxel)
    assert ctx.info().canonical == 0
    want, tie = sp.span32(q.Tree32(nodes, s.min, s.voxel), o, d, tmn, tmx, ties=True)
    got = ctx.query_spans(o, d, tmn, tmx)
    _spans_equal(got, want, "slot-permuted array")
    closest = ctx.query_rays(o, d, tmn, tmx, q.CLOSEST)
    assert (got["t_enter"].view(np.int32) == closest["t"].view(np.int32)).all()
    assert (got["leaves"][~tie] > 0).sum() > 500
    _closest_part_equal(got[~tie], closest[~tie], "slot-permuted array, rays without a tie")


def _chain(levels, slot):
    """A non-canonical chain: every level one internal node whose child `slot` is the next level and whose other 7 are solid
    leaves; every box is the voxel at the origin."""
    import ray_tracing_octrees_amd as rto
    chain = np.zeros(8 * levels + 1, rto.NODE_DTYPE)
    chain["size"] = 1
    chain["isLeaf"] = chain["isUniform"] = chain["isSolid"] = 1
    chain["child"] = -1
    p = 0
    for lvl in range(levels):
        chain["isLeaf"][p] = chain["isUniform"][p] = chain["isSolid"][p] = 0
        chain["child"][p] = 8 * lvl + 1 + np.arange(8)
        p = 8 * lvl + 1 + slot
    return chain


@gpu
def test_stack_need_in_octant_order(ctx, scenes):
    """The span walk pushes children in the ray's octant order, so the upload's bound on the stack, taken in slot order, does not
    cover it.  A 21-level chain with its internal child in slot 0 needs 8 entries in slot order and is accepted; with flip = 0 the
    span walk would pop slot 0 first and hold 7 * 21 + 1 = 148 > 141: the span entries refuse it with RTO_E_UNSUPPORTED, the box
    queries still answer, and the context stays usable.  The same chain of 20 levels (141 entries) is walked, for every flip."""
    from ray_tracing_octrees_amd import hip
    gmin, vs = np.full(3, -0.5, np.float32), np.float32(1.0)
    o = np.array([[-2, -2, -2], [2, 2, 2], [-2, 2, -2], [2, -2, 2], [3, 3, 3]], np.float32)
    d = np.array([[1, 1, 1], [-1, -1, -1], [1, -1, 1], [-1, 1, -1], [1, 1, 1]], np.float32)
    deep = _chain(21, 0)
    assert ds.stack_need(deep) == 8
    ctx.upload_octree(deep, gmin, vs)
    with pytest.raises(hip.RtoError) as e:
        ctx.query_spans(o, d)
    assert e.value.code == hip.RTO_E_UNSUPPORTED
    f = _rto().make_frame(np.eye(4, dtype=np.float32), (0.0, 0.0, 5.0), 1.0, FOV, 8, 8)
    with pytest.raises(hip.RtoError) as e:
        ctx.query_span_pixels(f, _all_pixels(8, 8))
    assert e.value.code == hip.RTO_E_UNSUPPORTED
    assert (ctx.query_rays(o, d, 0.0, 1e30, q.CLOSEST)["node"][:4] >= 0).all()
    for slot in (0, 7, 3):
        chain = _chain(20, slot)
        ctx.upload_octree(chain, gmin, vs)
        got = ctx.query_spans(o, d)
        _spans_equal(got, sp.span32(q.Tree32(chain, gmin, vs), o, d), f"20-level chain, internal child in slot {slot}")
        assert (got["leaves"][:4] == 7 * 20 + 1).all() and got["leaves"][4] == 0       # the last level's 8 children are all leaves
    s = scenes("sphere64")
    _upload(ctx, s)                                                  # a canonical tree after the refused array: walked again
    assert (ctx.query_spans(o * 0.25, d)["leaves"][:4] > 0).all()


@gpu
@pytest.mark.parametrize("kind,d", [("frac", 11), ("far", 16), ("tenth", 19), ("frac", 20)])
def test_deep_octrees_against_float64(ctx, orc, kind, d):
    """Depth 11-20 trees (tests/deep_scenes.py), pixel rays of the scene's cameras and seeded rays: both kernels give span32's
    records, and every ray's length lies within the float64 bound."""
    rto = _rto()
    s = ds.scene(kind, d)
    T = q.Tree32(s.nodes, s.min, s.voxel)
    W, H = 48, 40
    rays = []
    for _, view, pos in s.cameras(orc):
        rd = _pixel_rays(orc, view, pos, W, H)
        rays.append((np.broadcast_to(pos, rd.shape).astype(np.float32), rd, np.zeros(len(rd), np.float32), np.full(len(rd), 1e30, np.float32)))
    rays.append(q.seeded_rays(T, 1024, d))
    o, dd, tmn, tmx = (np.concatenate(x) for x in zip(*rays))
    want = sp.span32(T, o, dd, tmn, tmx)
    ref = sp.Octree64S(s.nodes, s.min, s.voxel).span_windows(o, dd, tmn, tmx)
    for kernel in (rto.KERNEL_AUTO, rto.KERNEL_GENERIC):
        _upload(ctx, s, kernel)
        got = ctx.query_spans(o, dd, tmn, tmx)
        _spans_equal(got, want, f"{kind}{d} kernel {kernel}")
        err = np.abs(got["length"].astype(np.float64) - ref["length"])
        bad = np.nonzero(~(err <= ref["tol"]))[0]
        assert not len(bad), (kind, d, bad[:5], err[bad[:5]], ref["tol"][bad[:5]])
    assert (want["leaves"] > 0).sum() > 100
    ctx.set_kernel(rto.KERNEL_AUTO)


@gpu
def test_spans_after_a_voxel_edit(ctx, orc):
    """The slab scene built on the GPU answers the hand arithmetic; carving a 4 x 4 x 2 box through the middle slab takes exactly
    its two voxels off the axis ray's length, and leaves is the rebuilt tree's column count."""
    from ray_tracing_octrees_amd import hip
    g, nodes = _slabs(orc)
    ctx.build_octree(g.data, g.min, g.voxel_size)
    o, d, tmn, tmx = _axis_rays()
    _check_axis_cases(ctx.query_spans(o, d, tmn, tmx), nodes, "GPU")
    centre = (-0.5 + 8 * VS, -0.5 + 6 * VS, -0.5 + 6 * VS)           # voxels x [6, 10), y [4, 8), z [5, 7)
    changed = ctx.edit_voxels(hip.make_brushes([centre], [(2 * VS, 2 * VS, VS)], hip.BRUSH_BOX, hip.EDIT_CARVE))
    want_grid = g.data.copy()
    want_grid[5:7, 4:8, 6:10] = 0
    assert changed == 32 and (ctx.download_voxels() == want_grid).all()
    rebuilt = ctx.download_nodes()
    got = ctx.query_spans(o[:2], d[:2])
    assert (got["length"] == np.float32(6 * VS)).all() and (got["leaves"] == _column_leaves(rebuilt, *COL)).all()
    assert _column_leaves(rebuilt, *COL) == 4
    assert (got["t_enter"] == np.float32(0.625)).all() and (got["t_exit"] == np.float32(1.375)).all()
    _spans_equal(got, sp.span32(q.Tree32(rebuilt, g.min, g.voxel_size), o[:2], d[:2]), "after the edit")


@gpu
def test_drop_in_class_intersect_spans_and_pick_span(scenes):
    """RayTracerBVH::intersectSpans and pickSpan give the C ABI's records."""
    rto = _rto()
    W, H = 96, 72
    grid = rto.VoxelGrid.test_sphere(64)
    root = rto.createOctreeFromVoxelGrid(grid)
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    rt.setOctree(root, grid)
    s, T, (o, d, _, _), _ = _seeded(scenes, "sphere64", 4096, 11)
    o, d = o[:2048], d[:2048]
    cam = rto.Camera(*SPHERE_CAM)
    ctx = rto.Context(0)
    try:
        ctx.upload_octree(s.nodes, s.min, s.voxel)
        _spans_equal(rt.intersectSpans(o, d), ctx.query_spans(o, d), "intersectSpans")
        _spans_equal(rt.intersectSpans(o, d, 0.05, 0.9), ctx.query_spans(o, d, 0.05, 0.9), "intersectSpans with a window")
        f = rto.make_frame(cam.getView(), cam.getPos(), W / H, FOV, W, H)
        rng = np.random.default_rng(3)
        pix = np.concatenate([rng.integers(0, [W, H], (60, 2)), [[W // 2, H // 2], [0, 0], [W, H]]]).astype(np.int32)
        want = ctx.query_span_pixels(f, pix)
        hits = 0
        for (px, py), w in zip(pix, want):
            got = rt.pickSpan(cam, int(px), int(py), W, H, W / H, FOV)
            assert (got is not None) == bool(w["leaves"] > 0), (px, py)
            if got is not None:
                hits += 1
                assert got.tobytes() == w.tobytes(), (px, py, got, w)
        assert hits > 5
    finally:
        ctx.close()
    rto.freeOctree(root)
