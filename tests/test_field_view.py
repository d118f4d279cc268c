"""Field views (rto_render_field_*, Context.render_field_*, RayTracerBVH::renderField): a frame of the octree coloured by an int32
volume of the resident grid.  CPU: the ABI's layout, the index arithmetic against brute force, ramp_lut against its formula, the
numpy statement (tests/field_view_ref.py) against the oracle's frame, the kernels' register figures.  GPU: values, colours, summary
and bins against that statement, bit for bit; against rto_query_pixels and rto_render_lit_host without it; FRONT, clip boxes, auto
range, adversarial values, the lifecycle, every error, a one-leaf tree, a full-size frame and the drop-in class.

Grids: the lifecycle suite's 40 x 12 x 12 (leaves of 1, 2 and 4 voxels) and a 32^3 grid with a 16^3 block (leaves of 8)."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import field_view_ref as fr
import query_ref as q
from conftest import SPHERE_CAM, make_camera

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOV = 45.0
VGPR_BUDGET = 80            # k_lit_primary's
GMIN, VOX = np.array([-0.5, -0.5, -0.5], np.float32), np.float32(1.0 / 64)
EXPO_DIRS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [-1, 2, 1]], np.int32)
REACH = 8
SOURCES = ("distance", "geodesic", "thickness", "skeleton", "exposure", "parts", "labels")


def _hip():
    from ray_tracing_octrees_amd import hip
    return hip


def _lut():
    return _hip().ramp_lut([(0, 0, 96, 255), (0, 200, 255, 255), (255, 255, 0, 200), (255, 32, 0, 255)])


def _base():
    g = np.zeros((12, 12, 40), np.uint8)             # tests/test_field_lifecycle.py's grid
    g[2:10, 2:10, 4:20] = 1
    g[6, 6, 30] = 1
    return g


def _block32():
    g = np.zeros((32, 32, 32), np.uint8)
    g[8:24, 8:24, 8:24] = 1
    return g


GRIDS = {"base": _base, "block32": _block32}
_TREES = {}


def _tree(orc, name):
    """(grid, oracle nodes, Tree32) of a named grid, made once."""
    if name not in _TREES:
        g = GRIDS[name]()
        nodes = orc.build_flat_octree(orc.Grid((g.shape[2], g.shape[1], g.shape[0]), GMIN, VOX, g))
        _TREES[name] = (g, nodes, q.Tree32(nodes, GMIN, VOX))
    return _TREES[name]


def _vpos(x, y, z):
    return (GMIN + np.array([x, y, z], np.float32) * VOX).astype(np.float32)


def _camera(orc, name):
    """(view, pos) by name, "name@R" for another orbit radius.  base grid: "outside" (oblique, at the block), "axis" (theta =
    phi = 0: the view axes are the world axes, so the centre pixel of an odd frame has two zero direction components), "low"
    (from below and behind), "inside" (in the size-2 leaf at the block's low corner, looking into the block: under FIRST part
    of the frame hits leaves popped earlier).  block32: "block" (oblique), "face" (head-on at the +z face)."""
    name, _, radius = name.partition("@")

    def orbit(th, ph, R, target):
        cam = orc.Camera(th, ph, float(radius) if radius else R)
        cam.set_target(*[float(v) for v in target])
        return cam.get_view(), cam.get_pos()
    if name == "outside":
        return orbit(0.6, 0.45, 0.45, _vpos(12, 6, 6))
    if name == "axis":
        return orbit(0.0, 0.0, 0.5, _vpos(20, 6, 6))
    if name == "low":
        return orbit(3.9, -0.5, 0.45, _vpos(12, 6, 6))
    if name == "inside":
        return orbit(3.7, -0.45, 0.45, _vpos(12, 6, 6))[0], _vpos(4.5, 2.5, 2.5)
    if name == "block":
        return orbit(0.6, 0.45, 0.9, _vpos(16, 16, 16))
    if name == "face":
        return orbit(0.0, 0.0, 0.8, _vpos(16, 16, 16))
    raise KeyError(name)


def _rays(orc, view, pos, W, H):
    return orc.generate_rays(view, pos, W / H, FOV, W, H).reshape(-1, 3)


def _frame(view, pos, W, H):
    return _hip().make_frame(view, pos, W / H, FOV, W, H)


def _make_fields(ctx, g, which=SOURCES):
    """Builds grid g on the context and makes the named products; returns {source: (hip FIELD_* constant, the volume)}."""
    hip = _hip()
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g, GMIN, VOX)
    out = {}
    if "distance" in which:
        out["distance"] = (hip.FIELD_DISTANCE, ctx.distance_field(hip.SET_EMPTY)[0])           # on SOLID: d2 to the nearest EMPTY voxel
    if "geodesic" in which:
        out["geodesic"] = (hip.FIELD_GEODESIC, ctx.geodesic_field([0], hip.SET_EMPTY, hip.CONN_FACE)[0])
    if "thickness" in which:
        out["thickness"] = (hip.FIELD_THICKNESS, ctx.thickness_field(hip.SET_SOLID, 4 * float(VOX))[0])
    if "skeleton" in which:
        out["skeleton"] = (hip.FIELD_SKELETON, ctx.skeleton_field(hip.SET_SOLID, hip.CONN_FULL, hip.SKEL_TOPOLOGY)[0])
    if "exposure" in which:
        out["exposure"] = (hip.FIELD_EXPOSURE, ctx.exposure_field(EXPO_DIRS, None, hip.EXPO_SKIN, REACH)[0])
    if "parts" in which:
        ctx.segment_parts(hip.SET_SOLID, hip.CONN_FACE, 1001)
        out["parts"] = (hip.FIELD_PARTS, ctx.part_labels())
    if "labels" in which:
        ctx.label_components(hip.SET_SOLID, hip.CONN_FACE)
        out["labels"] = (hip.FIELD_LABELS, ctx.component_labels())
    return out


def _same(got, want, what):
    """A frame's four results against the statement's, bit for bit."""
    rgba, values, summary, bins = got
    wr, wv, ws, wb = want
    assert np.array_equal(values, wv), f"{what}: {int((values != wv).sum())} values differ"
    assert summary.tolist() == ws.tolist(), (what, summary, ws)
    assert np.array_equal(bins, wb), what
    assert rgba.shape == wr.shape and rgba.tobytes() == wr.tobytes(), \
        f"{what}: {int((rgba.view(np.uint32) != wr.view(np.uint32)).any(-1).sum())} pixels differ"


# ================================================================ CPU
def test_field_view_structs_match_the_header():
    """ctypes rto_field_view and rto_field_view_summary are the header's: sizes, field order and offsets; constants and symbols."""
    hip = _hip()
    V, S = hip.FieldView, hip.FieldViewSummary
    assert C.sizeof(V) == 112 and C.sizeof(S) == 32 and hip.FIELD_VIEW_SUMMARY_DTYPE.itemsize == 32
    offs = {name: getattr(V, name).offset for name, _ in V._fields_}
    assert offs == {"source": 0, "sample": 4, "mode": 8, "scale": 12, "valid_lo": 16, "valid_hi": 20, "range_lo": 24, "range_hi": 28,
                    "clip": 32, "clip_lo": 36, "clip_hi": 48, "shade": 60, "miss_rgba": 64, "none_rgba": 80, "reserved": 96}
    assert {name: getattr(S, name).offset for name, _ in S._fields_} == {"hits": 0, "valued": 8, "vmin": 16, "vmax": 20, "lo": 24, "hi": 28}
    assert [hip.FIELD_VIEW_SUMMARY_DTYPE.fields[n][1] for n in ("hits", "valued", "vmin", "vmax", "lo", "hi")] == [0, 8, 16, 20, 24, 28]
    hdr = open(os.path.join(ROOT, "include", "rto_hip.h")).read()
    for struct, cls in (("rto_field_view", V), ("rto_field_view_summary", S)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in re.findall(r"(?:float|int32_t|int64_t)\s+([^;]+);", body):
            names += [re.sub(r"\[\d+\]", "", n).strip() for n in decl.split(",")]
        assert names == [n for n, _ in cls._fields_], struct
    consts = {"FIELD_DISTANCE": 0, "FIELD_GEODESIC": 1, "FIELD_THICKNESS": 2, "FIELD_SKELETON": 3, "FIELD_EXPOSURE": 4, "FIELD_PARTS": 5,
              "FIELD_LABELS": 6, "FIELD_CALLER": 7, "SAMPLE_HIT": 0, "SAMPLE_FRONT": 1, "SCALE_LINEAR": 0, "SCALE_SQRT": 1, "SCALE_CATEGORY": 2}
    for name, value in consts.items():
        assert re.search(r"#define RTO_%s\s+%d\b" % (name, value), hdr) and getattr(hip, name) == value, name
    assert hip.FIELD_PIXEL_MISS == -2 ** 31 == fr.MISS and hip.FIELD_PIXEL_NONE == -2 ** 31 + 1 == fr.NONE
    for sym in ("rto_render_field_device", "rto_render_field_host", "rto_last_field_view_ms"):
        assert sym in hip.SYMBOLS
    v = hip.make_field_view(hip.FIELD_THICKNESS)
    assert (v.valid_lo, v.valid_hi, v.range_lo, v.range_hi, v.clip, v.shade, list(v.reserved)) == (0, 0x7ffffffe, 0, 0, 0, 0, [0, 0, 0, 0])


def test_linear_and_sqrt_indices_are_the_brute_force_search():
    """On every (w, s) of small ranges, and at the ends of the int32 range: LINEAR is the largest k with k s <= 255 w, SQRT the
    largest k with k k s <= 65025 w, both found by trying every k in exact Python integers."""
    for s in (1, 2, 3, 7, 16, 100, 255, 256, 1000):
        for lo in (0, -5, 17):
            v = np.arange(lo - 2, lo + s + 3)
            lin = fr.lut_index(v, lo, lo + s, fr.LINEAR)
            sq = fr.lut_index(v, lo, lo + s, fr.SQRT)
            for i, x in enumerate(v.tolist()):
                w = min(max(x, lo), lo + s) - lo
                assert lin[i] == max(k for k in range(256) if k * s <= 255 * w), (s, lo, x)
                assert sq[i] == max(k for k in range(256) if k * k * s <= 65025 * w), (s, lo, x)
    lo, hi = -2 ** 31 + 2, 2 ** 31 - 1
    v = np.array([lo, lo + 1, -1, 0, 1, hi - 1, hi], np.int64)
    for scale, rhs in ((fr.LINEAR, 255), (fr.SQRT, 65025)):
        got = fr.lut_index(v, lo, hi, scale)
        for i, x in enumerate(v.tolist()):
            want = max(k for k in range(256) if (k * k if scale == fr.SQRT else k) * (hi - lo) <= rhs * (x - lo))
            assert got[i] == want, (scale, x)
        assert got[0] == 0 and got[-1] == 255
    assert (fr.lut_index(np.arange(5), 3, 3, fr.LINEAR) == 0).all() and (fr.lut_index(np.arange(5), 3, 3, fr.SQRT) == 0).all()
    def mix32(x):                                                   # the lit render's hash, in Python integers
        x ^= x >> 16; x = x * 0x7feb352d & 0xffffffff; x ^= x >> 15; x = x * 0x846ca68b & 0xffffffff
        return x ^ x >> 16
    cat = [0, 1, -1, 2 ** 31 - 1, -2 ** 31 + 2, 12345]
    assert fr.lut_index(np.array(cat), 5, 9, fr.CATEGORY).tolist() == [mix32(x & 0xffffffff) & 255 for x in cat]


def test_ramp_lut_is_its_formula():
    """Entry i lies between anchors j = i (n - 1) // 255 and j + 1 with weight f = i (n - 1) % 255, per channel
    (a (255 - f) + b f + 127) // 255 in integers; bytes r, g, b, a in memory order; the ends are the end anchors."""
    hip = _hip()
    for anchors in ([(0, 0, 0, 255), (255, 255, 255, 255)], [(10, 200, 30, 255), (250, 0, 90, 128), (0, 0, 255, 0)], [(7, 8, 9, 10)],
                    [(0, 0, 96, 255), (0, 200, 255, 255), (255, 255, 0, 200), (255, 32, 0, 255)]):
        lut = hip.ramp_lut(anchors)
        assert lut.dtype == np.uint32 and lut.shape == (256,)
        b = lut.view(np.uint8).reshape(256, 4)
        n = len(anchors)
        for i in range(256):
            j, f = divmod(i * (n - 1), 255)
            nxt = anchors[min(j + 1, n - 1)]
            assert b[i].tolist() == [(anchors[j][c] * (255 - f) + nxt[c] * f + 127) // 255 for c in range(4)], (anchors, i)
        assert b[0].tolist() == list(anchors[0]) and b[255].tolist() == list(anchors[-1])
        assert int(lut[0]) == anchors[0][0] | anchors[0][1] << 8 | anchors[0][2] << 16 | anchors[0][3] << 24
    assert np.array_equal(fr.lut_colours(hip.ramp_lut([(0, 51, 102, 255), (0, 51, 102, 255)]))[7],
                          np.float32([0, 51, 102, 255]) / np.float32(255))


def test_statement_without_a_clip_box_hits_the_oracle_frame(orc, scenes):
    """field_view_ref on sphere32, FIRST, no clip: its miss mask is the oracle frame's; on every pixel whose leaf is one voxel the
    value is the volume's at that leaf; a whole-grid clip box changes nothing; the Lambert term is the oracle's."""
    hip = _hip()
    s = scenes("sphere32")
    T = q.Tree32(s.nodes, s.min, s.voxel)
    view, pos = make_camera(orc, *SPHERE_CAM)
    W, H = 48, 36
    rd = _rays(orc, view, pos, W, H)
    dz, dy, dx = s.grid.data.shape
    vol = np.arange(dz * dy * dx, dtype=np.int32).reshape(dz, dy, dx)
    v = hip.make_field_view(hip.FIELD_CALLER, shade=True, range=(0, dz * dy * dx - 1))
    lut = hip.ramp_lut([(255, 255, 255, 255), (255, 255, 255, 255)])
    rgba, values, summary, bins = fr.frame(T, s.min, s.voxel, pos, rd, W, H, vol, v, lut)
    want, _ = orc.render(s.nodes, s.min, s.voxel, view, pos, W / H, FOV, W, H)
    want = want.reshape(H, W, 4)
    assert ((values == fr.MISS) == (want[..., 0] < 0.05)).all() and summary["hits"] == (want[..., 0] > 0.05).sum() > 100
    hits = q.query32(T, pos, rd)[q.FIRST].reshape(H, W)
    one = (hits["node"] >= 0) & (hits["size"] == 1)
    assert one.sum() > 100 and (values[one] == vol[hits["z"][one], hits["y"][one], hits["x"][one]]).all()
    # white LUT, shaded: r = 0.25 + 0.75 ndotl, and the oracle's red channel is ndotl + 0.1
    hit = values != fr.MISS
    nd = ((rgba[..., 0][hit] - np.float32(0.25)) / np.float32(0.75)).astype(np.float32)
    assert np.abs(nd - (want[..., 0][hit] - np.float32(0.1))).max() < 1e-6
    whole = hip.make_field_view(hip.FIELD_CALLER, shade=True, range=(0, dz * dy * dx - 1), clip=((0, 0, 0), (dx, dy, dz)))
    again = fr.frame(T, s.min, s.voxel, pos, rd, W, H, vol, whole, lut)
    assert again[0].tobytes() == rgba.tobytes() and np.array_equal(again[1], values) and np.array_equal(again[3], bins)
    assert bins.sum() == summary["valued"]


def test_field_view_kernels_keep_their_budgets():
    """The built metadata (the product's flags): the three k_field_* kernels without scratch or spills, within k_lit_primary's 80
    VGPRs; the sample kernels no larger than one allocation granule (8) above k_lit_primary itself, so its occupancy is kept."""
    import test_isa_contract as isa
    asm = isa.built_asm()
    if asm is None:
        pytest.skip("no hipcc in this environment")
    meta = isa.kernel_meta(asm)
    names = [k for k in meta if "k_field_" in k]
    assert len(names) == 3 and len([k for k in names if "k_field_sample" in k]) == 2, names
    lit = meta[isa.find(meta, "13k_lit_primary")[0]]["vgpr"]
    waves = lambda vgpr: 512 // ((vgpr + 7) // 8 * 8)                # waves per SIMD the register file admits
    for k in names:
        m = meta[k]
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, (k, m)
        assert m["vgpr"] <= VGPR_BUDGET, (k, m)
        if "k_field_sample" in k:
            assert waves(m["vgpr"]) >= waves(lit), (k, m, lit)


# ================================================================ GPU
# (grid, camera, W, H, source, make_field_view's keywords)
CASES = [
    ("base", "outside", 24, 16, "geodesic", dict(sample=1)),
    ("base", "outside", 24, 16, "thickness", dict(mode=1, shade=True, scale=1)),
    ("base", "outside", 24, 16, "parts", dict(scale=2, shade=True)),
    ("base", "outside", 24, 16, "distance", dict(scale=1, clip=((0, 0, 0), (12, 12, 12)))),
    ("base", "outside@0.2", 13, 9, "skeleton", dict(mode=1, clip=((0, 0, 0), (12, 12, 12)))),
    ("base", "low", 24, 16, "exposure", dict(sample=1, shade=True)),
    ("base", "axis@0.25", 13, 9, "geodesic", dict(sample=1, mode=1)),
    ("base", "axis", 24, 16, "labels", dict(range=(0, 1))),
    ("base", "axis@0.25", 72, 8, "geodesic", dict(sample=1, shade=True, range=(10, 40))),
    ("base", "axis@0.25", 8, 8, "thickness", dict(scale=1)),
    ("base", "inside", 24, 16, "distance", dict()),
    ("base", "inside", 13, 9, "distance", dict(shade=True, scale=1)),
    ("base", "inside", 24, 16, "thickness", dict(sample=1, mode=0)),
    ("base", "outside", 1, 1, "thickness", dict(shade=True)),
    ("block32", "block", 24, 16, "thickness", dict(shade=True)),
    ("block32", "block@0.6", 13, 9, "geodesic", dict(sample=1, mode=1)),
]


def _case_view(hip, code, kw):
    return hip.make_field_view(code, none_rgba=(0.5, 0.25, 0.125, 0.75), miss_rgba=(0.0, 0.125, 0.25, 1.0), **kw)


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c[:5]) + "".join("-%s" % k for k in c[5]))
def test_gpu_frames_equal_the_statement(ctx, orc, case):
    """values, rgba, summary and bins of a frame, bit for bit against field_view_ref on the same volume.  Every source, HIT and
    FRONT, FIRST and CLOSEST, shaded and not, the three scales; frames of partial tiles, one pixel, one tile and nine tiles;
    cameras outside, on the axes and inside a solid leaf.  The statement's own frame is first shown not to be degenerate: at
    least 20 valued pixels and two LUT indices (a frame of one pixel: that pixel is valued)."""
    hip = _hip()
    gname, cam, W, H, source, kw = case
    g, nodes, T = _tree(orc, gname)
    view, pos = _camera(orc, cam)
    code, vol = _make_fields(ctx, g, (source,))[source]
    v = _case_view(hip, code, kw)
    rd = _rays(orc, view, pos, W, H)
    want = fr.frame(T, GMIN, VOX, pos, rd, W, H, vol, v, _lut())
    if W * H == 1:
        assert want[2]["valued"] == 1
    else:
        assert not fr.degenerate(want[1], v), (case, want[2])
    if cam == "inside":
        hits = q.query32(T, pos, rd)[v.mode]
        assert (hits["face"][hits["node"] >= 0] == -1).sum() >= 20
    if cam.startswith("axis") and W % 2:
        assert (rd == 0).sum(1).max() == 2
    _same(ctx.render_field_host(_frame(view, pos, W, H), v, _lut()), want, str(case))


@gpu
def test_gpu_values_are_the_field_at_the_query_record(ctx, orc, scenes):
    """Without the new statement: sphere64 at 256 x 144, distance to EMPTY, HIT.  Under FIRST and under CLOSEST every pixel whose
    rto_query_pixels record (same mode) is a one-voxel leaf holds field[z, y, x] of that record; the miss mask under FIRST is
    rto_render_lit_host's vis == -1."""
    hip = _hip()
    s = scenes("sphere64")
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(s.grid.data, s.min, s.voxel)
    field = ctx.distance_field(hip.SET_EMPTY)[0]
    view, pos = make_camera(orc, *SPHERE_CAM)
    W, H = 256, 144
    f = hip.make_frame(view, pos, W / H, FOV, W, H)
    yy, xx = np.mgrid[0:H, 0:W]
    xy = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.int32)
    for mode in (hip.QUERY_FIRST, hip.QUERY_CLOSEST):
        rgba, values, summary, bins = ctx.render_field_host(f, hip.make_field_view(hip.FIELD_DISTANCE, mode=mode, scale=hip.SCALE_SQRT), _lut())
        rec = ctx.query_pixels(f, xy, mode).reshape(H, W)
        assert ((values == hip.FIELD_PIXEL_MISS) == (rec["node"] < 0)).all()
        one = (rec["node"] >= 0) & (rec["size"] == 1)
        assert one.sum() > 1000
        assert (values[one] == field[rec["z"][one], rec["y"][one], rec["x"][one]]).all()
        assert summary["hits"] == (rec["node"] >= 0).sum() and bins.sum() == summary["valued"]
        if mode == hip.QUERY_FIRST:
            _, vis = ctx.render_lit_host(f, vis=True, shadow=False, ao_samples=0)
            assert ((values == hip.FIELD_PIXEL_MISS) == (vis == -1)).all()


@gpu
def test_gpu_front_samples_the_voxel_in_front_of_the_surface(ctx, orc):
    """An exposure SKIN field lives on the EMPTY voxels that touch the solid: under FRONT every valued pixel is the field at the
    record's neighbour voxel (one-voxel leaves, by rto_query_pixels), and HIT sees no value at all.  A solid flush with the grid's
    +z face, seen head-on: its neighbours lie outside the grid, so its pixels are NONE."""
    hip = _hip()
    g, nodes, T = _tree(orc, "base")
    code, field = _make_fields(ctx, g, ("exposure",))["exposure"]
    W, H = 40, 24
    yy, xx = np.mgrid[0:H, 0:W]
    xy = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.int32)
    seen, sizes = set(), set()
    for cam in ("axis", "low"):
        view, pos = _camera(orc, cam)
        f = _frame(view, pos, W, H)
        rgba, values, summary, bins = ctx.render_field_host(f, hip.make_field_view(code, sample=hip.SAMPLE_FRONT), _lut())
        rec = ctx.query_pixels(f, xy, hip.QUERY_FIRST).reshape(H, W)
        valued = (values != hip.FIELD_PIXEL_MISS) & (values != hip.FIELD_PIXEL_NONE)
        assert valued.sum() >= 20 and summary["valued"] == valued.sum()
        assert (rec["face"][valued] >= 0).all()
        # the voxel of the hit in float64 from the record's t, on pixels whose hit point is clear of every voxel boundary; the
        # face's axis is the leaf's own boundary voxel, moved one out
        rd = _rays(orc, view, pos, W, H).reshape(H, W, 3).astype(np.float64)
        t = np.where(rec["node"] >= 0, rec["t"], 0).astype(np.float64)
        p = (pos.astype(np.float64) + rd * t[..., None] - GMIN.astype(np.float64)) / float(VOX)
        clear = np.abs(p - np.round(p)) > 1e-3
        face = rec["face"]
        clear[np.arange(H)[:, None], np.arange(W)[None, :], np.where(face >= 0, face >> 1, 0)] = True
        sure = valued & clear.all(-1)
        assert sure.sum() >= 20 and sure.sum() > 0.8 * valued.sum(), cam
        lo = np.stack([rec["x"], rec["y"], rec["z"]], -1)
        vox = np.clip(np.floor(p).astype(np.int64), lo, lo + rec["size"][..., None] - 1)[sure]
        fs, sz, los = face[sure], rec["size"][sure], lo[sure]
        rows = np.arange(len(vox))
        vox[rows, fs >> 1] = np.where(fs & 1, los[rows, fs >> 1] + sz, los[rows, fs >> 1] - 1)
        assert (values[sure] == field[vox[:, 2], vox[:, 1], vox[:, 0]]).all(), cam
        sizes |= set(rec["size"][sure].tolist())
        seen |= set(values[sure].tolist())
    assert len(seen) >= 3 and len(sizes) >= 2, (seen, sizes)
    hit_only = ctx.render_field_host(f, hip.make_field_view(code), _lut())
    assert hit_only[2]["valued"] == 0 and hit_only[2]["hits"] == summary["hits"] > 0
    assert (hit_only[0][hit_only[1] == hip.FIELD_PIXEL_NONE] == np.float32([0.25, 0.25, 0.25, 1.0])).all()
    # flush with the +z face of an 8^3 grid, seen along -z
    flush = np.zeros((8, 8, 8), np.uint8)
    flush[6:8, 2:6, 2:6] = 1
    ctx.build_octree(flush, GMIN, VOX)
    vol = np.arange(512, dtype=np.int32).reshape(8, 8, 8)
    cam = orc.Camera(0.0, 0.0, 0.2)
    cam.set_target(*[float(x) for x in _vpos(4, 4, 4)])
    fview, fpos = cam.get_view(), cam.get_pos()
    assert fpos[2] > _vpos(0, 0, 8)[2]                           # the camera looks at the +z face from outside
    ff = _frame(fview, fpos, 24, 16)
    v = hip.make_field_view(hip.FIELD_CALLER, sample=hip.SAMPLE_FRONT)
    got = ctx.render_field_host(ff, v, _lut(), vol)
    T8 = q.Tree32(orc.build_flat_octree(orc.Grid((8, 8, 8), GMIN, VOX, flush)), GMIN, VOX)
    want = fr.frame(T8, GMIN, VOX, fpos, _rays(orc, fview, fpos, 24, 16), 24, 16, vol, v, _lut())
    assert (want[1] == fr.NONE).sum() >= 8 and want[2]["hits"] > want[2]["valued"]
    _same(got, want, "flush with the grid face")
    assert (got[1] == hip.FIELD_PIXEL_NONE).sum() == (want[1] == fr.NONE).sum()


@gpu
def test_gpu_clip_boxes(ctx, orc):
    """The 16^3 block cut through its middle shows distance to EMPTY: the statement's cut pixels carry values > 1 and the GPU
    equals it; a clip plane at offset 3 inside a leaf of 8; a whole-grid clip box is the frame without one, bit for bit; a clip
    box no ray meets gives a frame of miss_rgba."""
    hip = _hip()
    g, nodes, T = _tree(orc, "block32")
    code, vol = _make_fields(ctx, g, ("distance",))["distance"]
    view, pos = _camera(orc, "block@0.6")
    W, H = 24, 16
    f = _frame(view, pos, W, H)
    rd = _rays(orc, view, pos, W, H)
    high = [int(x) for x in ((pos - GMIN) / VOX > 16)]           # the side of the block the camera is on, per axis
    cuts = {"middle": 16, "offset 3 in a leaf of 8": 11 if high[0] else 21}
    for name, x in cuts.items():
        clip = ((0, 0, 0), (x, 32, 32)) if high[0] else ((x, 0, 0), (32, 32, 32))
        v = hip.make_field_view(code, scale=hip.SCALE_SQRT, shade=True, clip=clip)
        want = fr.frame(T, GMIN, VOX, pos, rd, W, H, vol, v, _lut())
        assert (want[1] > 1).sum() >= 10 and not fr.degenerate(want[1], v), (name, want[2])
        hits = q.query32(T, pos, rd)[q.FIRST]
        assert (hits["size"] == 8).any()
        _same(ctx.render_field_host(f, v, _lut()), want, name)
    plain = ctx.render_field_host(f, hip.make_field_view(code, shade=True), _lut())
    whole = ctx.render_field_host(f, hip.make_field_view(code, shade=True, clip=((0, 0, 0), (32, 32, 32))), _lut())
    assert plain[2]["valued"] >= 20
    _same(whole, plain, "a whole-grid clip box")
    away = ((0, 0, 0), (2, 2, 2)) if high[0] else ((30, 30, 30), (32, 32, 32))      # the grid corner behind the block
    v = hip.make_field_view(code, clip=away, miss_rgba=(0.125, 0.5, 0.75, 0.25))
    want = fr.frame(T, GMIN, VOX, pos, rd, W, H, vol, v, _lut())
    assert (want[1] == fr.MISS).all()
    got = ctx.render_field_host(f, v, _lut())
    _same(got, want, "a clip box the rays miss")
    assert (got[0] == np.float32([0.125, 0.5, 0.75, 0.25])).all() and got[2].tolist() == (0, 0, 0, 0, 0, 0) and got[3].sum() == 0


@gpu
def test_gpu_auto_range_and_the_device_form(ctx, orc):
    """Auto range is the frame of the explicit range (vmin, vmax), bit for bit; the device form on a caller's stream (with and
    without the optional outputs) is the host form; the bins sum to `valued`; the kernels' times are reported."""
    torch = pytest.importorskip("torch")
    hip = _hip()
    g, nodes, T = _tree(orc, "base")
    code, vol = _make_fields(ctx, g, ("geodesic",))["geodesic"]
    view, pos = _camera(orc, "outside")
    W, H = 72, 40
    f = _frame(view, pos, W, H)
    auto = ctx.render_field_host(f, hip.make_field_view(code, sample=1, shade=True), _lut())
    s = auto[2]
    assert s["valued"] >= 20 and s["vmin"] < s["vmax"] and (s["lo"], s["hi"]) == (s["vmin"], s["vmax"])
    explicit = ctx.render_field_host(f, hip.make_field_view(code, sample=1, shade=True, range=(int(s["vmin"]), int(s["vmax"]))), _lut())
    _same(explicit, auto, "explicit (vmin, vmax)")
    assert auto[3].sum() == s["valued"] and (auto[3] > 0).sum() >= 2
    ms = ctx.last_field_view_ms()
    assert len(ms) == 2 and ms[0] > 0 and ms[1] > 0
    other = torch.cuda.Stream()
    d_lut = torch.from_numpy(_lut().view(np.int32)).cuda()
    d_rgba = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
    d_values = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    d_summary = torch.zeros(4, dtype=torch.int64, device="cuda")
    d_bins = torch.full((256,), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    v = hip.make_field_view(code, sample=1, shade=True)
    ctx.render_field_device(f, v, d_lut.data_ptr(), d_rgba.data_ptr(), 0, d_values.data_ptr(), d_summary.data_ptr(), d_bins.data_ptr(),
                            other.cuda_stream)
    other.synchronize()
    assert d_rgba.cpu().numpy().tobytes() == auto[0].tobytes() and d_values.cpu().numpy().tobytes() == auto[1].tobytes()
    assert d_summary.cpu().numpy().view(hip.FIELD_VIEW_SUMMARY_DTYPE)[0].tolist() == s.tolist()
    assert np.array_equal(d_bins.cpu().numpy(), auto[3])
    d_rgba.zero_()
    torch.cuda.synchronize()
    ctx.render_field_device(f, v, d_lut.data_ptr(), d_rgba.data_ptr(), stream=other.cuda_stream)      # the context's own value buffer
    other.synchronize()
    assert d_rgba.cpu().numpy().tobytes() == auto[0].tobytes()
    # a caller's volume on the device
    d_vol = torch.from_numpy(vol).cuda()
    torch.cuda.synchronize()
    ctx.render_field_device(f, hip.make_field_view(hip.FIELD_CALLER, sample=1, shade=True), d_lut.data_ptr(), d_rgba.data_ptr(),
                            d_vol.data_ptr(), stream=other.cuda_stream)
    other.synchronize()
    assert d_rgba.cpu().numpy().tobytes() == auto[0].tobytes()


ADVERSARIAL = np.array([0, 1, 0x7ffffffe, -1, -7, -2 ** 31 + 2, 0x7fffffff, 2, 1000, -2 ** 30], np.int64)


@gpu
@pytest.mark.parametrize("scale", [0, 1, 2], ids=["linear", "sqrt", "category"])
def test_gpu_caller_volumes_with_adversarial_values(ctx, orc, scale):
    """A caller's volume of 0, 1, 0x7ffffffe, negatives, INT32_MIN + 2 and INT32_MAX, one per voxel in turn, through each scale:
    with valid_lo = INT32_MIN + 2 and the widest range s = hi - lo needs 33 bits and w * 65025 needs 48: nothing wraps.  Auto
    range, the widest explicit range, a narrow one that clamps, and the default validity (which drops the negatives and
    INT32_MAX) all equal the statement."""
    hip = _hip()
    g, nodes, T = _tree(orc, "base")
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g, GMIN, VOX)
    idx = np.arange(g.size).reshape(g.shape)
    vol = ADVERSARIAL[(idx * 7 + idx // 40) % len(ADVERSARIAL)].astype(np.int32)
    view, pos = _camera(orc, "outside")
    W, H = 24, 16
    f = _frame(view, pos, W, H)
    rd = _rays(orc, view, pos, W, H)
    lo, hi = -2 ** 31 + 2, 2 ** 31 - 1
    for kw in (dict(valid=(lo, hi)), dict(valid=(lo, hi), range=(lo, hi)), dict(valid=(lo, hi), range=(-7, 1000)),
               dict(valid=(lo, 0x7ffffffe), range=(lo, 0x7ffffffe)), dict()):
        v = hip.make_field_view(hip.FIELD_CALLER, scale=scale, **kw)
        want = fr.frame(T, GMIN, VOX, pos, rd, W, H, vol, v, _lut())
        assert not fr.degenerate(want[1], v), (kw, want[2])
        if "valid" in kw:
            assert (want[2]["vmin"], want[2]["vmax"]) == (lo, kw["valid"][1])
            assert (want[2]["valued"] == want[2]["hits"]) == (kw["valid"][1] == hi)        # only INT32_MAX can fall outside
        else:
            assert 0 < want[2]["valued"] < want[2]["hits"] and want[2]["vmin"] == 0
        _same(ctx.render_field_host(f, v, _lut(), vol), want, f"{scale} {kw}")


@gpu
def test_gpu_an_edit_drops_the_named_sources_and_keeps_the_caller(ctx, orc):
    """After an rto_edit_voxels with changed > 0 every named source is refused in its readers' words and nothing else on the
    context moved (the next CALLER frame is the statement on the edited tree; the voxels are the edited grid); making a field
    again renders again."""
    hip = _hip()
    g, nodes, T = _tree(orc, "base")
    fields = _make_fields(ctx, g)
    view, pos = _camera(orc, "outside")
    W, H = 24, 16
    f = _frame(view, pos, W, H)
    rd = _rays(orc, view, pos, W, H)
    before = ctx.render_field_host(f, hip.make_field_view(hip.FIELD_THICKNESS), _lut())
    brush = hip.make_brushes([GMIN + np.float32(0.5) * VOX], 0.5 * float(VOX), hip.BRUSH_SPHERE, hip.EDIT_FILL)
    assert ctx.edit_voxels(brush) > 0
    edited = g.copy()
    edited[0, 0, 0] = 1
    for name, (code, _) in fields.items():
        with pytest.raises(hip.RtoError) as e:
            ctx.render_field_host(f, hip.make_field_view(code), _lut())
        assert e.value.code == hip.RTO_E_INVALID and "the grid has changed since" in str(e.value), (name, str(e.value))
    assert np.array_equal(ctx.download_voxels(), edited)
    vol = np.arange(g.size, dtype=np.int32).reshape(g.shape)
    v = hip.make_field_view(hip.FIELD_CALLER, scale=hip.SCALE_CATEGORY)
    T2 = q.Tree32(ctx.download_nodes(), GMIN, VOX)
    _same(ctx.render_field_host(f, v, _lut(), vol), fr.frame(T2, GMIN, VOX, pos, rd, W, H, vol, v, _lut()), "CALLER after the edit")
    ctx.thickness_field(hip.SET_SOLID, 4 * float(VOX))
    after = ctx.render_field_host(f, hip.make_field_view(hip.FIELD_THICKNESS), _lut())
    assert after[2]["valued"] >= 20
    _same(after, fr.frame(T2, GMIN, VOX, pos, rd, W, H, ctx.thickness(), hip.make_field_view(hip.FIELD_THICKNESS), _lut()), "made again")
    assert after[2]["hits"] >= before[2]["hits"]


@gpu
def test_gpu_error_codes_in_the_header_s_order(ctx, orc, scenes):
    """Every refusal of the header.  Each call below is wrong in the way named and also in every way checked later, so the code
    and text it answers show the order: NULLs, alignment, source, sample, mode, scale, reserved, valid, range, frame size, frame
    limits, the volume's presence, (fresh context) no octree, no grid, non-canonical, the clip box, the source's residency.  A
    refused call leaves the next frame unchanged."""
    torch = pytest.importorskip("torch")
    hip = _hip()
    g, nodes, T = _tree(orc, "base")
    code, vol = _make_fields(ctx, g, ("thickness",))["thickness"]
    view, pos = _camera(orc, "outside")
    W, H = 24, 16
    f = _frame(view, pos, W, H)
    lut = _lut()
    ref = ctx.render_field_host(f, hip.make_field_view(code), lut)
    Lib = ctx._L
    out = np.zeros((H, W, 4), np.float32)

    def call(view_, frame=f, lut_=lut, buf=out, volume=None, c=ctx):
        rc = Lib.rto_render_field_host(c._h, C.byref(frame) if frame is not None else None, C.byref(view_) if view_ is not None else None,
                                       lut_.ctypes.data if lut_ is not None else None, volume.ctypes.data if volume is not None else None,
                                       buf.ctypes.data if buf is not None else None, None, None, None)
        return rc, Lib.rto_last_error(c._h).decode()

    def worst():
        """A view wrong in every way a view can be, on a source that is not resident."""
        v = hip.make_field_view(hip.FIELD_GEODESIC, sample=5, mode=hip.QUERY_ANY, scale=9, valid=(3, 2), range=(5, 1),
                                clip=((0, 0, 0), (41, 12, 12)))
        v.reserved[2] = 1
        return v

    big = hip.make_frame(view, pos, 1.0, FOV, 65536, 65536)
    flat = hip.make_frame(view, pos, 1.0, FOV, 0, 16)
    assert call(hip.make_field_view(code))[0] == hip.RTO_OK
    for kw in (dict(frame=None), dict(lut_=None), dict(buf=None)):
        rc, msg = call(worst(), volume=vol, **kw)
        assert rc == hip.RTO_E_INVALID and "NULL" in msg, kw
    assert call(None)[0] == hip.RTO_E_INVALID
    # the view's own fields, each fixed in turn; the frame stays too large and the volume unwanted until their turn comes
    v = worst()
    steps = [("source", lambda: setattr(v, "source", 8), "unknown source"), ("source", lambda: setattr(v, "source", -1), "unknown source"),
             ("sample", lambda: setattr(v, "source", hip.FIELD_GEODESIC), "unknown sample"),
             ("mode", lambda: setattr(v, "sample", 1), "mode must be"), ("scale", lambda: setattr(v, "mode", 1), "unknown scale"),
             ("reserved", lambda: setattr(v, "scale", 2), "reserved"), ("valid", lambda: v.reserved.__setitem__(2, 0), "valid_lo"),
             ("valid", lambda: (setattr(v, "valid_lo", -2 ** 31 + 1), setattr(v, "valid_hi", 5)), "valid_lo"),
             ("range", lambda: setattr(v, "valid_lo", -2 ** 31 + 2), "range_lo > range_hi")]
    for what, fix, text in steps:
        fix()
        rc, msg = call(v, frame=big, volume=vol)
        assert rc == hip.RTO_E_INVALID and text in msg, (what, msg)
    v.range_lo = 1
    rc, msg = call(v, frame=flat, volume=vol)
    assert rc == hip.RTO_E_INVALID and "width/height" in msg
    rc, msg = call(v, frame=big, volume=vol)
    assert rc == hip.RTO_E_INVALID and "too large" in msg
    rc, msg = call(v, volume=vol)
    assert rc == hip.RTO_E_INVALID and "RTO_FIELD_CALLER only" in msg
    v.source = hip.FIELD_CALLER
    rc, msg = call(v)
    assert rc == hip.RTO_E_INVALID and "needs a volume" in msg
    # the context's state: nothing uploaded, no grid, a non-canonical array -- each in front of the clip box and the residency
    fresh = hip.Context(0)
    try:
        v.source = hip.FIELD_GEODESIC
        assert call(v, c=fresh)[0] == hip.RTO_E_NO_OCTREE
        s = scenes("sphere16")
        fresh.upload_octree(s.nodes, GMIN, VOX)
        rc, msg = call(v, c=fresh)
        assert rc == hip.RTO_E_UNSUPPORTED and "no voxel grid is resident" in msg
        perm = s.nodes.copy()
        n = len(perm)
        p = np.concatenate([[0], 1 + np.random.default_rng(5).permutation(n - 1)])
        moved = np.zeros_like(perm)
        moved[p] = perm
        moved["child"] = np.where(moved["child"] >= 0, p[np.maximum(moved["child"], 0)], -1)
        fresh.upload_octree(moved, GMIN, VOX)
        assert fresh.info().canonical == 0
        assert call(v, c=fresh)[0] == hip.RTO_E_UNSUPPORTED
    finally:
        fresh.close()
    rc, msg = call(v)
    assert rc == hip.RTO_E_INVALID and "clip box" in msg                      # clip_hi[0] = 41 > 40, on a source that is not resident
    for lo_, hi_ in (((-1, 0, 0), (40, 12, 12)), ((5, 0, 0), (5, 12, 12)), ((0, 0, 7), (40, 12, 6)), ((0, 0, 0), (40, 13, 12))):
        for a in range(3):
            v.clip_lo[a], v.clip_hi[a] = lo_[a], hi_[a]
        rc, msg = call(v)
        assert rc == hip.RTO_E_INVALID and "clip box" in msg, (lo_, hi_)
    for a, d in enumerate((40, 12, 12)):
        v.clip_lo[a], v.clip_hi[a] = 0, d
    rc, msg = call(v)
    assert rc == hip.RTO_E_INVALID and "no geodesic field is resident" in msg and "the grid has changed since" in msg
    v.source = hip.FIELD_LABELS
    rc, msg = call(v)
    assert rc == hip.RTO_E_INVALID and "no labels are resident" in msg and "the grid has changed since" in msg
    v.source = code
    assert call(v)[0] == hip.RTO_OK
    # the device form's alignment, behind the NULLs and in front of everything else
    dev = Lib.rto_render_field_device
    d = torch.zeros(W * H * 4 + 64, dtype=torch.float32, device="cuda")
    d_lut = torch.from_numpy(lut.view(np.int32)).cuda()
    p0 = d.data_ptr()
    P = lambda x: C.c_void_p(x) if x else None

    def devcall(view_, lut_=d_lut.data_ptr(), volume=0, rgba=p0, values=0, summary=0, bins=0):
        return dev(ctx._h, C.byref(f), C.byref(view_), P(lut_), P(volume), P(rgba), P(values), P(summary), P(bins), None), \
            Lib.rto_last_error(ctx._h).decode()

    bad = worst()
    for kw in (dict(rgba=p0 + 4), dict(lut_=p0 + 2), dict(volume=p0 + 2), dict(values=p0 + 2), dict(summary=p0 + 4), dict(bins=p0 + 4)):
        rc, msg = devcall(bad, **kw)
        assert rc == hip.RTO_E_INVALID and "aligned" in msg, kw
    rc, msg = devcall(bad, rgba=0)
    assert rc == hip.RTO_E_INVALID and "NULL" in msg
    rc, msg = devcall(bad)
    assert rc == hip.RTO_E_INVALID and "unknown sample" in msg
    torch.cuda.synchronize()
    _same(ctx.render_field_host(f, hip.make_field_view(code), lut), ref, "after the refusals")


@gpu
def test_gpu_a_tree_that_is_one_leaf(ctx, orc):
    """An all-solid 8^3 grid builds a tree of one node (no descriptors): frames from outside and from inside, HIT and FRONT,
    FIRST and CLOSEST, with a clip box that cuts the leaf, equal the statement."""
    hip = _hip()
    full = np.ones((8, 8, 8), np.uint8)
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(full, GMIN, VOX)
    assert ctx.info().num_nodes == 1
    nodes = orc.build_flat_octree(orc.Grid((8, 8, 8), GMIN, VOX, full))
    assert len(nodes) == 1
    T = q.Tree32(nodes, GMIN, VOX)
    vol = (np.arange(512, dtype=np.int32).reshape(8, 8, 8) * 37) % 101
    cam = orc.Camera(0.6, 0.45, 0.4)
    cam.set_target(*[float(x) for x in _vpos(4, 4, 4)])
    view, out_pos = cam.get_view(), cam.get_pos()
    W, H = 24, 16
    valued = 0
    for pos in (out_pos, _vpos(2.3, 5.1, 3.7)):
        f = _frame(view, pos, W, H)
        rd = _rays(orc, view, pos, W, H)
        for kw in (dict(), dict(mode=1, shade=True), dict(sample=1), dict(clip=((0, 0, 0), (8, 8, 5)), shade=True),
                   dict(mode=1, clip=((3, 0, 0), (8, 6, 8)), scale=2)):
            v = hip.make_field_view(hip.FIELD_CALLER, **kw)
            want = fr.frame(T, GMIN, VOX, pos, rd, W, H, vol, v, _lut())
            _same(ctx.render_field_host(f, v, _lut(), vol), want, f"{pos} {kw}")
            valued += int(want[2]["valued"])
            if pos is out_pos and not kw:
                assert not fr.degenerate(want[1], v)
    assert valued > 200


@gpu
def test_gpu_full_size_frame(ctx, orc, scenes):
    """sphere256 at 1920 x 1080, thickness, FIRST: the statement on a seeded sample of 2,048 pixels (values, and colours under the
    frame's own range); on the whole frame every one-voxel record of rto_query_pixels holds the field's value and the miss mask
    is the lit render's."""
    hip = _hip()
    s = scenes("sphere256")
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(s.grid.data, s.min, s.voxel)
    field = ctx.thickness_field(hip.SET_SOLID, 4 * float(s.voxel))[0]
    view, pos = make_camera(orc, *SPHERE_CAM)
    W, H = 1920, 1080
    f = hip.make_frame(view, pos, W / H, FOV, W, H)
    v = hip.make_field_view(hip.FIELD_THICKNESS, shade=True, scale=hip.SCALE_SQRT)
    rgba, values, summary, bins = ctx.render_field_host(f, v, _lut())
    assert bins.sum() == summary["valued"] > 100000
    yy, xx = np.mgrid[0:H, 0:W]
    xy = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.int32)
    rec = ctx.query_pixels(f, xy, hip.QUERY_FIRST).reshape(H, W)
    assert ((values == hip.FIELD_PIXEL_MISS) == (rec["node"] < 0)).all()
    one = (rec["node"] >= 0) & (rec["size"] == 1)
    assert one.sum() > 100000 and (values[one] == field[rec["z"][one], rec["y"][one], rec["x"][one]]).all()
    _, vis = ctx.render_lit_host(f, vis=True, shadow=False, ao_samples=0)
    assert ((values == hip.FIELD_PIXEL_MISS) == (vis == -1)).all()
    # the statement on a sample: the rays of the sampled pixels, the frame's range
    rng = np.random.default_rng(11)
    hitpix = np.flatnonzero(values.ravel() != hip.FIELD_PIXEL_MISS)
    pick = np.concatenate([rng.choice(hitpix, 1536, replace=False), rng.choice(W * H, 512, replace=False)])
    rd = _rays(orc, view, pos, W, H)[pick]
    T = q.Tree32(s.nodes, s.min, s.voxel)
    wv, nd, _ = fr.sample(T, s.min, s.voxel, pos, rd, field, v)
    assert np.array_equal(values.ravel()[pick], wv)
    fixed = hip.make_field_view(hip.FIELD_THICKNESS, shade=True, scale=hip.SCALE_SQRT, range=(int(summary["lo"]), int(summary["hi"])))
    assert summary["lo"] < summary["hi"]
    wr, _, _ = fr.colour(wv, nd, fixed, _lut())
    assert rgba.reshape(-1, 4)[pick].tobytes() == wr.tobytes()


@gpu
def test_gpu_drop_in_render_field(orc):
    """RayTracerBVH::renderField through host.py: framebuffer(), fieldValues() and fieldSummary() are the C ABI's frame."""
    import ray_tracing_octrees_amd as rto
    hip = _hip()
    grid = rto.VoxelGrid.test_sphere(32)
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    rt.setOctreeFromGrid(grid)
    cam = rto.Camera(*SPHERE_CAM)
    W, H = 96, 72
    v = hip.make_field_view(hip.FIELD_DISTANCE, scale=hip.SCALE_SQRT, shade=True, mode=hip.QUERY_CLOSEST)
    assert rt.renderField(cam, W, H, W / H, FOV, v, _lut()) == hip.RTO_E_INVALID and "the grid has changed since" in rt.lastError
    assert rt.distanceField(hip.SET_EMPTY)[0] == hip.RTO_OK
    assert rt.renderField(cam, W, H, W / H, FOV, v, _lut()) == hip.RTO_OK
    img, values, summary = rt.framebuffer(), rt.fieldValues(), rt.fieldSummary()
    assert img.shape == (H, W, 4) and values.shape == (H, W)
    og = orc.test_sphere_grid(32)
    ctx = rto.Context(0)
    try:
        ctx.build_octree(og.data, og.min, og.voxel_size)
        ctx.distance_field(hip.SET_EMPTY)
        f = rto.make_frame(cam.getView(), cam.getPos(), W / H, FOV, W, H)
        want = ctx.render_field_host(f, v, _lut())
    finally:
        ctx.close()
    assert want[2]["valued"] > 500
    assert img.tobytes() == want[0].tobytes() and np.array_equal(values, want[1]) and summary.tolist() == want[2].tolist()
