"""Field compositing (rto_composite_field_*, Context.composite_field_*, RayTracerBVH::compositeField): a resident int32 volume
seen through, LUT colour and opacity composited front to back along the pixel rays of tests/test_projection.py's walk.  CPU: the
ABI's layout; the statement (tests/composite_ref.py) against the host form; the kernel's thresholds against the field views' index;
the rule's two consequences and its invariants on the statement; the frames' conditions; the kernels' register figures.  GPU: every
output against the statement, bit for bit and with no pixel excluded, with the tables and without; the cross-checks against the
projections; the device form; the lifecycle; a frustum update in force; every refusal; the solid table's launch shapes; the
drop-in class.

Grids, frames and cameras are test_projection.py's."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import composite_ref as cr
import distance_ref as dr
import field_view_ref as fr
import geodesic_ref as gr
import projection_ref as pr
import test_projection as tp
from conftest import SPHERE_CAM

gpu = pytest.mark.gpu
ROOT = tp.ROOT
FOV = tp.FOV
GMIN, VOX = tp.GMIN, tp.VOX
MARCH_VGPRS, SOLID_VGPRS = 64, 64        # 8 waves per SIMD for both
WIDE = (-2 ** 31 + 2, 2 ** 31 - 1)
BG, MISS = (0.25, 0.5, 0.125, 0.5), (0.0, 0.125, 0.25, 1.0)


def _hip():
    from ray_tracing_octrees_amd import hip
    return hip


def _lut(name):
    """"fog": alpha bytes 1 to 8.  "ramp": alpha rising with the index, a run of zero-alpha entries in the middle (64 .. 191: the
    prefix count decides skips) and fully opaque entries at the top.  "opaque": alpha 255 everywhere.  "ones": alpha 1 everywhere."""
    rgb = tp._lut() & np.uint32(0x00ffffff)
    i = np.arange(256)
    a = {"fog": 1 + i // 32, "ramp": np.where((i >= 64) & (i < 192), 0, np.where(i >= 248, 255, 40 + i // 2)),
         "opaque": np.full(256, 255), "ones": np.ones(256, np.int64)}[name]
    return (rgb | (a.astype(np.uint32) << np.uint32(24))).astype(np.uint32)


def _comp(hip, code, **kw):
    kw.setdefault("range", (1, 200))
    return hip.make_field_composite(code, background_rgba=BG, miss_rgba=MISS, **kw)


def _under(W, H):
    """A frame to composite over: seeded colours in [0, 1), a few above 1 and a few negative."""
    rng = np.random.default_rng(W * 1000 + H)
    u = rng.random((H, W, 4), dtype=np.float32)
    u[::3, ::5, 0] = np.float32(1.5)
    u[1::4, ::7, 2] = np.float32(-0.25)
    return u


NAMES = ("rgba", "transmittance", "first", "stops", "counts", "summary")


def _same(got, want, what):
    """A frame's six results against the statement's (or another frame's), bit for bit."""
    for name, a, b in zip(NAMES, got, want):
        if name == "summary":
            assert a.tolist() == b.tolist(), (what, a, b)
        elif name == "rgba":
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), \
                f"{what}: {int((a.view(np.uint32) != b.view(np.uint32)).any(-1).sum())} pixels differ"
        else:
            assert a.dtype == b.dtype and np.array_equal(a, b), f"{what}: {int((np.asarray(a) != np.asarray(b)).sum())} {name} differ"


def _caller_volumes(g):
    """{name: (volume, valid window, range)} on grid g: test_projection's "lone" (one valued voxel in the far corner brick), "all",
    "adversarial" (INT32_MIN + 2 and INT32_MAX in one window) and "negative"."""
    v = tp._caller_volumes(g)
    return {"lone": v["lone"] + ((0, 10),), "all": v["all"] + ((0, 100),), "adversarial": v["adversarial"] + (WIDE,),
            "negative": v["negative"] + ((-12, -1),)}


def _cpu_volume(source, g):
    """The volume of a source that the CPU references can make: what the frames' conditions are checked on without a GPU."""
    if source == "air":
        return dr.field(g, dr.SET_SOLID).astype(np.int32)
    if source == "distance":
        return dr.field(g, dr.SET_EMPTY).astype(np.int32)
    if source == "geodesic":
        return gr.field(g, [0]).astype(np.int32)
    if source.startswith("caller:"):
        return _caller_volumes(g)[source[7:]][0]
    return None


def _gpu_volume(ctx, source, g):
    """(FIELD_* code, the volume, the caller's volume or None) of a source on the context, which holds grid g."""
    hip = _hip()
    if source == "air":
        return hip.FIELD_DISTANCE, ctx.distance_field(hip.SET_SOLID)[0], None
    if source.startswith("caller:"):
        vol = _caller_volumes(g)[source[7:]][0]
        return hip.FIELD_CALLER, vol, vol
    code, vol = tp._make_fields(ctx, g, (source,))[source]
    return code, vol, None


def _bites(want, cells, grid, comp, sat, what):
    """The conditions that keep a frame from hiding a failure, on the statement alone."""
    counts, ends = want[4].ravel(), want[6]
    assert (counts >= 3).sum() >= 20, (what, "3 or more contributions", int((counts >= 3).sum()))
    if sat:
        assert (ends == cr.SATURATED).sum() >= 20, (what, "saturated", int((ends == cr.SATURATED).sum()))
    if comp.occlude:
        behind = 0
        for c, e in zip(cells, ends):
            if e == cr.OCCLUDED:
                solid = [int(grid[z, y, x]) == 1 for x, y, z in c]
                behind += solid.index(True) >= 3              # the voxels in front of the first FILLED one are air
        assert behind >= 20, (what, "occluded behind 3 or more air voxels", behind)


# (grid, camera, W, H, source, make_field_composite's keywords, LUT, under, saturating)
CASES = [
    ("base", "outside", 24, 16, "air", dict(valid=(1, 0x7ffffffe), range=(1, 300)), "fog", None, False),
    ("base", "outside", 24, 16, "air", dict(valid=(1, 0x7ffffffe), range=(1, 40), stop_q16=256, occlude=1), "ramp", "separate", True),
    ("base", "axis", 24, 16, "air", dict(valid=(1, 0x7ffffffe), range=(1, 60), stop_q16=32768, occlude=1), "ramp", "in place", True),
    ("base", "axis", 24, 16, "geodesic", dict(range=(0, 60), occlude=1), "fog", None, False),
    ("base", "inside", 24, 16, "geodesic", dict(scale=2, clip=((3, 0, 1), (37, 12, 11))), "fog", "separate", False),
    ("base", "empty", 24, 16, "air", dict(valid=(1, 0x7ffffffe), range=(1, 400), scale=1, stop_q16=32768), "ramp", None, True),
    ("base", "outside", 24, 16, "distance", dict(valid=(1, 0x7ffffffe), range=(1, 16), scale=1), "fog", "in place", False),
    ("base", "outside", 24, 16, "caller:all", dict(range=(0, 400), stop_q16=32768), "ramp", None, True),
    ("base", "outside", 24, 16, "caller:all", dict(range=(-2 ** 31, 2 ** 31 - 1), scale=1), "fog", None, False),
    ("base", "outside", 24, 16, "caller:adversarial", dict(valid=WIDE, range=WIDE), "fog", None, False),
    ("base", "axis", 24, 16, "caller:adversarial", dict(valid=WIDE, range=WIDE, scale=1, occlude=1), "fog", "separate", False),
    ("base", "outside", 24, 16, "caller:negative", dict(valid=WIDE, range=(-12, -1), scale=2), "ramp", None, False),
    ("base", "plane", 72, 8, "distance", dict(valid=(1, 0x7ffffffe), range=(1, 16)), "opaque", None, False),
    ("base", "plane", 72, 8, "air", dict(valid=(1, 0x7ffffffe), range=(1, 300), stop_q16=65535, occlude=1), "fog", "in place", False),
    ("base", "diagonal", 13, 9, "thickness", dict(valid=(1, 0x7ffffffe), range=(1, 64), scale=1), "fog", None, False),
    ("base", "diagonal", 13, 9, "air", dict(valid=(1, 0x7ffffffe), range=(1, 300), occlude=1), "ramp", "separate", False),
    ("base", "outside", 13, 9, "skeleton", dict(scale=2), "ramp", None, False),
    ("base", "axis@0.25", 8, 8, "exposure", dict(range=(0, 5), occlude=1), "fog", None, False),
    ("base", "outside", 13, 9, "parts", dict(scale=2, valid=(1, 0x7ffffffe)), "opaque", "in place", False),
    ("base", "outside", 13, 9, "labels", dict(scale=2, stop_q16=65535), "fog", None, False),
    ("base", "outside", 1, 1, "air", dict(valid=(1, 0x7ffffffe), range=(1, 300)), "fog", None, False),
    ("base", "outside", 13, 9, "caller:lone", dict(range=(0, 10)), "opaque", None, False),
    ("odd", "outside", 24, 16, "air", dict(valid=(1, 0x7ffffffe), range=(1, 30)), "fog", None, False),
    ("odd", "outside", 13, 9, "geodesic", dict(range=(0, 30), occlude=1, stop_q16=256), "ramp", "separate", False),
    ("odd", "inside", 24, 16, "geodesic", dict(scale=2), "fog", None, False),
    ("odd", "axis@0.125", 8, 8, "air", dict(valid=(1, 0x7ffffffe), range=(1, 30), scale=1, occlude=1), "opaque", None, False),
    ("block32", "outside", 24, 16, "air", dict(valid=(1, 0x7ffffffe), range=(1, 600), stop_q16=256, occlude=1,
                                               clip=((3, 0, 2), (32, 29, 32))), "ramp", None, True),
    ("block32", "outside@0.6", 13, 9, "distance", dict(valid=(1, 0x7ffffffe), range=(1, 64)), "ramp", None, False),
    ("block32", "inside", 72, 8, "geodesic", dict(range=(0, 90), occlude=1), "fog", "separate", False),
    ("one", "outside", 8, 8, "air", dict(valid=(1, 0x7ffffffe), range=(1, 20), occlude=1), "ramp", None, False),
    ("one", "inside", 24, 16, "distance", dict(valid=(1, 0x7ffffffe), range=(1, 9)), "fog", None, False),
]
_IDS = ["-".join(str(x) for x in c[:5]) + "-" + c[6] + "".join("-%s" % k for k in c[5]) + ("-" + c[7].replace(" ", "") if c[7] else "") for c in CASES]


def _statement(orc, case, vol, g):
    """(view, pos, cells, composite, lut, under, the statement's frame) of a case on the volume given."""
    hip = _hip()
    gname, cam, W, H, source, kw, lname, under, sat = case
    code = hip.FIELD_CALLER if source.startswith("caller:") else {"air": hip.FIELD_DISTANCE}.get(source, getattr(hip, "FIELD_" + source.upper(), 0))
    v = _comp(hip, code, **kw)
    view, pos, cells = tp._walks(orc, gname, cam, W, H, v)
    lut = _lut(lname)
    u = _under(W, H) if under else None
    return view, pos, cells, v, lut, u, cr.frame_of(cells, W, H, vol, g, v, lut, u)


# ================================================================ CPU
def test_composite_struct_matches_the_header():
    """ctypes rto_field_composite is the header's: size, field order and offsets; the summary's dtype; the symbols exported."""
    hip = _hip()
    V = hip.FieldComposite
    assert C.sizeof(V) == 112
    offs = {name: getattr(V, name).offset for name, _ in V._fields_}
    assert offs == {"source": 0, "scale": 4, "valid_lo": 8, "valid_hi": 12, "range_lo": 16, "range_hi": 20, "clip": 24, "clip_lo": 28,
                    "clip_hi": 40, "stop_q16": 52, "occlude": 56, "background_rgba": 60, "miss_rgba": 76, "reserved": 92}
    hdr = open(os.path.join(ROOT, "include", "rto_hip.h")).read()

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in re.findall(r"(?:float|int32_t|int64_t)\s+([^;]+);", body):
            names += [re.sub(r"\[\d+\]", "", n).strip() for n in decl.split(",")]
        return names
    assert fields("rto_field_composite") == [n for n, _ in V._fields_]
    assert fields("rto_composite_summary") == list(hip.COMPOSITE_SUMMARY_DTYPE.names) == list(cr.SUMMARY_DTYPE.names)
    assert hip.COMPOSITE_SUMMARY_DTYPE.itemsize == 32 and hip.COMPOSITE_SUMMARY_DTYPE == cr.SUMMARY_DTYPE
    lib = hip.load()
    for sym in ("rto_composite_field_device", "rto_composite_field_host", "rto_last_composite_ms"):
        assert sym in hip.SYMBOLS and hasattr(lib, sym) and re.search(r"\b%s\(" % sym, hdr), sym
    assert "static_assert(sizeof(rto_field_composite) == 112 && sizeof(rto_composite_summary) == 32" in open(
        os.path.join(ROOT, "ray_tracing_octrees_amd", "csrc", "rto_composite.inc")).read()
    v = hip.make_field_composite(hip.FIELD_EXPOSURE)
    assert (v.scale, v.valid_lo, v.valid_hi, v.range_lo, v.range_hi, v.clip, v.stop_q16, v.occlude, list(v.reserved)) == \
        (0, 0, 0x7ffffffe, 0, 1, 0, 0, 0, [0] * 5)


def test_the_statement_against_the_host_form():
    """host/Composite (the plain walk, composited in C++) through host_capi on test_projection's seeded rays: T, R, G, B, first,
    stop, count and end, and the colour's bytes, under the three scales, the three LUTs, the four stops, occlusion on and off and
    with a pixel below or without; the settings cycle with the ray, each combination of (LUT, stop, occlude) on at least 30 walks."""
    from ray_tracing_octrees_amd import host
    hip = _hip()
    L = host.load()
    adv = np.array([0, 1, 0x7ffffffe, -1, -7, -2 ** 31 + 2, 0x7fffffff, 2, 1000, -2 ** 30, 5, 9, 77], np.int64)
    luts = [_lut(n) for n in ("fog", "ramp", "opaque")]
    seen, ended = {}, {cr.THROUGH: 0, cr.SATURATED: 0, cr.OCCLUDED: 0}
    res, rgba = np.zeros(8, np.int64), np.zeros(4, np.float32)
    i = 0
    for kind, g, vs, dim, o, d, lo, hi in tp._seeded_rays(13, 3000):
        want_cells = pr.walk(g, vs, dim, o, d, lo, hi)
        i += 1
        li, stop, occ, scale = i % 3, (0, 256, 32768, 65535)[(i // 3) % 4], (i // 12) % 2, (i // 24) % 3
        idx = np.arange(dim[0] * dim[1] * dim[2]).reshape(dim[2], dim[1], dim[0])
        vol = np.ascontiguousarray(adv[(idx * 7 + idx // 5) % len(adv)].astype(np.int32))
        grid = np.ascontiguousarray(((idx * 11 + idx // 3) % 9 == 0).astype(np.uint8))
        window, rng = ((WIDE, WIDE), ((0, 0x7ffffffe), (0, 1000)), ((-7, 77), (-7, 77)))[(i // 72) % 3]
        v = _comp(hip, hip.FIELD_CALLER, scale=scale, valid=window, range=rng, stop_q16=stop, occlude=occ)
        under = np.array([0.5, 1.25, -0.5, 0.75], np.float32) if i % 2 else None
        cells = np.ascontiguousarray(np.array(want_cells, np.int32).reshape(-1, 3))
        dims = np.array(dim, np.int32)
        L.rtoh_composite_ray(vol.ctypes.data, grid.ctypes.data, dims.ctypes.data, cells.ctypes.data, len(want_cells), C.addressof(v),
                             luts[li].ctypes.data, under.ctypes.data if under is not None else None, res.ctypes.data, rgba.ctypes.data)
        T, R, G, B, first, stopv, count, end, _ = cr.ray(want_cells, vol, cr.index_volume(vol, v), grid, v, luts[li])
        assert res.tolist() == [T, R, G, B, first, stopv, count, end], (kind, dim, o, d, li, stop, occ, scale)
        want = cr.colour([T], [R], [G], [B], [bool(want_cells)], v, None if under is None else under[None, :])[0]
        assert rgba.tobytes() == want.tobytes(), (kind, dim, o, d, rgba, want)
        if want_cells:
            seen[(li, stop, occ)] = seen.get((li, stop, occ), 0) + 1
            ended[end] += 1
    assert len(seen) == 24 and min(seen.values()) >= 30, seen
    assert min(ended.values()) >= 100, ended


@pytest.mark.parametrize("scale", [fr.LINEAR, fr.SQRT])
def test_thresholds_give_the_field_views_index(scale):
    """thr[k] = ceil(k m(k) s / D): the number of thresholds <= w is lut_index's index.  Every w of 0 .. s for s in {1, 2, 254, 255,
    256, 65025, 65026}; 20,000 seeded w, the ends and every threshold with its two neighbours for s = 2^32 - 1 (the widest range
    there is, INT32_MIN to INT32_MAX) and for s = 2^32 - 3 (INT32_MIN + 2 to INT32_MAX, the widest window of valued voxels).  The statement's thresholds (Python integers) and host/Composite's (int64, the kernel's
    expression) are the same 256 numbers, sorted and below 2^32."""
    from ray_tracing_octrees_amd import host
    L = host.load()
    for s in (1, 2, 254, 255, 256, 65025, 65026, 2 ** 32 - 3, 2 ** 32 - 1):
        lo = -2 ** 31 if s >= 2 ** 32 - 3 else -7
        hi = lo + s
        thr = cr.thresholds(s, scale)
        got = np.zeros(256, np.uint32)
        L.rtoh_composite_thresholds(scale, lo, hi, got.ctypes.data)
        assert got.tolist() == thr and thr == sorted(thr) and thr[0] == 0 and thr[255] == s
        if s < 2 ** 32 - 3:
            w = np.arange(s + 1, dtype=np.int64)
        else:
            rng = np.random.default_rng(5)
            near = np.array(thr, np.int64)
            w = np.unique(np.clip(np.concatenate([rng.integers(0, s + 1, 20000), [0, 1, s - 1, s], near - 1, near, near + 1]), 0, s))
        want = fr.lut_index(w + lo, lo, hi, scale)
        assert np.array_equal(cr.index_of_thresholds(thr, w), want), (s, scale)
        if s <= 256:                                   # the host form's own index, value by value, clamping included
            for v in range(lo - 2, hi + 3):
                assert L.rtoh_composite_index(v, lo, hi, scale) == int(fr.lut_index([v], lo, hi, scale)[0])


def _small_frame(orc, lname, **kw):
    """The base grid's air field from the "outside" camera at 24 x 16 on the statement."""
    hip = _hip()
    g = tp._base()
    vol = _cpu_volume("air", g)
    v = _comp(hip, hip.FIELD_DISTANCE, valid=(1, 0x7ffffffe), range=(1, 300), **kw)
    view, pos, cells = tp._walks(orc, "base", "outside", 24, 16, v)
    return g, vol, v, cells, cr.frame_of(cells, 24, 16, vol, g, v, _lut(lname))


def test_an_opaque_lut_shows_the_first_valued_voxel(orc):
    """The rule's first consequence on the statement: with alpha 255 everywhere a visiting pixel with a valued voxel has T = 0, one
    contribution, and bit for bit the colour projection_ref gives the pixel under FIRST; a visiting pixel without one keeps the
    background."""
    hip = _hip()
    g, vol, v, cells, want = _small_frame(orc, "opaque")
    p = hip.make_field_projection(hip.FIELD_DISTANCE, hip.PROJECT_FIRST, valid=(1, 0x7ffffffe), range=(1, 300))
    first = pr.frame_of(cells, 24, 16, vol, p, _lut("opaque"))
    valued = first[1] > pr.NONE
    assert valued.sum() >= 100
    assert want[0][valued].tobytes() == first[0][valued].tobytes()
    assert (want[1][valued] == 0).all() and (want[4][valued] == 1).all() and np.array_equal(want[2][valued], first[2][valued])
    none = first[1] == pr.NONE
    assert (want[0][none] == np.float32(BG)).all() and (want[0][first[1] == pr.MISS] == np.float32(MISS)).all()


def test_a_thin_lut_counts_the_valued_voxels(orc):
    """The second consequence: alpha 1 everywhere, stop_q16 = 0, no occlusion: counts are the projection's counts and first is
    FIRST's voxel; no walk saturates."""
    hip = _hip()
    g, vol, v, cells, want = _small_frame(orc, "ones")
    p = hip.make_field_projection(hip.FIELD_DISTANCE, hip.PROJECT_FIRST, valid=(1, 0x7ffffffe))
    first = pr.frame_of(cells, 24, 16, vol, p, _lut("ones"))
    assert np.array_equal(want[4], first[4]) and np.array_equal(want[2], first[2]) and (first[4] >= 3).sum() >= 100
    assert want[5]["saturated"] == 0 and (want[3] == -1).all() and (want[1] > 0).all()


def test_transmittance_never_rises_and_bounds_the_colour(orc):
    """On the statement, for the three LUTs and the four stops: T never increases along a walk and R, G, B <= 255 (65536 - T)."""
    g = tp._base()
    vol = _cpu_volume("air", g)
    hip = _hip()
    steps = 0
    for lname in ("fog", "ramp", "opaque"):
        for stop in (0, 256, 32768, 65535):
            v = _comp(hip, hip.FIELD_DISTANCE, valid=(1, 0x7ffffffe), range=(1, 300), stop_q16=stop)
            view, pos, cells = tp._walks(orc, "base", "outside", 24, 16, v)
            index = cr.index_volume(vol, v)
            for c in cells:
                T, R, G, B, first, stopv, count, end, trace = cr.ray(c, vol, index, g, v, _lut(lname))
                assert all(b <= a for a, b in zip([65536] + trace, trace)) and len(trace) == count
                assert max(R, G, B) <= 255 * (65536 - T) and 0 <= T <= 65536
                assert (end == cr.SATURATED) == (count > 0 and T <= stop)
                steps += count
    assert steps > 5000


@pytest.mark.parametrize("case", [c for c in CASES if c[2] >= 24 and c[3] >= 16], ids=[i for c, i in zip(CASES, _IDS) if c[2] >= 24 and c[3] >= 16])
def test_frames_of_24_by_16_meet_their_conditions(orc, case):
    """Every case at 24 x 16 or larger, on the volume the CPU references make for it: at least 20 pixels with 3 or more
    contributions; at least 20 saturated pixels where the case is a saturating one; at least 20 occluded pixels with 3 or more air
    voxels in front where occlude is set."""
    g = tp.GRIDS[case[0]]()
    vol = _cpu_volume(case[4], g)
    assert vol is not None, "a frame of this size needs a source the CPU references can make"
    view, pos, cells, v, lut, u, want = _statement(orc, case, vol, g)
    _bites(want, cells, g, v, case[8], str(case[:5]))


def test_composite_kernels_keep_their_budgets():
    """The built metadata: k_composite_march, the five k_composite_solid and k_composite_fold without scratch and without VGPR
    spills, within the 64 VGPRs (8 waves per SIMD) DESIGN.md section 29 argues from occupancy; the figures the build gives are
    recorded there."""
    import test_isa_contract as isa
    asm = isa.built_asm()
    if asm is None:
        pytest.skip("no hipcc in this environment")
    meta = isa.kernel_meta(asm)
    names = [k for k in meta if "k_composite_" in k]
    assert len(names) == 7 and len([k for k in names if "k_composite_solid" in k]) == 5 and len([k for k in names if "march" in k]) == 1, names
    for k in names:
        m = meta[k]
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0, (k, m)
        assert m["vgpr"] <= (MARCH_VGPRS if "march" in k else SOLID_VGPRS), (k, m)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("## 29."):]
    assert re.search(r"k_composite_march[^.]*\b%d VGPRs" % MARCH_VGPRS, sec) and re.search(r"k_composite_solid[^.]*\b%d VGPRs" % SOLID_VGPRS, sec)


# ================================================================ GPU
def _build(ctx, g, gmin=GMIN, vox=VOX):
    hip = _hip()
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(g, gmin, vox)


def _run(ctx, f, v, lut, volume, u, mode):
    """composite_field_host with the frame below absent, separate or in place."""
    if u is None:
        return ctx.composite_field_host(f, v, lut, volume)
    return ctx.composite_field_host(f, v, lut, volume, under=u, in_place=(mode == "in place"))


@gpu
@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_gpu_frames_equal_the_statement(ctx, orc, case):
    """Every output of a frame, bit for bit against composite_ref on the same volume and grid, with the tables and without them.
    Frames of 24 x 16 or larger first meet their conditions on the statement."""
    gname, cam, W, H, source, kw, lname, under, sat = case
    g = tp.GRIDS[gname]()
    _build(ctx, g)
    code, vol, caller = _gpu_volume(ctx, source, g)
    cpu = _cpu_volume(source, g)
    if cpu is not None:
        assert np.array_equal(vol, cpu)
    view, pos, cells, v, lut, u, want = _statement(orc, case, vol, g)
    assert v.source == code
    if W >= 24 and H >= 16:
        _bites(want, cells, g, v, sat, str(case[:5]))
    if W * H == 1:
        assert want[4][0, 0] >= 3
    if cam in ("inside", "empty", "plane"):
        assert all(0 <= (pos[a] - GMIN[a]) / VOX < tp._dims(g)[a] for a in range(3))
    f = tp._frame(view, pos, W, H)
    try:
        for table in (True, False):
            ctx.debug_set_projection_table(table)
            _same(_run(ctx, f, v, lut, caller, u, under), want, f"{case[:5]} table {table}")
    finally:
        ctx.debug_set_projection_table(True)


@gpu
def test_gpu_looking_away_is_a_frame_of_misses(ctx, orc):
    """A camera that looks away from the grid: miss_rgba without a frame below, the frame below (through the rule's formulas) with
    one; T = 65536, no voxel, a zero summary."""
    hip = _hip()
    g = tp._base()
    _build(ctx, g)
    vol = ctx.distance_field(hip.SET_SOLID)[0]
    view, pos, cells = tp._walks(orc, "base", "away", 13, 9)
    assert not any(cells)
    v = _comp(hip, hip.FIELD_DISTANCE, occlude=1)
    f = tp._frame(view, pos, 13, 9)
    for u, mode in ((None, None), (_under(13, 9), "separate"), (_under(13, 9), "in place")):
        got = _run(ctx, f, v, _lut("ramp"), None, u, mode)
        _same(got, cr.frame_of(cells, 13, 9, vol, g, v, _lut("ramp"), u), f"away {mode}")
        assert (got[1] == 65536).all() and (got[2] == -1).all() and (got[3] == -1).all() and got[5].tolist() == (0, 0, 0, 0)
        assert (got[0] == (np.float32(MISS) if u is None else u + np.float32(0))).all()


@gpu
@pytest.mark.parametrize("stop", [0, 256, 32768, 65535])
@pytest.mark.parametrize("lname", ["fog", "ramp", "opaque"])
def test_gpu_settings_cross(ctx, orc, lname, stop):
    """The three LUTs times the four stops on the base grid's air field at 13 x 9, each with occlusion and without, under the three
    scales in turn, tables on and off: the statement."""
    hip = _hip()
    g = tp._base()
    _build(ctx, g)
    vol = ctx.distance_field(hip.SET_SOLID)[0]
    W, H = 13, 9
    try:
        for occ in (0, 1):
            scale = (["fog", "ramp", "opaque"].index(lname) + [0, 256, 32768, 65535].index(stop) + occ) % 3
            v = _comp(hip, hip.FIELD_DISTANCE, valid=(1, 0x7ffffffe), range=(1, 150), scale=scale, stop_q16=stop, occlude=occ)
            view, pos, cells = tp._walks(orc, "base", "outside", W, H, v)
            want = cr.frame_of(cells, W, H, vol, g, v, _lut(lname))
            assert want[5]["contributing"] >= 20
            for table in (True, False):
                ctx.debug_set_projection_table(table)
                _same(ctx.composite_field_host(tp._frame(view, pos, W, H), v, _lut(lname), None), want, f"{lname} {stop} occlude {occ} table {table}")
    finally:
        ctx.debug_set_projection_table(True)


@gpu
def test_gpu_cross_checks_against_the_projections(ctx, orc):
    """Against code from before, without the statement.  The opaque LUT: on every visiting pixel with a valued voxel the colour is
    rto_project_field_*'s under FIRST, bit for bit, and the first voxel is its d_voxels.  Alpha 1 everywhere, stop_q16 = 0, no
    occlusion: d_counts and d_first are the projection's d_counts and FIRST's d_voxels."""
    hip = _hip()
    g = tp._base()
    _build(ctx, g)
    ctx.distance_field(hip.SET_SOLID)
    view, pos = tp._camera(orc, "outside", g)
    W, H = 72, 40
    f = tp._frame(view, pos, W, H)
    p = hip.make_field_projection(hip.FIELD_DISTANCE, hip.PROJECT_FIRST, valid=(1, 0x7ffffffe), range=(1, 300))
    first = ctx.project_field_host(f, p, _lut("opaque"))
    v = _comp(hip, hip.FIELD_DISTANCE, valid=(1, 0x7ffffffe), range=(1, 300))
    opaque = ctx.composite_field_host(f, v, _lut("opaque"))
    valued = first[1] > hip.FIELD_PIXEL_NONE
    assert valued.sum() >= 500
    assert opaque[0][valued].tobytes() == first[0][valued].tobytes() and np.array_equal(opaque[2][valued], first[2][valued])
    assert (opaque[1][valued] == 0).all() and opaque[5]["saturated"] == valued.sum() == opaque[5]["contributing"]
    thin = ctx.composite_field_host(f, v, _lut("ones"))
    assert np.array_equal(thin[4], first[4]) and np.array_equal(thin[2], first[2]) and (thin[4] >= 3).sum() >= 500
    assert thin[5]["saturated"] == 0 and thin[5]["visited"] == (first[1] != hip.FIELD_PIXEL_MISS).sum()


@gpu
def test_gpu_the_device_form(ctx, orc):
    """The device form on a caller's stream is the host form: with every optional output, with none, over a separate frame and
    in place, with a caller's volume on the device; the three times are reported."""
    torch = pytest.importorskip("torch")
    hip = _hip()
    g = tp._base()
    _build(ctx, g)
    vol = ctx.distance_field(hip.SET_SOLID)[0]
    view, pos = tp._camera(orc, "outside", g)
    W, H = 72, 40
    n = W * H
    f = tp._frame(view, pos, W, H)
    lut = _lut("ramp")
    v = _comp(hip, hip.FIELD_DISTANCE, valid=(1, 0x7ffffffe), range=(1, 40), stop_q16=256, occlude=1)
    u = _under(W, H)
    plain = ctx.composite_field_host(f, v, lut)
    over = ctx.composite_field_host(f, v, lut, under=u)
    # 7.5 times the pixels of the 24 x 16 frame of this camera and setting, which is held to 20 of each
    assert plain[5]["contributing"] >= 150 and plain[5]["saturated"] >= 150 and plain[5]["occluded"] >= 150
    ms = ctx.last_composite_ms()
    assert len(ms) == 3 and all(m > 0 for m in ms)
    other = torch.cuda.Stream()
    d_lut = torch.from_numpy(lut.view(np.int32)).cuda()
    d_rgba = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
    d_trans, d_first, d_stops, d_counts = (torch.full((n,), 7, dtype=torch.int32, device="cuda") for _ in range(4))
    d_summary = torch.full((4,), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.composite_field_device(f, v, d_lut.data_ptr(), d_rgba.data_ptr(), 0, 0, d_trans.data_ptr(), d_first.data_ptr(), d_stops.data_ptr(),
                               d_counts.data_ptr(), d_summary.data_ptr(), other.cuda_stream)
    other.synchronize()
    got = (d_rgba.cpu().numpy().reshape(H, W, 4), d_trans.cpu().numpy().view(np.uint32).reshape(H, W), d_first.cpu().numpy().reshape(H, W),
           d_stops.cpu().numpy().reshape(H, W), d_counts.cpu().numpy().reshape(H, W),
           d_summary.cpu().numpy().view(hip.COMPOSITE_SUMMARY_DTYPE)[0])
    _same(got, plain, "the device form")
    d_under = torch.from_numpy(u.reshape(-1)).cuda()
    d_rgba.zero_()
    torch.cuda.synchronize()
    ctx.composite_field_device(f, v, d_lut.data_ptr(), d_rgba.data_ptr(), d_under=d_under.data_ptr(), stream=other.cuda_stream)
    other.synchronize()
    assert d_rgba.cpu().numpy().tobytes() == over[0].tobytes() and d_under.cpu().numpy().tobytes() == u.tobytes()
    torch.cuda.synchronize()
    ctx.composite_field_device(f, v, d_lut.data_ptr(), d_under.data_ptr(), d_under=d_under.data_ptr(), stream=other.cuda_stream)     # in place
    other.synchronize()
    assert d_under.cpu().numpy().tobytes() == over[0].tobytes()
    d_vol = torch.from_numpy(vol).cuda()
    vc = _comp(hip, hip.FIELD_CALLER, valid=(1, 0x7ffffffe), range=(1, 40), stop_q16=256, occlude=1)
    d_rgba.zero_()
    torch.cuda.synchronize()
    ctx.composite_field_device(f, vc, d_lut.data_ptr(), d_rgba.data_ptr(), d_vol.data_ptr(), stream=other.cuda_stream)
    other.synchronize()
    assert d_rgba.cpu().numpy().tobytes() == plain[0].tobytes()


@gpu
def test_gpu_untimed_and_captured_frames(orc):
    """What the three field families share on the host and no other test runs: frames that record no events, and work buffers that
    would have to grow inside a stream capture.  The "odd" grid's air field at 13 x 9 on a context of its own (its work buffers
    must not exist yet), a MAX projection and an occluded composite against their statements bit for bit, a field view against
    its own timed frame.  (1) A capture in which the brick table, then the solid table would have to be allocated: each call is
    refused with RTO_E_UNSUPPORTED and its family's text, and the capture goes on.  (2) Frames captured in a HIP graph, tables on
    and off: the replay is the statement, and rto_last_*_ms give -1.  (3) A camera with an infinite coordinate, the one miss rule
    of the walk's entry that no frame meets otherwise: the statement's frame of misses.  (4) The host forms under
    rto_timing_begin(ctx, -1): the statement, and -1 again.  (5) A second context whose first frames are a field view and a
    composite: its first projection allocates nothing, so it may be captured, and replays to the statement."""
    torch = pytest.importorskip("torch")
    import ray_tracing_octrees_amd as rto
    hip = _hip()
    g = tp._odd()
    W, H = 13, 9
    n = W * H
    c = rto.Context(0)
    try:
        _build(c, g)
        vol = c.distance_field(hip.SET_SOLID)[0]
        p = tp._proj(hip, hip.FIELD_DISTANCE, pr.MAX, valid=(1, 0x7ffffffe))
        v = _comp(hip, hip.FIELD_DISTANCE, valid=(1, 0x7ffffffe), range=(1, 150), stop_q16=256, occlude=1)
        fv = hip.make_field_view(hip.FIELD_DISTANCE, sample=hip.SAMPLE_FRONT)
        view, pos, cells = tp._walks(orc, "odd", "outside", W, H, p)
        f = tp._frame(view, pos, W, H)
        want_p = pr.frame_of(cells, W, H, vol, p, tp._lut())
        want_c = cr.frame_of(cells, W, H, vol, g, v, _lut("ramp"))
        assert want_p[5]["valued"] >= 20 and want_c[5]["contributing"] >= 20 and want_c[5]["occluded"] >= 20
        stream = torch.cuda.Stream()
        sp = stream.cuda_stream
        d_plut = torch.from_numpy(tp._lut().view(np.int32)).cuda()
        d_clut = torch.from_numpy(_lut("ramp").view(np.int32)).cuda()
        rgba_v, rgba_p, rgba_c = (torch.zeros(n * 4, dtype=torch.float32, device="cuda") for _ in range(3))
        values, counts = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
        torch.cuda.synchronize()

        def field_view():
            c.render_field_device(f, fv, d_plut.data_ptr(), rgba_v.data_ptr(), stream=sp)

        def projection():
            c.project_field_device(f, p, d_plut.data_ptr(), rgba_p.data_ptr(), d_values=values.data_ptr(), stream=sp)

        def composite():
            c.composite_field_device(f, v, d_clut.data_ptr(), rgba_c.data_ptr(), d_counts=counts.data_ptr(), stream=sp)

        def replayed(graph, *checks):
            for t in (rgba_v, rgba_p, rgba_c, values, counts):
                t.fill_(7)
            graph.replay()
            torch.cuda.synchronize()
            for check in checks:
                check()

        def is_view():
            assert rgba_v.cpu().numpy().tobytes() == timed_view

        def is_projection():
            assert rgba_p.cpu().numpy().tobytes() == want_p[0].tobytes() and np.array_equal(values.cpu().numpy().reshape(H, W), want_p[1])

        def is_composite():
            assert rgba_c.cpu().numpy().tobytes() == want_c[0].tobytes() and np.array_equal(counts.cpu().numpy().reshape(H, W), want_c[4])

        field_view()                                         # the ray tables and the views' buffers; no brick table yet
        stream.synchronize()
        timed_view = rgba_v.cpu().numpy().tobytes()
        assert all(m > 0 for m in c.last_field_view_ms()) and timed_view != bytes(len(timed_view))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                with pytest.raises(rto.RtoError) as e:
                    projection()
                field_view()
        assert e.value.code == hip.RTO_E_UNSUPPORTED and "rto_project_field_device: a larger grid allocates the brick table" in str(e.value)
        assert c.last_field_view_ms() == (-1.0, -1.0)
        replayed(graph, is_view)
        projection()
        stream.synchronize()
        is_projection()
        assert all(m > 0 for m in c.last_projection_ms())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                with pytest.raises(rto.RtoError) as e:
                    composite()
                projection()
        assert e.value.code == hip.RTO_E_UNSUPPORTED and "rto_composite_field_device: a larger grid allocates the solid table" in str(e.value)
        assert c.last_projection_ms() == (-1.0, -1.0, -1.0)
        replayed(graph, is_projection)
        composite()
        stream.synchronize()
        is_composite()
        assert all(m > 0 for m in c.last_composite_ms())
        for table in (True, False):
            c.debug_set_projection_table(table)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(stream):
                with torch.cuda.graph(graph, stream=stream):
                    field_view()
                    projection()
                    composite()
            assert c.last_composite_ms() == c.last_projection_ms() == (-1.0, -1.0, -1.0) and c.last_field_view_ms() == (-1.0, -1.0)
            replayed(graph, is_view, is_projection, is_composite)
        del graph
        far = np.array(pos, np.float32)
        far[1] = np.inf                                      # a camera that is nowhere: every pixel misses by the walk's first rule
        none = pr.walks(tp.GMIN, tp.VOX, tp._dims(g), far, tp._rays(orc, view, far, W, H), None)
        assert len(none) == n and not any(none)
        ff = tp._frame(view, far, W, H)
        tp._same(c.project_field_host(ff, p, tp._lut()), pr.frame_of(none, W, H, vol, p, tp._lut()), "a camera at infinity")
        _same(c.composite_field_host(ff, v, _lut("ramp")), cr.frame_of(none, W, H, vol, g, v, _lut("ramp")), "a camera at infinity")
        c.timing_begin(-1)
        for table in (True, False):
            c.debug_set_projection_table(table)
            tp._same(c.project_field_host(f, p, tp._lut()), want_p, f"no events, table {table}")
            _same(c.composite_field_host(f, v, _lut("ramp")), want_c, f"no events, table {table}")
            assert c.render_field_host(f, fv, tp._lut())[0].tobytes() == timed_view
            assert c.last_composite_ms() == c.last_projection_ms() == (-1.0, -1.0, -1.0) and c.last_field_view_ms() == (-1.0, -1.0)
    finally:
        c.close()
    # (5) on a second context: the composite makes the brick table, so the projections' events have to come with it
    c = rto.Context(0)
    try:
        _build(c, g)
        c.distance_field(hip.SET_SOLID)
        field_view()
        composite()
        stream.synchronize()
        is_composite()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                projection()
        assert c.last_projection_ms() == (-1.0, -1.0, -1.0)
        replayed(graph, is_projection)
        del graph
        projection()
        stream.synchronize()
        is_projection()
        assert all(m > 0 for m in c.last_projection_ms())
    finally:
        c.close()


@gpu
def test_gpu_an_edit_drops_the_named_sources_and_renews_the_tables(ctx, orc):
    """After an rto_edit_voxels with changed > 0 every named source is refused in its readers' words; a CALLER composite with
    occlusion is the statement on the edited grid (the solid table is the new grid's); after the field is made again the composite
    is the statement on the new field."""
    hip = _hip()
    g = tp._base()
    fields = tp._make_fields(ctx, g)
    W, H = 24, 16
    view, pos, cells = tp._walks(orc, "base", "axis", W, H)
    f = tp._frame(view, pos, W, H)
    lut = _lut("ramp")
    air = _cpu_volume("air", g)
    vc = _comp(hip, hip.FIELD_CALLER, valid=(1, 0x7ffffffe), range=(1, 60), occlude=1)
    before = ctx.composite_field_host(f, vc, lut, air)
    _same(before, cr.frame_of(cells, W, H, air, g, vc, lut), "before the edit")
    # a slab of solid in front of the "axis" camera: it occludes pixels that saw the volume before
    lo, hi = tp._vpos(22, 0, 10), tp._vpos(36, 12, 12)
    brush = hip.make_brushes([(lo + hi) / 2], [(hi - lo) / 2], hip.BRUSH_BOX, hip.EDIT_FILL)
    assert ctx.edit_voxels(brush) > 0
    edited = ctx.download_voxels()
    assert (edited != g).sum() > 0
    for name, (code, _) in fields.items():
        with pytest.raises(hip.RtoError) as e:
            ctx.composite_field_host(f, _comp(hip, code), lut)
        assert e.value.code == hip.RTO_E_INVALID and "the grid has changed since" in str(e.value), (name, str(e.value))
    assert np.array_equal(ctx.download_voxels(), edited)
    want = cr.frame_of(cells, W, H, air, edited, vc, lut)
    assert want[5]["occluded"] != before[5]["occluded"] or not np.array_equal(want[3], before[3])
    for table in (True, False):
        ctx.debug_set_projection_table(table)
        _same(ctx.composite_field_host(f, vc, lut, air), want, f"CALLER after the edit, table {table}")
    ctx.debug_set_projection_table(True)
    field = ctx.distance_field(hip.SET_SOLID)[0]
    assert np.array_equal(field, dr.field(edited, dr.SET_SOLID))
    v = _comp(hip, hip.FIELD_DISTANCE, valid=(1, 0x7ffffffe), range=(1, 60), occlude=1)
    after = ctx.composite_field_host(f, v, lut)
    assert after[5]["contributing"] >= 20
    _same(after, cr.frame_of(cells, W, H, field, edited, v, lut), "made again")


@gpu
def test_gpu_composites_ignore_a_frustum_update(ctx, orc):
    """rto_update_frustum in force changes nothing: every output in every state of test_frustum_states.py's first grid scene equals
    the call with culling off, which is the statement's."""
    import frustum_states as fs
    import test_frustum_states as tfs
    hip = _hip()
    s = tfs.scene(orc, fs.GRID_SCENES[0])
    lut = _lut("ramp")
    comps = {"fog": _comp(hip, hip.FIELD_DISTANCE, valid=(1, 0x7ffffffe), range=(1, 40), scale=hip.SCALE_SQRT, occlude=0),
             "stopped": _comp(hip, hip.FIELD_DISTANCE, valid=(1, 0x7ffffffe), range=(1, 40), stop_q16=256, occlude=1, clip=tfs._clip(s))}
    tfs._resident(ctx, s)
    vol = ctx.distance_field(hip.SET_SOLID)[0]
    grid = np.ascontiguousarray(s.grid.data, np.uint8)

    def call():
        out = {}
        for table in (True, False):
            ctx.debug_set_projection_table(table)
            for cname, v in comps.items():
                for W, H in fs.FRAMES:
                    got = ctx.composite_field_host(tfs._frame(s, W, H), v, lut)
                    out.update({f"{cname} table {table} {W}x{H} {k}": x for k, x in zip(NAMES, got)})
        ctx.debug_set_projection_table(True)
        return out

    def statement(out):
        W, H = fs.FRAMES[1]
        rd = tfs._pixel_rays(orc, s, W, H)
        dim = (grid.shape[2], grid.shape[1], grid.shape[0])
        for cname, v in comps.items():
            want = cr.frame_of(cr.walks(s.min, s.voxel, dim, s.pos, rd, v), W, H, vol, grid, v, lut)
            assert want[5]["contributing"] >= 100
            for table in (True, False):
                for k, w in zip(NAMES, want):
                    assert np.ascontiguousarray(out[f"{cname} table {table} {W}x{H} {k}"]).tobytes() == np.ascontiguousarray(w).tobytes(), \
                        f"{cname} table {table}: {k} differs from composite_ref"

    tfs._ignoring(ctx, orc, s, call, statement)


@gpu
def test_gpu_error_codes_in_the_header_s_order(ctx, orc, scenes):
    """Every refusal of the header.  Each call below is wrong in the way named and also in every way checked later, so the code
    and text it answers show the order: NULLs, alignment, source, scale, reserved, valid, the range, stop_q16, occlude, frame size,
    frame limits, the volume's presence, (fresh context) no octree, no grid, the clip box, the source's residency.  A refused call
    leaves the next frame unchanged."""
    torch = pytest.importorskip("torch")
    hip = _hip()
    g = tp._base()
    code, vol = tp._make_fields(ctx, g, ("thickness",))["thickness"]
    view, pos = tp._camera(orc, "outside", g)
    W, H = 24, 16
    f = tp._frame(view, pos, W, H)
    lut = _lut("ramp")
    good = _comp(hip, code, range=(1, 16), occlude=1)
    ref = ctx.composite_field_host(f, good, lut)
    Lib = ctx._L
    out = np.zeros((H, W, 4), np.float32)

    def call(comp, frame=f, lut_=lut, buf=out, volume=None, c=ctx):
        rc = Lib.rto_composite_field_host(c._h, C.byref(frame) if frame is not None else None, C.byref(comp) if comp is not None else None,
                                          lut_.ctypes.data if lut_ is not None else None, volume.ctypes.data if volume is not None else None,
                                          None, buf.ctypes.data if buf is not None else None, None, None, None, None, None)
        return rc, Lib.rto_last_error(c._h).decode()

    def worst():
        """A composite wrong in every way one can be, on a source that is not resident."""
        v = hip.make_field_composite(hip.FIELD_GEODESIC, scale=9, valid=(3, 2), range=(5, 5), clip=((0, 0, 0), (41, 12, 12)), stop_q16=65536,
                                     occlude=2)
        v.reserved[3] = 1
        return v

    big = hip.make_frame(view, pos, 1.0, FOV, 65536, 65536)
    flat = hip.make_frame(view, pos, 1.0, FOV, 0, 16)
    assert call(good)[0] == hip.RTO_OK
    for kw in (dict(frame=None), dict(lut_=None), dict(buf=None)):
        rc, msg = call(worst(), volume=vol, **kw)
        assert rc == hip.RTO_E_INVALID and "NULL" in msg, kw
    assert call(None)[0] == hip.RTO_E_INVALID
    v = worst()
    steps = [("source", lambda: setattr(v, "source", 8), "unknown source"), ("source", lambda: setattr(v, "source", -1), "unknown source"),
             ("scale", lambda: setattr(v, "source", hip.FIELD_GEODESIC), "unknown scale"), ("scale", lambda: setattr(v, "scale", -1), "unknown scale"),
             ("reserved", lambda: setattr(v, "scale", 0), "reserved"), ("valid", lambda: v.reserved.__setitem__(3, 0), "valid_lo"),
             ("valid", lambda: (setattr(v, "valid_lo", -2 ** 31 + 1), setattr(v, "valid_hi", 5)), "valid_lo"),
             ("range", lambda: setattr(v, "valid_lo", -2 ** 31 + 2), "range_lo < range_hi"),
             ("range", lambda: (setattr(v, "scale", 1), setattr(v, "range_lo", 6)), "range_lo < range_hi"),
             ("stop", lambda: setattr(v, "range_lo", 1), "stop_q16"), ("stop", lambda: setattr(v, "stop_q16", -1), "stop_q16"),
             ("occlude", lambda: setattr(v, "stop_q16", 65535), "occlude"), ("occlude", lambda: setattr(v, "occlude", -1), "occlude")]
    for what, fix, text in steps:
        fix()
        rc, msg = call(v, frame=big, volume=vol)
        assert rc == hip.RTO_E_INVALID and text in msg, (what, msg)
    v.occlude = 1
    rc, msg = call(v, frame=flat, volume=vol)
    assert rc == hip.RTO_E_INVALID and "width/height" in msg
    rc, msg = call(v, frame=big, volume=vol)
    assert rc == hip.RTO_E_INVALID and "too large" in msg
    rc, msg = call(v, volume=vol)
    assert rc == hip.RTO_E_INVALID and "RTO_FIELD_CALLER only" in msg
    v.source = hip.FIELD_CALLER
    rc, msg = call(v)
    assert rc == hip.RTO_E_INVALID and "needs a volume" in msg
    # CATEGORY ignores the range: equal ends are no refusal
    cat = _comp(hip, code, scale=hip.SCALE_CATEGORY, range=(7, 7))
    assert call(cat)[0] == hip.RTO_OK
    fresh = hip.Context(0)
    try:
        v.source = hip.FIELD_GEODESIC
        assert call(v, c=fresh)[0] == hip.RTO_E_NO_OCTREE
        s = scenes("sphere16")
        fresh.upload_octree(s.nodes, GMIN, VOX)
        rc, msg = call(v, c=fresh)
        assert rc == hip.RTO_E_UNSUPPORTED and "no voxel grid is resident" in msg
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
    assert rc == hip.RTO_E_INVALID and "no labels are resident" in msg
    # the device form's alignment, behind the NULLs and in front of everything else
    dev = Lib.rto_composite_field_device
    d = torch.zeros(W * H * 4 + 64, dtype=torch.float32, device="cuda")
    d_lut = torch.from_numpy(lut.view(np.int32)).cuda()
    p0 = d.data_ptr()
    P = lambda x: C.c_void_p(x) if x else None

    def devcall(comp, lut_=d_lut.data_ptr(), volume=0, under=0, rgba=p0, trans=0, first=0, stops=0, counts=0, summary=0):
        return dev(ctx._h, C.byref(f), C.byref(comp), P(lut_), P(volume), P(under), P(rgba), P(trans), P(first), P(stops), P(counts),
                   P(summary), None), Lib.rto_last_error(ctx._h).decode()

    bad = worst()
    for kw in (dict(rgba=p0 + 4), dict(under=p0 + 8), dict(lut_=p0 + 2), dict(volume=p0 + 2), dict(trans=p0 + 2), dict(first=p0 + 2),
               dict(stops=p0 + 2), dict(counts=p0 + 2), dict(summary=p0 + 4)):
        rc, msg = devcall(bad, **kw)
        assert rc == hip.RTO_E_INVALID and "aligned" in msg, kw
    rc, msg = devcall(bad, rgba=0)
    assert rc == hip.RTO_E_INVALID and "NULL" in msg
    rc, msg = devcall(bad)
    assert rc == hip.RTO_E_INVALID and "unknown scale" in msg
    torch.cuda.synchronize()
    _same(ctx.composite_field_host(f, good, lut), ref, "after the refusals")


# ---------------------------------------------------------------- the solid table's launch shapes
# k_composite_solid loads BYTES = the largest power of two up to 16 that divides dimX; a wave's run is 8 BYTES voxels along x.
# name: (BYTES, runs along x): every BYTES, one run and several, whole and partial last runs, partial brick rows in y and z,
# a last workgroup that is not full.
LONG_SHAPES = {"long65": (1, 9), "long72": (8, 2), "long100": (4, 4), "long128": (16, 1), "long130": (2, 9), "long200": (8, 4)}


def _long_solids(name):
    """test_projection's long grid emptied at x < 64 and thinned behind: air everywhere in front, solids only at x >= 64, so that a
    missing or wrong record of a later run shows as a pixel that is not occluded (or a brick that is skipped)."""
    dx, dy, dz, _ = tp.LONG[name]
    z, y, x = np.meshgrid(np.arange(dz), np.arange(dy), np.arange(dx), indexing="ij")
    return ((x >= 64) & ((x + 2 * y + z) % 3 == 0)).astype(np.uint8)


def _long_cells(orc, name):
    """[(camera, W, H, view, pos, walks)]: from inside the grid at x = 56.5 looking along +x at 24 x 16, and test_projection's
    oblique "orbit" around (max(64, dimX / 2), dimY / 2, dimZ / 2) at 13 x 9."""
    dx, dy, dz, (gmin, vox) = tp.LONG[name]
    at = lambda x, y, z: (gmin + (np.array([x, y, z], np.float32) * vox).astype(np.float32)).astype(np.float32)
    out = []
    pos = at(56.5, dy / 2 + 0.3, dz / 2 + 0.2)
    view = tp._x_view(pos, 1)
    out.append(("inside", tp.LW, tp.LH, view, pos, pr.walks(gmin, vox, (dx, dy, dz), pos, tp._rays(orc, view, pos, tp.LW, tp.LH))))
    cam = orc.Camera(0.6, 0.45, float(np.float32(12 * float(vox))))
    cam.set_target(*[float(v) for v in at(max(64, dx / 2), dy / 2, dz / 2)])
    view, pos = cam.get_view(), cam.get_pos()
    out.append(("orbit", 13, 9, view, pos, pr.walks(gmin, vox, (dx, dy, dz), pos, tp._rays(orc, view, pos, 13, 9))))
    return out


def _long_runs(hip, name, g):
    """[(composite, caller volume or None, LUT)] of a long grid.  The resident distance to SOLID under fog: every air voxel
    contributes, the march reads the grid's bytes all the way.  A caller's volume -- that distance at x < 64 and nothing valued
    behind -- under the ramp: every brick of the later runs is one the value table would skip, so the solid table alone keeps the
    march from jumping over their solids."""
    air = _cpu_volume("air", g)
    front = np.where(np.arange(g.shape[2])[None, None, :] < 64, air, -1).astype(np.int32)
    return [(_comp(hip, hip.FIELD_DISTANCE, valid=(1, 0x7ffffffe), range=(1, 50), occlude=1), None, "fog"),
            (_comp(hip, hip.FIELD_CALLER, valid=(1, 0x7ffffffe), range=(1, 200), occlude=1), front, "ramp")]


@pytest.mark.parametrize("name", list(LONG_SHAPES))
def test_long_rows_take_every_shape_of_the_solid_table(orc, name):
    """On the host alone: the grids' BYTES and runs are the ones the table of DESIGN.md section 29 lists.  On the statement, for
    both settings of _long_runs: every occluding voxel lies at x >= 64, and the "inside" frame (24 x 16) meets the frames'
    conditions: 20 pixels with 3 or more contributions, 20 occluded behind 3 or more air voxels.  Sensitivity: a solid table that called every brick of the
    later runs empty would let the march skip them under the second setting, which is the statement on a grid without solids: it
    differs from the statement in d_stops on every occluded pixel."""
    dx, dy, dz, _ = tp.LONG[name]
    b = next(k for k in (16, 8, 4, 2, 1) if dx % k == 0)
    assert (b, -(-dx // (8 * b))) == LONG_SHAPES[name]
    hip = _hip()
    g = _long_solids(name)
    assert not g[:, :, :64].any()
    air = _cpu_volume("air", g)
    for v, volume, lname in _long_runs(hip, name, g):
        for cname, W, H, view, pos, cells in _long_cells(orc, name):
            want = cr.frame_of(cells, W, H, air if volume is None else volume, g, v, _lut(lname))
            occ = want[6] == cr.OCCLUDED
            assert (want[3].ravel()[occ] % dx >= 64).all(), (name, cname)
            if cname == "inside":
                _bites(want, cells, g, v, False, f"{name} {cname} {lname}")
            if volume is not None:
                blind = cr.frame_of(cells, W, H, volume, np.zeros_like(g), v, _lut(lname))
                assert (blind[3].ravel() != want[3].ravel()).sum() == occ.sum() > 0


@gpu
@pytest.mark.parametrize("name", list(LONG_SHAPES))
def test_gpu_long_rows_equal_the_statement(ctx, orc, name):
    """Rows of 65 to 200 voxels with occlusion: every BYTES of k_composite_solid, with one run and with several, against the
    statement, with the tables and without; solids only at x >= 64, under _long_runs' two settings."""
    hip = _hip()
    dx, dy, dz, (gmin, vox) = tp.LONG[name]
    g = _long_solids(name)
    _build(ctx, g, gmin, vox)
    vol = ctx.distance_field(hip.SET_SOLID)[0]
    assert np.array_equal(vol, _cpu_volume("air", g))
    try:
        for cname, W, H, view, pos, cells in _long_cells(orc, name):
            f = tp._frame(view, pos, W, H)
            for v, volume, lname in _long_runs(hip, name, g):
                want = cr.frame_of(cells, W, H, vol if volume is None else volume, g, v, _lut(lname))
                if cname == "inside":
                    _bites(want, cells, g, v, False, f"{name} {cname} {lname}")
                for table in (True, False):
                    ctx.debug_set_projection_table(table)
                    _same(ctx.composite_field_host(f, v, _lut(lname), volume), want, f"{name} {cname} {lname} table {table}")
    finally:
        ctx.debug_set_projection_table(True)


@gpu
def test_gpu_drop_in_composite_field(orc):
    """RayTracerBVH::compositeField through host.py: framebuffer(), compositeValues() and compositeSummary() are the C ABI's frame,
    without a frame below and over one."""
    import ray_tracing_octrees_amd as rto
    hip = _hip()
    grid = rto.VoxelGrid.test_sphere(32)
    rt = rto.RayTracerBVH()
    rt.ensureComputeInitialized()
    rt.setOctreeFromGrid(grid)
    cam = rto.Camera(*SPHERE_CAM)
    W, H = 96, 72
    lut = _lut("ramp")
    v = _comp(hip, hip.FIELD_DISTANCE, valid=(1, 0x7ffffffe), range=(1, 100), scale=hip.SCALE_SQRT, stop_q16=256, occlude=1)
    assert rt.compositeField(cam, W, H, W / H, FOV, v, lut) == hip.RTO_E_INVALID and "the grid has changed since" in rt.lastError
    assert rt.compositeValues() is None
    assert rt.distanceField(hip.SET_SOLID)[0] == hip.RTO_OK
    og = orc.test_sphere_grid(32)
    ctx = rto.Context(0)
    try:
        ctx.build_octree(og.data, og.min, og.voxel_size)
        ctx.distance_field(hip.SET_SOLID)
        f = rto.make_frame(cam.getView(), cam.getPos(), W / H, FOV, W, H)
        for u in (None, _under(W, H)):
            assert rt.compositeField(cam, W, H, W / H, FOV, v, lut, under=u) == hip.RTO_OK
            want = ctx.composite_field_host(f, v, lut, under=u)
            assert want[5]["contributing"] > 500 and want[5]["occluded"] > 100
            _same((rt.framebuffer(),) + rt.compositeValues() + (rt.compositeSummary(),), want, "the drop-in class")
    finally:
        ctx.close()
