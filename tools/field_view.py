#!/usr/bin/env python3
"""Makes a field on a scene, renders it from the scene's camera with rto_render_field_host and writes the frame as a binary PPM
and the legend (range, the 256 bins, the LUT) as JSON beside it.  numpy only.

    python3 tools/field_view.py --scene calgary --field sky --out calgary_sky.ppm
    python3 tools/field_view.py --scene sphere128 --field thickness --clip 0.5 --out cut.ppm
    python3 tools/field_view.py --scene sphere128 --field distance --project max --out xray.ppm
    python3 tools/field_view.py --scene calgary --field air --composite --over-lit --out fog.ppm
    python3 tools/field_view.py --scene calgary --field dose --sources 200,120,3,1000000 60,40,5,500000 --composite --out dose.ppm

Scenes: sphereN (the test sphere of edge N, Camera(0.5, 0.7, 1.8)) and calgary (the shipped city grid, Camera(0.6, 0.5, 3500)).
Fields: distance (to EMPTY, SQRT scale: how deep inside), thickness (SQRT), skeleton, labels and parts (CATEGORY), geodesic
(through EMPTY from voxel 0, sampled in FRONT of the surface), sun (exposure along one direction) and sky (exposure over 64
directions of the upper hemisphere: the sky view factor; both sampled in FRONT of the surface).  --clip F keeps the part of the
grid below the fraction F of its x extent (a section through the solid).  --project OP (max, min, mean, count, first) renders a
projection instead (rto_project_field_host): the reduction of the field along every pixel ray through the grid, or through the
--clip box; --window LO HI sets the values that count (for first: the threshold of an isosurface seen through walls).
--composite renders the field as a volume seen through (rto_composite_field_*): the LUT's colours with an opacity that rises from
--opacity / 4 to --opacity (alpha bytes), composited front to back; --see-through lets the rays pass the solids (by default they
stop at the first one); --stop Q ends a ray once its transmittance (of 65536) is at most Q; --range LO HI is the range of the
colours (by default the smallest and largest value a 160 x 90 projection from the same camera finds).  --over-lit renders the lit
frame on the device and composites over it in place (needs torch for the device buffers); without it the background is the sky
colour.  Field `air` is the distance to SOLID, which lives in the empty space.  Field `dose` (rto_dose_field) takes its point sources
from --sources, one `i,j,k,w` each (a voxel of the grid and a weight), with --transmit (Q16 table entries; none: line of sight),
--reach and the inverse-square falloff unless --no-falloff; it has no FIELD_* code, so its plain view, --project and --composite go
through Context.dose_device() and FIELD_CALLER on the device entry points (needs torch for the device buffers)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import ray_tracing_octrees_amd as rto
from ray_tracing_octrees_amd import hip

HEAT = [(12, 7, 60, 255), (90, 20, 140, 255), (200, 60, 90, 255), (250, 150, 40, 255), (252, 250, 180, 255)]


def scene(name):
    """(grid, camera, the index of the axis that points up)."""
    if name == "calgary":
        z = np.load(os.path.join(ROOT, "tests", "golden", "ref_scene_cache.npz"))
        dims = tuple(int(x) for x in z["dims"])
        data = np.unpackbits(z["packed"])[: dims[0] * dims[1] * dims[2]].reshape(dims[2], dims[1], dims[0])
        return rto.VoxelGrid.from_array(data, z["min"].astype(np.float32), np.float32(z["voxel"])), rto.Camera(0.6, 0.5, 3500.0), 2
    if name.startswith("sphere"):
        return rto.VoxelGrid.test_sphere(int(name[6:])), rto.Camera(0.5, 0.7, 1.8), 1
    raise SystemExit(f"unknown scene {name}")


def sky_directions(n, up):
    """n directions spread evenly in solid angle over the hemisphere around axis `up` (a golden-angle spiral), as integers."""
    i = np.arange(n)
    h = 1.0 - (i + 0.5) / n
    r = np.sqrt(1.0 - h * h)
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    d = np.zeros((n, 3))
    d[:, up] = h
    d[:, (up + 1) % 3] = r * np.cos(phi)
    d[:, (up + 2) % 3] = r * np.sin(phi)
    return hip.quantize_directions(d, 31)


def make_field(ctx, field, up, voxel):
    """Makes the field resident; returns make_field_view's keywords for it."""
    if field == "distance":
        ctx.distance_field(hip.SET_EMPTY)
        return dict(source=hip.FIELD_DISTANCE, scale=hip.SCALE_SQRT)
    if field == "air":
        ctx.distance_field(hip.SET_SOLID)
        return dict(source=hip.FIELD_DISTANCE, scale=hip.SCALE_SQRT, valid=(1, 0x7ffffffe))
    if field == "thickness":
        ctx.thickness_field(hip.SET_SOLID, 8 * float(voxel))
        return dict(source=hip.FIELD_THICKNESS, scale=hip.SCALE_SQRT)
    if field == "skeleton":
        ctx.skeleton_field()
        return dict(source=hip.FIELD_SKELETON, scale=hip.SCALE_CATEGORY)
    if field == "labels":
        ctx.label_components(hip.SET_SOLID, hip.CONN_FACE)
        return dict(source=hip.FIELD_LABELS, scale=hip.SCALE_CATEGORY)
    if field == "parts":
        ctx.segment_parts(hip.SET_SOLID, hip.CONN_FACE, 800)
        return dict(source=hip.FIELD_PARTS, scale=hip.SCALE_CATEGORY)
    if field == "geodesic":
        ctx.geodesic_field([0], hip.SET_EMPTY, hip.CONN_FACE)
        return dict(source=hip.FIELD_GEODESIC, sample=hip.SAMPLE_FRONT)
    if field in ("sun", "sky"):
        dirs = sky_directions(64, up) if field == "sky" else sky_directions(8, up)[2:3]
        ctx.exposure_field(dirs, None, hip.EXPO_SKIN, None)
        return dict(source=hip.FIELD_EXPOSURE, sample=hip.SAMPLE_FRONT, range=(0, len(dirs)))
    raise SystemExit(f"unknown field {field}")


def dose_frame(ctx, f, a, lut, kw):
    """The frame of --field dose and its legend: the resident dose field as FIELD_CALLER's device volume, whichever the mode."""
    import torch
    src = np.asarray([[int(c) for c in s.split(",")] for s in a.sources], np.int64).reshape(-1, 4)
    e, s = ctx.dose_field(src, a.transmit, hip.DOSE_FALLOFF_NONE if a.no_falloff else hip.DOSE_FALLOFF_INVERSE_SQUARE,
                          hip.DOSE_ALL if (a.composite or a.project) else hip.DOSE_SKIN, a.reach)
    del e
    volume = ctx.dose_device()
    kw = dict(kw, source=hip.FIELD_CALLER, scale=hip.SCALE_SQRT, range=tuple(a.range) if a.range else (0, max(1, int(s["peak"]))))
    if a.window:
        kw["valid"] = tuple(a.window)
    n = f.width * f.height
    sky = (0.55, 0.7, 0.9, 1.0)
    d_rgba = torch.empty(n * 4, dtype=torch.float32, device="cuda")
    d_summary = torch.zeros(4, dtype=torch.int64, device="cuda")
    legend = {name: int(s[name]) for name in hip.DOSE_SUMMARY_DTYPE.names}
    legend.update(covered=ctx.dose_coverage().tolist(), dose_ms=list(ctx.last_dose_ms()))
    if a.composite:
        alpha = np.clip(a.opacity // 4 + (np.arange(256) * (a.opacity - a.opacity // 4)) // 255, 0, 255).astype(np.uint32)
        lut = (lut & np.uint32(0x00ffffff)) | (alpha << np.uint32(24))
        kw["valid"] = kw.get("valid", (1, 0x7ffffffe))                  # dark air adds nothing
        comp = hip.make_field_composite(stop_q16=a.stop, occlude=not a.see_through, background_rgba=sky, miss_rgba=sky, **kw)
        d_lut = torch.from_numpy(lut.view(np.int32)).cuda()
        ctx.composite_field_device(f, comp, d_lut.data_ptr(), d_rgba.data_ptr(), volume, d_summary=d_summary.data_ptr())
        names, ms = hip.COMPOSITE_SUMMARY_DTYPE, ctx.last_composite_ms
    elif a.project:
        op = {"max": hip.PROJECT_MAX, "min": hip.PROJECT_MIN, "mean": hip.PROJECT_MEAN, "count": hip.PROJECT_COUNT, "first": hip.PROJECT_FIRST}[a.project]
        view = hip.make_field_projection(op=op, miss_rgba=sky, none_rgba=(0.3, 0.3, 0.3, 1.0), **kw)
        d_lut = torch.from_numpy(lut.view(np.int32)).cuda()
        ctx.project_field_device(f, view, d_lut.data_ptr(), d_rgba.data_ptr(), volume, d_summary=d_summary.data_ptr())
        names, ms = hip.FIELD_VIEW_SUMMARY_DTYPE, ctx.last_projection_ms
    else:
        view = hip.make_field_view(sample=hip.SAMPLE_FRONT, mode=hip.QUERY_FIRST if a.mode == "first" else hip.QUERY_CLOSEST, shade=not a.flat,
                                   miss_rgba=sky, none_rgba=(0.3, 0.3, 0.3, 1.0), **kw)
        d_lut = torch.from_numpy(lut.view(np.int32)).cuda()
        ctx.render_field_device(f, view, d_lut.data_ptr(), d_rgba.data_ptr(), volume, d_summary=d_summary.data_ptr())
        names, ms = hip.FIELD_VIEW_SUMMARY_DTYPE, ctx.last_field_view_ms
    ctx.synchronize()
    frame = d_summary.cpu().numpy().view(names)[0]
    legend.update({name: int(frame[name]) for name in names.names})
    legend.update(range=list(kw["range"]), scale=int(kw["scale"]), lut_rgba=lut.view(np.uint8).reshape(256, 4).tolist(), ms=list(ms()))
    return d_rgba.cpu().numpy().reshape(f.height, f.width, 4), legend


def write_ppm(path, rgba):
    """Binary PPM of the frame's r, g, b (clamped to [0, 1], 8 bits)."""
    rgb = np.clip(np.rint(rgba[..., :3] * 255.0), 0, 255).astype(np.uint8)
    with open(path, "wb") as fh:
        fh.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
        fh.write(np.ascontiguousarray(rgb).tobytes())


def composite(ctx, f, kw, lut, a):
    """The frame of --composite and its legend."""
    kw = {k: v for k, v in kw.items() if k != "sample"}
    if a.window:
        kw["valid"] = tuple(a.window)
    if a.range:
        kw["range"] = tuple(a.range)
    elif kw.get("scale") != hip.SCALE_CATEGORY and "range" not in kw:
        small = rto.make_frame(np.array(f.view, np.float32), np.array(f.cam_pos, np.float32), f.aspect, f.fov_deg, 160, 90)
        pk = {k: v for k, v in kw.items() if k in ("source", "scale", "valid", "clip")}
        top = ctx.project_field_host(small, hip.make_field_projection(op=hip.PROJECT_MAX, **pk), lut, totals=False)[5]
        low = ctx.project_field_host(small, hip.make_field_projection(op=hip.PROJECT_MIN, **pk), lut, totals=False)[5]
        kw["range"] = (int(low["vmin"]), max(int(top["vmax"]), int(low["vmin"]) + 1))
    alpha = np.clip(a.opacity // 4 + (np.arange(256) * (a.opacity - a.opacity // 4)) // 255, 0, 255).astype(np.uint32)
    lut = (lut & np.uint32(0x00ffffff)) | (alpha << np.uint32(24))
    sky = (0.55, 0.7, 0.9, 1.0)
    comp = hip.make_field_composite(stop_q16=a.stop, occlude=not a.see_through, background_rgba=sky, miss_rgba=sky, **kw)
    if a.over_lit:
        import torch
        n = f.width * f.height
        d_rgba = torch.empty(n * 4, dtype=torch.float32, device="cuda")
        d_lut = torch.from_numpy(lut.view(np.int32)).cuda()
        d_summary = torch.zeros(4, dtype=torch.int64, device="cuda")
        ctx.render_lit_device(f, hip.make_lighting(), d_rgba.data_ptr())
        ctx.composite_field_device(f, comp, d_lut.data_ptr(), d_rgba.data_ptr(), d_under=d_rgba.data_ptr(), d_summary=d_summary.data_ptr())
        torch.cuda.synchronize()
        rgba = d_rgba.cpu().numpy().reshape(f.height, f.width, 4)
        summary = d_summary.cpu().numpy().view(hip.COMPOSITE_SUMMARY_DTYPE)[0]
    else:
        rgba, _, _, _, _, summary = ctx.composite_field_host(f, comp, lut)
    legend = {name: int(summary[name]) for name in hip.COMPOSITE_SUMMARY_DTYPE.names}
    legend.update(range=[int(comp.range_lo), int(comp.range_hi)], scale=int(comp.scale), stop_q16=int(comp.stop_q16), occlude=int(comp.occlude),
                  over_lit=bool(a.over_lit), lut_rgba=lut.view(np.uint8).reshape(256, 4).tolist(), ms=list(ctx.last_composite_ms()))
    return rgba, legend


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="calgary")
    ap.add_argument("--field", default="sky")
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--mode", choices=("first", "closest"), default="closest")
    ap.add_argument("--clip", type=float, default=None, help="keep the grid below this fraction of its x extent")
    ap.add_argument("--flat", action="store_true", help="no Lambert shading")
    ap.add_argument("--project", choices=("max", "min", "mean", "count", "first"), default=None,
                    help="a projection along the pixel rays instead of a view of the surface")
    ap.add_argument("--window", type=int, nargs=2, default=None, metavar=("LO", "HI"), help="with --project: the values that count")
    ap.add_argument("--composite", action="store_true", help="the field as a volume seen through, composited front to back")
    ap.add_argument("--over-lit", action="store_true", help="with --composite: over the lit frame, in place on the device")
    ap.add_argument("--see-through", action="store_true", help="with --composite: the rays pass the solids")
    ap.add_argument("--opacity", type=int, default=24, help="with --composite: the largest alpha byte of the LUT")
    ap.add_argument("--stop", type=int, default=256, help="with --composite: stop_q16")
    ap.add_argument("--range", type=int, nargs=2, default=None, metavar=("LO", "HI"), help="with --composite: the colours' range")
    ap.add_argument("--sources", nargs="+", default=None, metavar="I,J,K,W", help="with --field dose: the point sources")
    ap.add_argument("--transmit", type=int, nargs="+", default=None, help="with --field dose: the Q16 transmission table")
    ap.add_argument("--reach", type=int, default=None, help="with --field dose: the reach in voxels")
    ap.add_argument("--no-falloff", action="store_true", help="with --field dose: no inverse-square falloff")
    ap.add_argument("--out", default="field_view.ppm")
    a = ap.parse_args()
    grid, cam, up = scene(a.scene)
    ctx = rto.Context(0)
    ctx.build_octree(grid.data, grid.min, grid.voxelSize)
    if a.field == "dose" and not a.sources:
        raise SystemExit("--field dose needs --sources I,J,K,W ...")
    kw = {} if a.field == "dose" else make_field(ctx, a.field, up, grid.voxelSize)
    dx, dy, dz = grid.dims
    if a.clip is not None:
        kw["clip"] = ((0, 0, 0), (max(1, min(dx, int(round(a.clip * dx)))), dy, dz))
    lut = hip.ramp_lut(HEAT)
    W, H = a.width, a.height
    f = rto.make_frame(cam.getView(), cam.getPos(), W / H, 45.0, W, H)
    if a.field == "dose":
        rgba, legend = dose_frame(ctx, f, a, lut, kw)
        write_ppm(a.out, rgba)
        legend.update(scene=a.scene, field=a.field, frame=[W, H], project=a.project, composite=bool(a.composite))
        with open(os.path.splitext(a.out)[0] + ".legend.json", "w") as fh:
            json.dump(legend, fh)
        print(f"{a.out}: {W}x{H}, dose of {len(a.sources)} sources: {legend['seen']} of {legend['evaluated']} voxels see one, peak {legend['peak']}")
        ctx.close()
        return
    if a.composite:
        rgba, legend = composite(ctx, f, kw, lut, a)
        write_ppm(a.out, rgba)
        legend.update(scene=a.scene, field=a.field, frame=[W, H])
        with open(os.path.splitext(a.out)[0] + ".legend.json", "w") as fh:
            json.dump(legend, fh)
        print(f"{a.out}: {W}x{H}, {legend['visited']} pixels visit the volume, {legend['contributing']} show it, {legend['saturated']} "
              f"saturated, {legend['occluded']} stopped by a solid")
        ctx.close()
        return
    if a.project:
        kw.pop("sample", None)
        if a.window:
            kw["valid"] = tuple(a.window)
        op = {"max": hip.PROJECT_MAX, "min": hip.PROJECT_MIN, "mean": hip.PROJECT_MEAN, "count": hip.PROJECT_COUNT, "first": hip.PROJECT_FIRST}[a.project]
        if op == hip.PROJECT_COUNT:
            kw.update(scale=hip.SCALE_LINEAR, range=(0, 0))
        view = hip.make_field_projection(op=op, miss_rgba=(0.55, 0.7, 0.9, 1.0), none_rgba=(0.3, 0.3, 0.3, 1.0), **kw)
        rgba, values, _, _, _, summary, bins = ctx.project_field_host(f, view, lut, totals=False)
        ms = list(ctx.last_projection_ms())
    else:
        kw["mode"] = hip.QUERY_FIRST if a.mode == "first" else hip.QUERY_CLOSEST
        view = hip.make_field_view(shade=not a.flat, miss_rgba=(0.55, 0.7, 0.9, 1.0), none_rgba=(0.3, 0.3, 0.3, 1.0), **kw)
        rgba, values, summary, bins = ctx.render_field_host(f, view, lut)
        ms = list(ctx.last_field_view_ms())
    write_ppm(a.out, rgba)
    legend = {"scene": a.scene, "field": a.field, "frame": [W, H], "hits": int(summary["hits"]), "valued": int(summary["valued"]),
              "vmin": int(summary["vmin"]), "vmax": int(summary["vmax"]), "range": [int(summary["lo"]), int(summary["hi"])],
              "scale": int(view.scale), "bins": bins.tolist(), "lut_rgba": lut.view(np.uint8).reshape(256, 4).tolist(),
              "project": a.project, "ms": ms}
    with open(os.path.splitext(a.out)[0] + ".legend.json", "w") as fh:
        json.dump(legend, fh)
    print(f"{a.out}: {W}x{H}, {legend['hits']} hit pixels, {legend['valued']} with a value in [{legend['vmin']}, {legend['vmax']}], "
          f"{int((bins > 0).sum())} of 256 legend bins in use")
    ctx.close()


if __name__ == "__main__":
    main()
