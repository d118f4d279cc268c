#!/usr/bin/env python3
"""Field views (rto_render_field_device) against the lit render's no-terms frame; one JSON line per case.

Cases: BASELINE config 2's sphere (256^3, Camera(0.5, 0.7, 1.8)) at 1920x1080, the Calgary grid (Camera(0.6, 0.5, 3500)) at
1920x1080, config 5's sphere (512^3) at 3840x2160; fov 45.  The field is the distance to EMPTY (RTO_FIELD_DISTANCE), SQRT scale,
auto range, values and bins written.  Per case, alternated within every round of one process:
  lit        rto_render_lit_device, shadow = 0, K = 0: the yardstick (the same walk, no field)
  copy       a device-to-device copy of the rgba buffer
  first      the field view under FIRST, no clip box, unshaded
  first_shaded   the same with shade = 1
  closest    under CLOSEST
  clipped    FIRST with a clip box that keeps the half of the grid away from the camera in x
Times are device events around `reps` frames on one stream, medians of `rounds` rounds; sample_ms / shade_ms are
rto_last_field_view_ms of one FIRST frame.  `expected_at_most` = 1.5 lit + copy; `within` says whether `first` met it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import ray_tracing_octrees_amd as rto
from ray_tracing_octrees_amd import hip


def timed_ms(fn, reps, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / reps


def calgary():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_scene_cache.npz"))
    dims = tuple(int(x) for x in z["dims"])
    data = np.unpackbits(z["packed"])[: dims[0] * dims[1] * dims[2]].reshape(dims[2], dims[1], dims[0])
    return rto.VoxelGrid.from_array(data, z["min"].astype(np.float32), np.float32(z["voxel"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="64^3 spheres and 320x180 frames: a rehearsal, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_bench.jsonl"))
    a = ap.parse_args()
    ctx = rto.Context(0)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    full, uhd = ((320, 180), (640, 360)) if a.small else ((1920, 1080), (3840, 2160))
    cases = (("config2_sphere256_1080p", lambda: rto.VoxelGrid.test_sphere(64 if a.small else 256), rto.Camera(0.5, 0.7, 1.8), full),
             ("calgary_1080p", calgary, rto.Camera(0.6, 0.5, 3500.0), full),
             ("config5_sphere512_4k", lambda: rto.VoxelGrid.test_sphere(64 if a.small else 512), rto.Camera(0.5, 0.7, 1.8), uhd))
    lut = torch.from_numpy(hip.ramp_lut([(0, 0, 96, 255), (0, 200, 255, 255), (255, 255, 0, 255), (255, 32, 0, 255)]).view(np.int32)).cuda()
    lines = []
    for name, make, cam, (W, H) in cases:
        g = make()
        ctx.build_octree(g.data, g.min, g.voxelSize)
        ctx.distance_field(hip.SET_EMPTY)
        dz, dy, dx = g.data.shape
        view, pos = cam.getView(), cam.getPos()
        f = rto.make_frame(view, pos, W / H, 45.0, W, H)
        rgba = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
        other = torch.zeros_like(rgba)
        values = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        summary = torch.zeros(4, dtype=torch.int64, device="cuda")
        bins = torch.zeros(256, dtype=torch.int64, device="cuda")
        L = hip.make_lighting((-1.0, -1.0, -1.0), False, 0, 1.0, 0)
        cam_high = float(pos[0]) > float(g.min[0]) + 0.5 * dx * float(g.voxelSize)
        clip = ((0, 0, 0), (dx // 2, dy, dz)) if cam_high else ((dx // 2, 0, 0), (dx, dy, dz))
        kinds = {"first": hip.make_field_view(hip.FIELD_DISTANCE, scale=hip.SCALE_SQRT),
                 "first_shaded": hip.make_field_view(hip.FIELD_DISTANCE, scale=hip.SCALE_SQRT, shade=True),
                 "closest": hip.make_field_view(hip.FIELD_DISTANCE, scale=hip.SCALE_SQRT, mode=hip.QUERY_CLOSEST),
                 "clipped": hip.make_field_view(hip.FIELD_DISTANCE, scale=hip.SCALE_SQRT, clip=clip)}

        def field(v):
            return lambda: ctx.render_field_device(f, v, lut.data_ptr(), rgba.data_ptr(), 0, values.data_ptr(), summary.data_ptr(),
                                                   bins.data_ptr(), sp)

        def copy():
            with torch.cuda.stream(stream):
                other.copy_(rgba, non_blocking=True)

        runs = {"lit": lambda: ctx.render_lit_device(f, L, rgba.data_ptr(), 0, sp), "copy": copy}
        runs.update({k: field(v) for k, v in kinds.items()})
        for fn in runs.values():                                    # warm-up: ray tables, work buffers, allocator
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                times[k].append(timed_ms(fn, a.reps, stream))
        out = {"case": name, "frame": [W, H], "grid": [dx, dy, dz], "rounds": a.rounds, "reps": a.reps, "rehearsal": bool(a.small)}
        out.update({k + "_ms": float(np.median(v)) for k, v in times.items()})
        runs["first"]()
        stream.synchronize()
        out["sample_ms"], out["shade_ms"] = [float(x) for x in ctx.last_field_view_ms()]
        s = summary.cpu().numpy().view(hip.FIELD_VIEW_SUMMARY_DTYPE)[0]
        out["hits"], out["valued"], out["range"] = int(s["hits"]), int(s["valued"]), [int(s["lo"]), int(s["hi"])]
        out["expected_at_most_ms"] = 1.5 * out["lit_ms"] + out["copy_ms"]
        out["within"] = bool(out["first_ms"] <= out["expected_at_most_ms"])
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
        del rgba, other, values
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
