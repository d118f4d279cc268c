#!/usr/bin/env python3
"""Times field projections (rto_project_field_device) against two yardsticks this feature does not touch.

    python3 tools/projection_bench.py [--scenes config2,calgary,config5] [--rounds 5] [--out profiles/projection_bench.jsonl]

Scenes: config 2 (the 256^3 test sphere at 1920 x 1080), calgary (the shipped city grid at 1920 x 1080) and config 5 (the 512^3
sphere at 3840 x 2160).  The field is the distance to EMPTY.  Kinds, all alternated inside every round of one process: MAX, MEAN
and FIRST (FIRST and a second MAX under a window above half the field's maximum), each with the brick table and without it
(rto_debug_set_projection_table); the field view of section 27 under FIRST from the same camera; a device-to-device copy of the
volume.  Every time is a pair of device events (rto_last_projection_ms, rto_last_field_view_ms, torch events around the copy);
one warm-up round, then the median of --rounds rounds.  One JSON line per scene goes to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import ray_tracing_octrees_amd as rto
from ray_tracing_octrees_amd import hip


def scene(name):
    if name == "calgary":
        z = np.load(os.path.join(ROOT, "tests", "golden", "ref_scene_cache.npz"))
        dims = tuple(int(x) for x in z["dims"])
        data = np.unpackbits(z["packed"])[: dims[0] * dims[1] * dims[2]].reshape(dims[2], dims[1], dims[0])
        return rto.VoxelGrid.from_array(data, z["min"].astype(np.float32), np.float32(z["voxel"])), rto.Camera(0.6, 0.5, 3500.0), 1920, 1080
    if name == "config2":
        return rto.VoxelGrid.test_sphere(256), rto.Camera(0.5, 0.7, 1.8), 1920, 1080
    if name == "config5":
        return rto.VoxelGrid.test_sphere(512), rto.Camera(0.5, 0.7, 1.8), 3840, 2160
    raise SystemExit(f"unknown scene {name}")


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="config2,calgary,config5")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "projection_bench.jsonl"))
    a = ap.parse_args()
    lines = []
    for name in a.scenes.split(","):
        grid, cam, W, H = scene(name)
        ctx = rto.Context(0)
        ctx.build_octree(grid.data, grid.min, grid.voxelSize)
        _, summary = ctx.distance_field(hip.SET_EMPTY)
        dmax = int(summary["max_d2"])
        d_field = ctx.distance_device()
        nvox = int(np.prod(grid.dims))
        f = rto.make_frame(cam.getView(), cam.getPos(), W / H, 45.0, W, H)
        d_lut = torch.from_numpy(hip.ramp_lut([(0, 0, 0, 255), (255, 255, 255, 255)]).view(np.int32)).cuda()
        d_rgba = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
        d_values = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        d_copy = torch.empty(nvox, dtype=torch.int32, device="cuda")
        src = torch.empty(nvox, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        half = (dmax // 2 + 1, 0x7ffffffe)
        kinds = {"max": (hip.PROJECT_MAX, (1, 0x7ffffffe)), "mean": (hip.PROJECT_MEAN, (1, 0x7ffffffe)),
                 "max_half": (hip.PROJECT_MAX, half), "first_half": (hip.PROJECT_FIRST, half)}
        times = {}
        valued = {}

        def project(kind, table):
            op, valid = kinds[kind]
            ctx.debug_set_projection_table(table)
            v = hip.make_field_projection(hip.FIELD_DISTANCE, op, scale=hip.SCALE_SQRT, valid=valid)
            ctx.project_field_device(f, v, d_lut.data_ptr(), d_rgba.data_ptr(), d_values=d_values.data_ptr())
            ms = ctx.last_projection_ms()
            times.setdefault(f"{kind}/{'table' if table else 'plain'}", []).append(ms)
            valued[kind] = int((d_values > hip.FIELD_PIXEL_NONE).sum().item())

        def field_view():
            v = hip.make_field_view(hip.FIELD_DISTANCE, mode=hip.QUERY_FIRST, scale=hip.SCALE_SQRT)
            ctx.render_field_device(f, v, d_lut.data_ptr(), d_rgba.data_ptr(), d_values=d_values.data_ptr())
            times.setdefault("field_view_first", []).append(ctx.last_field_view_ms())

        def copy():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            d_copy.copy_(src)
            e1.record()
            e1.synchronize()
            times.setdefault("copy_d2d", []).append((e0.elapsed_time(e1),))

        for r in range(a.rounds + 1):
            for kind in kinds:
                for table in (True, False):
                    project(kind, table)
            field_view()
            copy()
            if r == 0:
                times.clear()                       # the warm-up round
        ctx.debug_set_projection_table(True)
        med = {k: [round(statistics.median(x[i] for x in v), 4) for i in range(len(v[0]))] for k, v in times.items()}
        line = {"scene": name, "grid": list(grid.dims), "frame": [W, H], "field": "distance to EMPTY", "max_d2": dmax, "window_half": list(half),
                "rounds": a.rounds, "valued_pixels": valued, "unit": "ms, device events, median; projections: [bricks, march, shade]; "
                "field_view_first: [sample, shade]; copy_d2d: one copy of the int32 volume", "median_ms": med,
                "device": ctx.device_name}
        lines.append(line)
        print(json.dumps(line))
        ctx.close()
        del d_copy, src
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
