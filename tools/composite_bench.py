#!/usr/bin/env python3
"""Times field composites (rto_composite_field_device) against yardsticks this feature does not touch.

    python3 tools/composite_bench.py [--scenes config2,calgary,config5] [--rounds 5] [--out profiles/composite_bench.jsonl]

Scenes: config 2 (the 256^3 test sphere at 1920 x 1080), calgary (the shipped city grid at 1920 x 1080) and config 5 (the 512^3
sphere at 3840 x 2160).  Two fields per scene, one after the other (a context holds one distance field): the distance to EMPTY
(inside the solids, as tools/projection_bench.py measures it) and the distance to SOLID (the air field).  Composites, all
alternated inside every round of one process, each with the tables and without them (rto_debug_set_projection_table):

    fog          alpha bytes 1 .. 8 over the whole range: every valued voxel contributes, nothing saturates
    half         alpha 0 below half the field's maximum, 255 above: the first voxel above half ends the ray
    opaque       alpha 255 everywhere: the first valued voxel ends the ray

on the solid field without occlusion, and on the air field with occlude = 1 and with occlude = 0.  Yardsticks on the same scene and
camera: section 28's MEAN with totals (it walks every valued brick) and FIRST above half the maximum, section 27's field view, and
a device-to-device copy of the grid's bytes (what the solid table's pass reads).  Every time is a pair of device events
(rto_last_composite_ms, rto_last_projection_ms, rto_last_field_view_ms, torch events around the copy); one warm-up round, then the
median of --rounds rounds.  One JSON line per scene goes to --out."""
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

from projection_bench import scene


def luts(torch):
    rgb = hip.ramp_lut([(12, 7, 60, 255), (200, 60, 90, 255), (252, 250, 180, 255)]) & np.uint32(0x00ffffff)
    i = np.arange(256)
    alpha = {"fog": 1 + i // 32, "half": np.where(i >= 128, 255, 0), "opaque": np.full(256, 255)}
    return {k: torch.from_numpy((rgb | (a.astype(np.uint32) << np.uint32(24))).view(np.int32)).cuda() for k, a in alpha.items()}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="config2,calgary,config5")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "composite_bench.jsonl"))
    a = ap.parse_args()
    lines = []
    for name in a.scenes.split(","):
        grid, cam, W, H = scene(name)
        ctx = rto.Context(0)
        ctx.build_octree(grid.data, grid.min, grid.voxelSize)
        nvox = int(np.prod(grid.dims))
        f = rto.make_frame(cam.getView(), cam.getPos(), W / H, 45.0, W, H)
        d_lut = luts(torch)
        d_rgba = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
        d_counts = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        d_sums = torch.zeros(W * H, dtype=torch.int64, device="cuda")
        d_summary = torch.zeros(4, dtype=torch.int64, device="cuda")
        src = torch.zeros(nvox, dtype=torch.uint8, device="cuda")
        dst = torch.empty(nvox, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        times, facts = {}, {}

        def composite(field, kind, occlude, dmax, table):
            ctx.debug_set_projection_table(table)
            # LINEAR over (0, dmax): index 128 is half the maximum
            v = hip.make_field_composite(hip.FIELD_DISTANCE, valid=(1, 0x7ffffffe), range=(0, dmax), occlude=occlude, stop_q16=0)
            ctx.composite_field_device(f, v, d_lut[kind].data_ptr(), d_rgba.data_ptr(), d_counts=d_counts.data_ptr(), d_summary=d_summary.data_ptr())
            key = f"{field}/{kind}/{'occlude' if occlude else 'through'}/{'table' if table else 'plain'}"
            times.setdefault(key, []).append(ctx.last_composite_ms())
            s = d_summary.cpu().numpy().view(hip.COMPOSITE_SUMMARY_DTYPE)[0]
            facts[key] = {n: int(s[n]) for n in hip.COMPOSITE_SUMMARY_DTYPE.names} | {"contributions": int(d_counts.sum().item())}

        def yardsticks(field, dmax):
            half = (dmax // 2 + 1, 0x7ffffffe)
            for kind, op, valid, totals in (("mean_totals", hip.PROJECT_MEAN, (1, 0x7ffffffe), True), ("first_half", hip.PROJECT_FIRST, half, False)):
                ctx.debug_set_projection_table(True)
                p = hip.make_field_projection(hip.FIELD_DISTANCE, op, valid=valid, range=(0, dmax))
                ctx.project_field_device(f, p, d_lut["opaque"].data_ptr(), d_rgba.data_ptr(), d_sums=d_sums.data_ptr() if totals else 0,
                                         d_counts=d_counts.data_ptr() if totals else 0)
                times.setdefault(f"{field}/projection_{kind}", []).append(ctx.last_projection_ms())
            if field == "solid":
                v = hip.make_field_view(hip.FIELD_DISTANCE, mode=hip.QUERY_FIRST, range=(0, dmax))
                ctx.render_field_device(f, v, d_lut["opaque"].data_ptr(), d_rgba.data_ptr())
                times.setdefault("solid/field_view_first", []).append(ctx.last_field_view_ms())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            e1.synchronize()
            times.setdefault("copy_d2d_grid_bytes", []).append((e0.elapsed_time(e1),))

        maxima = {}
        for field, which, occludes in (("solid", hip.SET_EMPTY, (0,)), ("air", hip.SET_SOLID, (1, 0))):
            _, summary = ctx.distance_field(which)
            dmax = maxima[field] = int(summary["max_d2"])
            print(f"{name}: {field} field made, max_d2 {dmax}", file=sys.stderr, flush=True)
            mark = {k: len(v) for k, v in times.items()}
            for r in range(a.rounds + 1):
                for kind in ("fog", "half", "opaque"):
                    for occlude in occludes:
                        for table in (True, False):
                            composite(field, kind, occlude, dmax, table)
                yardsticks(field, dmax)
                if r == 0:                              # the warm-up round of this field
                    for k in list(times):
                        del times[k][mark.get(k, 0):]
        ctx.debug_set_projection_table(True)
        med = {k: [round(statistics.median(x[i] for x in v), 4) for i in range(len(v[0]))] for k, v in times.items()}
        line = {"scene": name, "grid": list(grid.dims), "frame": [W, H], "fields": {"solid": "distance to EMPTY", "air": "distance to SOLID"},
                "max_d2": maxima, "rounds": a.rounds, "facts": facts,
                "unit": "ms, device events, median; composites: [tables, march, fold]; projections: [bricks, march, shade]; field_view_first: "
                        "[sample, shade]; copy_d2d_grid_bytes: one copy of the uint8 grid", "median_ms": med, "device": ctx.device_name}
        lines.append(line)
        print(json.dumps(line))
        ctx.close()
        del src, dst
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
