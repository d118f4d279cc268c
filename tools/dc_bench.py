#!/usr/bin/env python3
"""Dual contouring on one GPU (rto_extract_dual_contour): one JSON line per scene, also appended to
profiles/dc_bench.jsonl with --store.

Scenes: BASELINE config 5 (the 512^3 test sphere, whose voxel size needs RTO_DC_AREA_NONE) and the Calgary fixture
(tests/golden/ref_scene_cache.npz), both under RTO_DC_AREA_NONE; --reference-rule adds the reference's area rule.  Per scene:
  gpu_ms          the three rto_last_dual_contour_ms phases (count, rank, emit), medians of --rounds calls after a warm-up call
  gpu_wall_ms     wall time of the call (launches, the read-back of the count, the events), median
  floor_ms        1 B x voxels + 52 B x triangles at 6.3 TB/s (the float4-copy figure of section 16): every voxel read once, every
                  record and cell index written once
  emit_GBps       52 B x triangles over the emit phase
  iso_ms          the comparator on the GPU: section 30's isosurface of the squared distance to EMPTY at level 0.5 on the same scene
                  in the same process (count, rank, emit; the distance field itself is not timed), and its triangles
  cpu_ms          the comparator on the CPU: the host layer's dualContourVolume on this machine, one core, timed inside the library
Neither comparator is the code under test.  Exit status 1 if a GPU list differs from the CPU list in a byte."""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import ray_tracing_octrees_amd as rto
from ray_tracing_octrees_amd import hip, host

COPY_TBPS = 6.3


def calgary():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_scene_cache.npz"))
    dims = tuple(int(x) for x in z["dims"])
    data = np.unpackbits(z["packed"])[: dims[0] * dims[1] * dims[2]].reshape(dims[2], dims[1], dims[0])
    return rto.VoxelGrid.from_array(data, z["min"].astype(np.float32), np.float32(z["voxel"]))


def timed(call, last_ms, rounds):
    call()                                              # warm-up: buffers, code objects
    ms, wall = [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        summary = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(last_ms())
    return summary, np.median(np.array(ms), 0), float(np.median(wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--cpu-rounds", type=int, default=1)
    ap.add_argument("--dim", type=int, default=512, help="edge of the config-5 sphere")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU comparator (and the byte comparison)")
    ap.add_argument("--reference-rule", action="store_true", help="also time RTO_DC_AREA_REFERENCE")
    ap.add_argument("--store", action="store_true", help="append the lines to profiles/dc_bench.jsonl")
    args = ap.parse_args()
    ctx = rto.Context(args.gpu)
    bad = 0
    lines = []
    for scene, grid in ((f"config5_sphere{args.dim}", rto.VoxelGrid.test_sphere(args.dim)), ("config4_calgary", calgary())):
        ctx.build_octree(grid.data, grid.min, grid.voxelSize)
        voxels = int(np.prod(grid.data.shape))
        ctx.distance_field(hip.SET_EMPTY)
        iso_p = hip.make_iso_params(hip.FIELD_DISTANCE, 0.5, 0.0)
        iso_s, iso_ms, iso_wall = timed(lambda: ctx.extract_isosurface_count(iso_p), ctx.last_isosurface_ms, args.rounds)
        for rule in ([hip.DC_AREA_NONE, hip.DC_AREA_REFERENCE] if args.reference_rule else [hip.DC_AREA_NONE]):
            params = hip.make_dc_params(rule)
            summary, ms, wall = timed(lambda: ctx.extract_dual_contour_count(params), ctx.last_dual_contour_ms, args.rounds)
            tris, cell = ctx.download_dual_contour()
            n = int(summary.triangles)
            floor = (voxels + 52 * n) / (COPY_TBPS * 1e12) * 1e3
            r = {"scene": scene, "area_rule": "none" if rule == hip.DC_AREA_NONE else "reference", "device": ctx.device_name,
                 "dims": list(grid.data.shape[::-1]), "rounds": args.rounds, "tris": n, "faces": int(summary.faces),
                 "dropped": int(summary.dropped), "degenerate": int(summary.degenerate), "vertex_voxels": int(summary.vertex_voxels),
                 "gpu_ms": [round(float(x), 4) for x in ms], "gpu_total_ms": round(float(ms.sum()), 4), "gpu_wall_ms": round(wall, 4),
                 "floor_ms": round(floor, 4), "total_over_floor": round(float(ms.sum()) / floor, 2),
                 "count_floor_ms": round(voxels / (COPY_TBPS * 1e12) * 1e3, 4), "emit_floor_ms": round(52 * n / (COPY_TBPS * 1e12) * 1e3, 4),
                 "emit_GBps": round(52 * n / (float(ms[2]) * 1e-3) / 1e9, 1) if ms[2] > 0 and n else None,
                 "iso_tris": int(iso_s.triangles), "iso_ms": [round(float(x), 4) for x in iso_ms], "iso_total_ms": round(float(iso_ms.sum()), 4),
                 "iso_wall_ms": round(iso_wall, 4)}
            if not args.no_cpu:
                cpu = float(np.median([host.dualContourVolumeMs(grid.data, grid.min, grid.voxelSize, params)[0] for _ in range(args.cpu_rounds)]))
                t18, wcell, _ = host.dualContourVolume(grid.data, grid.min, grid.voxelSize, params)
                want = np.ascontiguousarray(t18[:, :12])
                r["cpu_ms"] = round(cpu, 1)
                r["cpu_over_gpu_wall"] = round(cpu / wall, 1)
                r["equal"] = bool(hashlib.sha256(want.tobytes()).digest() == hashlib.sha256(tris.tobytes()).digest() and np.array_equal(cell, wcell))
                bad += 0 if r["equal"] else 1
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if args.store:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "dc_bench.jsonl"), "a") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
