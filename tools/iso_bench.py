#!/usr/bin/env python3
"""Field isosurfaces on one GPU (rto_extract_isosurface_device): one JSON line per case, also appended to
profiles/iso_bench.jsonl with --store.

Cases: BASELINE config 5 (the 512^3 test sphere) and config 4 (the Calgary fixture, tests/golden/ref_scene_cache.npz): the squared
distance to EMPTY at level 2.5, and the thickness field of the solids (balls up to 8 voxels) at level 4.5; pad on, outside 0.  Per case:
  gpu_ms          the three rto_last_isosurface_ms phases (count with the brick table, rank, emit), median of --rounds calls
  gpu_wall_ms     wall time of the call (launches, the read-back of the count, the events), median
  no_table_ms     the same phases with rto_debug_set_projection_table(ctx, 0); table_ratio = total without / total with
  floor_ms        4 B x voxels + 52 B x triangles at 6.3 TB/s (the float4-copy figure of section 16): every sample read once, every
                  record and cell index written once
  emit_GBps       52 B x triangles over the emit phase
  mesh_emit_GBps  section 16's emit row on the same scene (rto_extract_mesh, MC, unculled: 100 B per triangle over its emit phase)
  cpu_ms          the host layer's isoSurfaceVolume on this machine, one core, timed inside the library (the comparator)
Exit status 1 if a GPU list differs from the CPU list in a byte, or the list without the table from the list with it."""
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


def timed(ctx, params, rounds):
    ctx.extract_isosurface_count(params)               # warm-up: buffers, code objects
    ms, wall = [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        summary = ctx.extract_isosurface_count(params)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(ctx.last_isosurface_ms())
    return summary, np.median(np.array(ms), 0), float(np.median(wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--cpu-rounds", type=int, default=1)
    ap.add_argument("--dim", type=int, default=512, help="edge of the config-5 sphere")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU comparator (and the byte comparison)")
    ap.add_argument("--store", action="store_true", help="append the lines to profiles/iso_bench.jsonl")
    args = ap.parse_args()
    ctx = rto.Context(args.gpu)
    bad = 0
    lines = []
    for scene, grid in ((f"config5_sphere{args.dim}", rto.VoxelGrid.test_sphere(args.dim)), ("config4_calgary", calgary())):
        ctx.build_octree(grid.data, grid.min, grid.voxelSize)
        ctx.build_leaf_triangles()
        ctx.extract_mesh_count(hip.MESH_MC)
        mesh_ms, mesh_n = [], 0
        for _ in range(args.rounds):
            mesh_n = ctx.extract_mesh_count(hip.MESH_MC)
            mesh_ms.append(ctx.last_mesh_ms()[2])
        mesh_emit = float(np.median(mesh_ms))
        voxels = int(np.prod(grid.data.shape))
        for cname, source, level, make in (("distance_2.5", hip.FIELD_DISTANCE, 2.5, lambda: ctx.distance_field(hip.SET_EMPTY)[0]),
                                           ("thickness_4.5", hip.FIELD_THICKNESS, 4.5,
                                            lambda: ctx.thickness_field(hip.SET_SOLID, 8.0 * float(grid.voxelSize))[0])):
            field = make()
            params = hip.make_iso_params(source, level, 0.0)
            ctx.debug_set_projection_table(True)
            summary, ms, wall = timed(ctx, params, args.rounds)
            tris, cell = ctx.download_isosurface()
            ctx.debug_set_projection_table(False)
            _, ms_off, _ = timed(ctx, params, args.rounds)
            tris_off, cell_off = ctx.download_isosurface()
            ctx.debug_set_projection_table(True)
            n = int(summary.triangles)
            floor = (4 * voxels + 52 * n) / (COPY_TBPS * 1e12) * 1e3
            r = {"scene": scene, "case": cname, "device": ctx.device_name, "dims": list(grid.data.shape[::-1]), "rounds": args.rounds,
                 "tris": n, "active_cells": int(summary.active_cells), "degenerate": int(summary.degenerate),
                 "gpu_ms": [round(float(x), 4) for x in ms], "gpu_total_ms": round(float(ms.sum()), 4), "gpu_wall_ms": round(wall, 4),
                 "no_table_ms": [round(float(x), 4) for x in ms_off], "table_ratio": round(float(ms_off.sum() / ms.sum()), 3),
                 "floor_ms": round(floor, 4), "total_over_floor": round(float(ms.sum()) / floor, 2),
                 "emit_GBps": round(52 * n / (float(ms[2]) * 1e-3) / 1e9, 1) if ms[2] > 0 and n else None,
                 "mesh_tris": int(mesh_n), "mesh_emit_ms": round(mesh_emit, 4),
                 "mesh_emit_GBps": round(100 * mesh_n / (mesh_emit * 1e-3) / 1e9, 1) if mesh_emit > 0 and mesh_n else None,
                 "table_equal": bool(tris.tobytes() == tris_off.tobytes() and np.array_equal(cell, cell_off))}
            bad += 0 if r["table_equal"] else 1
            if not args.no_cpu:
                cpu = float(np.median([host.isoSurfaceVolumeMs(field, grid.min, grid.voxelSize, params)[0] for _ in range(args.cpu_rounds)]))
                t18, wcell, _ = host.isoSurfaceVolume(field, grid.min, grid.voxelSize, params)
                want = np.ascontiguousarray(t18[:, :12])
                r["cpu_ms"] = round(cpu, 1)
                r["cpu_over_gpu_wall"] = round(cpu / wall, 1)
                r["equal"] = bool(hashlib.sha256(want.tobytes()).digest() == hashlib.sha256(tris.tobytes()).digest() and np.array_equal(cell, wcell))
                bad += 0 if r["equal"] else 1
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if args.store:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "iso_bench.jsonl"), "a") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
