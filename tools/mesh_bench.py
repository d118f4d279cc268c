#!/usr/bin/env python3
"""Mesh extraction on one GPU (rto_extract_mesh) against the host layer's CPU renderOctree: prints one JSON line.

Scenes: BASELINE config 5 (the 512^3 test sphere, Camera(0.5, 0.7, 1.8)) and config 4 (the Calgary fixture,
tests/golden/ref_scene_cache.npz, Camera(0.6, 0.5, 3500)).  For each, both kinds (MC: the resident leaf triangles; CUBES: the exposed
faces of the solid leaves), unculled and culled by the scene's camera (fov 45, aspect 16:9, margin 50 as renderOctree's default --
and margin 0, where a unit-scale scene is culled at all):
  gpu_ms          the three rto_last_mesh_ms phases (count + cull, ranking passes, the emit kernel), median of --rounds calls
  gpu_wall_ms     wall time of the call (launches, the read-back of the count, the events), median
  depth           of the octree: the ranking passes are at most 2 x depth launches
  emit_GBps       bytes the emit pass moves (MC: 48 read + 52 written per triangle; CUBES: 52 written per triangle plus a mask
                  byte and an offset per node) over its time
  cpu_ms          the host layer's renderOctree on this machine, one CPU core, timed inside the library around the walk alone as
                  the reference times its own (the comparator; the reference publishes nothing); median of --cpu-rounds walks
Exit status 1 if a GPU list differs from the CPU list in a byte."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import ray_tracing_octrees_amd as rto
from ray_tracing_octrees_amd import hip, host

ASPECT = 16.0 / 9.0


def calgary():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_scene_cache.npz"))
    dims = tuple(int(x) for x in z["dims"])
    data = np.unpackbits(z["packed"])[: dims[0] * dims[1] * dims[2]].reshape(dims[2], dims[1], dims[0])
    return rto.VoxelGrid.from_array(data, z["min"].astype(np.float32), np.float32(z["voxel"]))


def cpu_list(root, grid, kind, planes, margin, rounds):
    r = host.MarchingCubesRenderer() if kind == hip.MESH_MC else host.VoxelCubeRenderer()
    ms = float(np.median([host.renderOctreePlanesMs(root, grid, r, planes, margin)[0] for _ in range(rounds)]))
    t = host.renderOctreePlanes(root, grid, r, planes, margin)          # the list itself, for the byte comparison; not timed
    return np.ascontiguousarray(np.concatenate([t[:, :9], t[:, 9:12]], 1)), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--cpu-rounds", type=int, default=3)
    ap.add_argument("--dim", type=int, default=512, help="edge of the config-5 sphere")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU comparator (and the byte comparison)")
    args = ap.parse_args()
    ctx = rto.Context(args.gpu)
    out = {"device": ctx.device_name, "rounds": args.rounds, "scenes": {}}
    bad = 0
    for name, grid, cam in ((f"config5_sphere{args.dim}", rto.VoxelGrid.test_sphere(args.dim), rto.Camera(0.5, 0.7, 1.8)),
                            ("config4_calgary", calgary(), rto.Camera(0.6, 0.5, 3500.0))):
        ctx.build_octree(grid.data, grid.min, grid.voxelSize)
        ctx.build_leaf_triangles()
        nodes, depth = int(ctx.info().num_nodes), int(ctx.info().depth)
        planes = ctx.frustum_planes(cam.getView(), 45.0, ASPECT)
        root = None if args.no_cpu else rto.createOctreeFromVoxelGrid(grid)
        res = {"nodes": nodes, "depth": depth}
        for kname, kind in (("mc", hip.MESH_MC), ("cubes", hip.MESH_CUBES)):
            for cname, pl, margin in (("unculled", None, 50.0), ("culled_m50", planes, 50.0), ("culled_m0", planes, 0.0)):
                ctx.extract_mesh_count(kind, pl, margin)       # warm-up: level table, buffers, code objects
                ms, wall = [], []
                for _ in range(args.rounds):
                    t0 = time.perf_counter()
                    n = ctx.extract_mesh_count(kind, pl, margin)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    ms.append(ctx.last_mesh_ms())
                ms = np.median(np.array(ms), 0)
                moved = n * 100 if kind == hip.MESH_MC else n * 52 + nodes * 5
                r = {"tris": n, "gpu_ms": [round(float(x), 4) for x in ms], "gpu_wall_ms": round(float(np.median(wall)), 4),
                     "emit_GBps": round(moved / (float(ms[2]) * 1e-3) / 1e9, 1) if ms[2] > 0 and n else None}
                if root is not None:
                    want, cpu_ms = cpu_list(root, grid, kind, pl, margin, args.cpu_rounds)
                    got, _ = ctx.download_mesh()
                    r["cpu_ms"] = round(cpu_ms, 2)
                    r["equal"] = bool(got.tobytes() == want.tobytes())
                    bad += 0 if r["equal"] else 1
                res[f"{kname}_{cname}"] = r
        if root is not None:
            rto.freeOctree(root)
        out["scenes"][name] = res
    print(json.dumps(out))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
