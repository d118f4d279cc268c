"""Mesh -> octree timing: rto_voxelize_mesh on the synthetic downtown (about 50 k triangles) at voxel 10, 5
and 2.5 and on a UV sphere in a FIXED 512^3 grid.  Per scene: the device ms per phase (rto_last_voxelize_ms: setup + scan, fill,
recentring reduction, octree build), the wall time of the call (median of --reps), and as a comparator the same grid made on the
host by tests/voxelize_ref.py (numpy, one thread) plus rto_build_octree.  One JSON line per scene.

    python tools/voxelize_bench.py [--reps 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import voxelize_ref as vr  # noqa: E402
from ray_tracing_octrees_amd import hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    ctx = hip.Context(0)
    town = vr.downtown()
    sphere = vr.uv_sphere(64, 128, 0.45)        # finer rings fail the rule's absolute 1e-7f cut (|denom| ~ (2 area)^2) everywhere
    s512 = ((512, 512, 512), np.full(3, -0.5, np.float32), np.float32(1.0 / 512))
    scenes = [("downtown_10", town, 10.0, None), ("downtown_5", town, 5.0, None), ("downtown_2.5", town, 2.5, None),
              ("uv_sphere_512", sphere, s512[2], s512)]
    for name, (xyz, tris), vox, grid in scenes:
        r = ctx.voxelize_mesh(xyz, tris, vox, grid=grid)                # warm-up (first use of the kernels and the memory pool)
        walls, phases = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r = ctx.voxelize_mesh(xyz, tris, vox, grid=grid)
            walls.append((time.perf_counter() - t0) * 1e3)
            phases.append(ctx.last_voxelize_ms())
        t0 = time.perf_counter()
        want = vr.voxelize(xyz, tris, vox, grid=grid)
        ctx.build_octree(want[0], want[2], want[3])
        host_ms = (time.perf_counter() - t0) * 1e3
        same = bool(np.array_equal(want[0], ctx.download_voxels()))
        ph = np.median(np.asarray(phases), axis=0)
        print(json.dumps({"scene": name, "faces": int(len(tris)), "dims": list(r.dims), "pairs": int(r.pairs), "filled": int(r.filled),
                          "device_ms": {"setup_scan": round(float(ph[0]), 4), "fill": round(float(ph[1]), 4),
                                        "recentre": round(float(ph[2]), 4), "octree": round(float(ph[3]), 4)},
                          "wall_ms_median": round(float(np.median(walls)), 3),
                          "host_numpy_plus_build_ms": round(host_ms, 1), "grids_equal": same}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
