#!/usr/bin/env python3
"""Connected-component labelling on one GPU (rto_label_components, rto_edit_components): one JSON line per scene and case.

Scenes: config 2's 256^3 test sphere, Calgary (tests/golden/ref_scene_cache.npz) and config 5's 512^3 test sphere.  Cases, each a
median over --rounds labellings in one process:
  label    SOLID / FACE and EMPTY / FACE: device ms of the four phases (rto_last_components_ms: tile-local labelling, merging,
           flatten + ranking, statistics), the merge launches, the component count and the wall time to the synchronised return
  carved   the same after a CARVE box two voxels thick through the grid's middle has cut the scene in two
  fill     fillCavities (EMPTY / FACE / ENCLOSED) on a closed box mesh voxelized into a --mesh-dim^3 grid: wall ms, voxels flipped
Comparators: `cpu_bfs_ms`, the host layer's breadth-first search (labelComponentsCPU) on one core, once per case (skipped above
--cpu-max voxels), and `copy_ms`, a device-to-device copy of a buffer the size of the label volume (4 bytes per voxel)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import ray_tracing_octrees_amd as rto
from oracle import orc   # the scene generator the tests and bench.py use
from ray_tracing_octrees_amd import hip


def calgary():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_scene_cache.npz"))
    dims = tuple(int(x) for x in z["dims"])
    data = np.unpackbits(z["packed"])[: dims[0] * dims[1] * dims[2]].reshape(dims[2], dims[1], dims[0])
    return np.ascontiguousarray(data, np.uint8), z["min"].astype(np.float32), np.float32(z["voxel"])


def sphere(dim):
    g = orc.test_sphere_grid(dim)
    return np.ascontiguousarray(g.data, np.uint8), g.min, g.voxel_size


def box_mesh(lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(hi if (i >> a) & 1 else lo)[a] for a in range(3)] for i in range(8)], np.float64)
    quads = [(0, 2, 6, 4), (1, 5, 7, 3), (0, 4, 5, 1), (2, 3, 7, 6), (0, 1, 3, 2), (4, 6, 7, 5)]
    return v, np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.int32)


def copy_ms(nvox, rounds):
    """Device ms of a device-to-device copy of nvox int32 (the floor for anything that writes the label volume once)."""
    L = hip.load()
    L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.hipFree.argtypes = [C.c_void_p]
    a, b = C.c_void_p(), C.c_void_p()
    assert L.hipMalloc(C.byref(a), 4 * nvox) == 0 and L.hipMalloc(C.byref(b), 4 * nvox) == 0
    L.hipDeviceSynchronize()
    ts = []
    for k in range(rounds + 1):
        t0 = time.perf_counter()
        assert L.hipMemcpy(b, a, 4 * nvox, 3) == 0            # hipMemcpyDeviceToDevice, synchronous
        L.hipDeviceSynchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    L.hipFree(a)
    L.hipFree(b)
    return float(np.median(ts[1:]))


def label_case(ctx, s, rounds):
    ms, wall = [], []
    n = 0
    for k in range(rounds + 1):                                 # round 0 warms the pool up and is dropped
        t0 = time.perf_counter()
        n = len(ctx.label_components(s, hip.CONN_FACE))
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(ctx.last_components_ms())
    m = np.median(np.asarray(ms[1:], np.float64), axis=0)
    return {"components": n, "passes": ctx.components_passes(), "local_ms": round(float(m[0]), 4), "merge_ms": round(float(m[1]), 4),
            "rank_ms": round(float(m[2]), 4), "stats_ms": round(float(m[3]), 4), "device_ms": round(float(m.sum()), 4),
            "wall_ms": round(float(np.median(wall[1:])), 4)}


def cpu_bfs_ms(data, gmin, vox, s):
    vg = rto.VoxelGrid.from_array(data, gmin, vox)
    t0 = time.perf_counter()
    vg.labelComponents(s, hip.CONN_FACE)
    return round((time.perf_counter() - t0) * 1e3, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--scenes", default="sphere256,calgary,sphere512")
    ap.add_argument("--mesh-dim", type=int, default=256)
    ap.add_argument("--cpu-max", type=int, default=1 << 28, help="largest grid (voxels) the CPU comparator runs on")
    a = ap.parse_args()
    ctx = hip.Context(0)
    for name in a.scenes.split(","):
        data, gmin, vox = calgary() if name == "calgary" else sphere(int(name[6:]))
        dims = data.shape[::-1]
        floor = round(copy_ms(data.size, a.rounds), 4)
        ctx.build_octree(data, gmin, vox)
        for state in ("label", "carved"):
            if state == "carved":
                centre = (np.asarray(gmin, np.float64) + np.asarray(dims, np.float64) / 2 * float(vox)).astype(np.float32)
                half = np.asarray(dims, np.float64) * float(vox)
                half[2] = 1.0 * float(vox)
                ctx.edit_voxels(hip.make_brushes([centre], [half.astype(np.float32)], hip.BRUSH_BOX, hip.EDIT_CARVE))
                data = ctx.download_voxels()
            for s, sname in ((hip.SET_SOLID, "solid"), (hip.SET_EMPTY, "empty")):
                r = {"scene": name, "dims": list(dims), "case": state, "set": sname, "connectivity": 6}
                r.update(label_case(ctx, s, a.rounds))
                r["copy_ms"] = floor
                r["cpu_bfs_ms"] = cpu_bfs_ms(data, gmin, vox, s) if data.size <= a.cpu_max else None
                print(json.dumps(r), flush=True)
    # fillCavities on a voxelized closed mesh
    n = a.mesh_dim
    vox = np.float32(1.0 / n)
    v, tris = box_mesh([0.2, 0.2, 0.2], [0.8, 0.8, 0.8])
    wall, changed = [], 0
    for k in range(a.rounds + 1):
        ctx.voxelize_mesh(v, tris, vox, grid=((n, n, n), np.zeros(3, np.float32), vox))       # untimed: the shell again
        t0 = time.perf_counter()
        changed = ctx.edit_components(hip.SET_EMPTY, hip.CONN_FACE, hip.SELECT_ENCLOSED)
        wall.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"scene": f"box mesh in {n}^3", "case": "fill", "changed": changed,
                      "wall_ms": round(float(np.median(wall[1:])), 4), "rebuild_ms": round(float(ctx.last_build_ms()[0]), 4)}), flush=True)


if __name__ == "__main__":
    main()
