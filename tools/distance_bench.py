#!/usr/bin/env python3
"""Distance fields and morphology on one GPU (rto_distance_field, rto_edit_morphology): one JSON line per scene and case.

Scenes: config 5's 512^3 test sphere and Calgary (tests/golden/ref_scene_cache.npz).  Every volume is compared with the CPU answer
(the host layer's distanceFieldCPU / applyMorphologyCPU) before anything is timed.  Cases, each a median over --rounds calls in one
process after one warm-up call:
  field    SOLID, uncapped and capped at 4 voxels: device ms per pass (rto_last_distance_ms: x, y, z, summary) and each pass as a fraction of the copy floor
  morph    the four ops at radii of 1.5 and 4 voxels, each from the scene as loaded (the untimed rebuild of the scene in between):
           device ms of transforms and flips, octree rebuild, triangle rebuild (rto_last_morphology_ms)
Comparators: `cpu_ms`, the host layer's transform on one core, once; `copy_ms`, a device-to-device copy of an int32 volume of the
grid's size (three of them are the floor of a three-pass transform that reads and writes the volume once per pass); `brush_ms`,
one rto_edit_voxels sphere brush of 4 voxels on the same scene, whose rebuild is the same rebuild."""
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

OPS = {"dilate": hip.MORPH_DILATE, "erode": hip.MORPH_ERODE, "open": hip.MORPH_OPEN, "close": hip.MORPH_CLOSE}


def calgary():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_scene_cache.npz"))
    dims = tuple(int(x) for x in z["dims"])
    data = np.unpackbits(z["packed"])[: dims[0] * dims[1] * dims[2]].reshape(dims[2], dims[1], dims[0])
    return np.ascontiguousarray(data, np.uint8), z["min"].astype(np.float32), np.float32(z["voxel"])


def sphere(dim):
    g = orc.test_sphere_grid(dim)
    return np.ascontiguousarray(g.data, np.uint8), g.min, g.voxel_size


def copy_ms(nvox, rounds):
    """Device ms (events) of a device-to-device copy of nvox int32."""
    L = hip.load()
    L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    L.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.hipFree.argtypes = [C.c_void_p]
    L.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    L.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    L.hipEventSynchronize.argtypes = [C.c_void_p]
    L.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    L.hipEventDestroy.argtypes = [C.c_void_p]
    a, b, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.hipMalloc(C.byref(a), 4 * nvox) == 0 and L.hipMalloc(C.byref(b), 4 * nvox) == 0
    assert L.hipEventCreate(C.byref(e0)) == 0 and L.hipEventCreate(C.byref(e1)) == 0
    ts = []
    for k in range(rounds + 1):
        L.hipEventRecord(e0, None)
        assert L.hipMemcpyAsync(b, a, 4 * nvox, 3, None) == 0    # hipMemcpyDeviceToDevice
        L.hipEventRecord(e1, None)
        L.hipEventSynchronize(e1)
        ms = C.c_float()
        L.hipEventElapsedTime(C.byref(ms), e0, e1)
        ts.append(ms.value)
    for p in (a, b):
        L.hipFree(p)
    for e in (e0, e1):
        L.hipEventDestroy(e)
    return float(np.median(ts[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--scenes", default="sphere512,calgary")
    ap.add_argument("--radii", default="1.5,4")
    ap.add_argument("--cap", type=float, default=4.0, help="the capped field's cap, in voxels")
    a = ap.parse_args()
    ctx = hip.Context(0)
    for name in a.scenes.split(","):
        data, gmin, vox = calgary() if name == "calgary" else sphere(int(name[6:]))
        dims = data.shape[::-1]
        vg = rto.VoxelGrid.from_array(data, gmin, vox)
        floor = copy_ms(data.size, a.rounds)
        ctx.build_octree(data, gmin, vox)
        ctx.build_leaf_triangles(None)
        base = {"scene": name, "dims": list(dims), "copy_ms": round(floor, 4)}
        # ---- fields
        for cap in (None, a.cap):
            max_dist = np.inf if cap is None else np.float32(cap) * np.float32(vox)
            mq = -1 if cap is None else int(np.floor(cap * 64.0 + 0.5))
            t0 = time.perf_counter()
            want, want_summary = vg.distanceField(hip.SET_SOLID, mq)
            cpu = (time.perf_counter() - t0) * 1e3
            got, gs = ctx.distance_field(hip.SET_SOLID, max_dist)    # the warm-up call, and the comparison
            if not np.array_equal(got, want) or gs.tobytes() != want_summary.tobytes():
                raise SystemExit(f"{name} cap {cap}: the field differs from the CPU answer")
            ms = []
            for k in range(a.rounds):
                ctx._check(ctx._L.rto_distance_field(ctx._h, hip.SET_SOLID, float(max_dist), gs.ctypes.data))
                ms.append(ctx.last_distance_ms())
            m = np.median(np.asarray(ms, np.float64), axis=0)
            r = dict(base, case="field", set="solid", cap_voxels=cap, x_ms=round(float(m[0]), 4), y_ms=round(float(m[1]), 4),
                     z_ms=round(float(m[2]), 4), summary_ms=round(float(m[3]), 4), cpu_ms=round(cpu, 1),
                     floor_fraction=[round(floor / float(t), 3) for t in m[:3]], max_d2=int(gs["max_d2"]))
            print(json.dumps(r), flush=True)
        # ---- one brush of the same size: the rebuild is the same rebuild
        centre = (np.asarray(gmin, np.float64) + np.asarray(dims, np.float64) / 2 * float(vox)).astype(np.float32)
        brush = hip.make_brushes([centre], float(np.float32(4.0) * np.float32(vox)), hip.BRUSH_SPHERE, hip.EDIT_CARVE)
        bm = []
        for k in range(a.rounds + 1):
            ctx.build_octree(data, gmin, vox)
            ctx.build_leaf_triangles(None)
            ctx.edit_voxels(brush)
            bm.append(ctx.last_edit_ms())
        bm = np.median(np.asarray(bm[1:], np.float64), axis=0)
        print(json.dumps(dict(base, case="brush", brush_ms=round(float(bm[0]), 4), rebuild_ms=round(float(bm[1]), 4),
                              triangles_ms=round(float(bm[2]), 4))), flush=True)
        # ---- morphology
        for radius in (float(x) for x in a.radii.split(",")):
            rq = int(np.floor(radius * 64.0 + 0.5))
            for opname, op in OPS.items():
                cpu_grid = rto.VoxelGrid.from_array(data, gmin, vox)
                t0 = time.perf_counter()
                want_changed = cpu_grid.applyMorphology(op, rq)
                cpu = (time.perf_counter() - t0) * 1e3
                ms = []
                for k in range(a.rounds + 1):
                    ctx.build_octree(data, gmin, vox)
                    ctx.build_leaf_triangles(None)
                    changed = ctx.edit_morphology(op, float(np.float32(radius) * np.float32(vox)))
                    if k == 0 and (changed != want_changed or not np.array_equal(ctx.download_voxels(), cpu_grid.data)):
                        raise SystemExit(f"{name} {opname} {radius}: the grid differs from the CPU answer")
                    ms.append(ctx.last_morphology_ms())
                m = np.median(np.asarray(ms[1:], np.float64), axis=0)
                print(json.dumps(dict(base, case="morph", op=opname, radius_voxels=radius, changed=int(want_changed),
                                      transform_ms=round(float(m[0]), 4), rebuild_ms=round(float(m[1]), 4),
                                      triangles_ms=round(float(m[2]), 4), cpu_ms=round(cpu, 1))), flush=True)


if __name__ == "__main__":
    main()
