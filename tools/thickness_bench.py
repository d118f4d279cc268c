#!/usr/bin/env python3
"""Local thickness fields on one GPU (rto_thickness_field): one JSON line per scene, medium and radius.

Scenes: config 5's 512^3 test sphere and Calgary (tests/golden/ref_scene_cache.npz), both media, at radii of 2, 4 and 8 voxels
(c = 4, 16, 64).  Every field, histogram and summary is compared with the CPU answer (the host layer's thicknessFieldCPU) before
anything is timed.  Per case, medians over --rounds calls in one process after one warm-up call: device ms of the call's own
transform, of the gather and of the summary (rto_last_thickness_ms), and the share of the 32 x 8 x 8 tiles that ran the gather's
loop (counted on the host from a capped rto_distance_field of the other set: the tiles that hold a voxel with 0 < D < c).
Comparators in the same run: `transform_ms`, the call's own transform; `copy_ms`, a device-to-device copy of an int32 volume of the
grid's size, read once and written once: the gather's floor when almost every tile leaves early; `cpu_ms`, thicknessFieldCPU on one
core, once."""
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

TILE = (8, 8, 32)        # (z, y, x): k_cc_local's tile


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


def tiles_looped(ctx, medium, radius, c):
    """(tiles that hold a voxel with 0 < D < c, tiles): the workgroups of k_thick_gather that load their halo and run the loop."""
    d2, _ = ctx.distance_field(1 - medium, radius)
    work = (d2 > 0) & (d2 < c)                                  # RTO_DIST_NONE clips to c
    del d2
    Z, Y, X = work.shape
    pad = [(0, (-n) % t) for n, t in zip(work.shape, TILE)]
    w = np.pad(work, pad)
    tz, ty, tx = (w.shape[0] // TILE[0], w.shape[1] // TILE[1], w.shape[2] // TILE[2])
    any_work = w.reshape(tz, TILE[0], ty, TILE[1], tx, TILE[2]).any(axis=(1, 3, 5))
    return int(any_work.sum()), int(any_work.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--scenes", default="sphere512,calgary")
    ap.add_argument("--radii", default="2,4,8", help="in voxels")
    ap.add_argument("--no-cpu", action="store_true", help="skip the comparison with, and the timing of, the CPU form")
    a = ap.parse_args()
    ctx = hip.Context(0)
    for name in a.scenes.split(","):
        data, gmin, vox = calgary() if name == "calgary" else sphere(int(name[6:]))
        dims = data.shape[::-1]
        vg = rto.VoxelGrid.from_array(data, gmin, vox)
        floor = copy_ms(data.size, a.rounds)
        ctx.build_octree(data, gmin, vox)
        base = {"scene": name, "dims": list(dims), "copy_ms": round(floor, 4)}
        for medium in (hip.SET_SOLID, hip.SET_EMPTY):
            for r_vox in (float(r) for r in a.radii.split(",")):
                radius = np.float32(r_vox) * np.float32(vox)
                mq = int(np.floor(float(radius) / float(np.float32(vox)) * 64.0 + 0.5))
                c = mq * mq // 4096
                got, gs = ctx.thickness_field(medium, radius)              # the warm-up call, and the comparison
                bins = ctx.thickness_histogram()
                cpu = None
                if not a.no_cpu:
                    t0 = time.perf_counter()
                    rc, want, want_bins, want_summary = vg.thicknessField(medium, mq)
                    cpu = (time.perf_counter() - t0) * 1e3
                    assert rc == 0
                    if not np.array_equal(got, want) or not np.array_equal(bins, want_bins) or gs.tobytes() != want_summary.tobytes():
                        raise SystemExit(f"{name} medium {medium} radius {r_vox}: the field differs from the CPU answer")
                    del want
                del got
                ms = []
                for k in range(a.rounds):
                    ctx._check(ctx._L.rto_thickness_field(ctx._h, medium, float(radius), gs.ctypes.data))
                    ms.append(ctx.last_thickness_ms())
                m = np.median(np.asarray(ms, np.float64), axis=0)
                looped, tiles = tiles_looped(ctx, medium, radius, c)
                print(json.dumps(dict(base, case="field", medium="solid" if medium == hip.SET_SOLID else "empty", radius_voxels=r_vox, c=c,
                                      transform_ms=round(float(m[0]), 4), gather_ms=round(float(m[1]), 4), summary_ms=round(float(m[2]), 4),
                                      cpu_ms=None if cpu is None else round(cpu, 1), tiles=tiles, tiles_looped=looped,
                                      min_t2=int(gs["min_t2"]), thin=int(gs["thin"]), medium_voxels=int(gs["medium"]))), flush=True)


if __name__ == "__main__":
    main()
