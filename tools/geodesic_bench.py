#!/usr/bin/env python3
"""Geodesic distance fields on one GPU (rto_geodesic_field): one JSON line per scene and case.

Scenes: config 5's 512^3 test sphere (EMPTY medium, seed at voxel 0, FACE and FULL, no limit and limit 64), Calgary
(tests/golden/ref_scene_cache.npz; EMPTY medium, seed at the first free voxel of the ground layer) and a 256^3 serpentine maze
(tests/geodesic_ref.py's generator: the case where a path re-enters tiles many times).  Every field and summary is compared with
the CPU answer (the host layer's geodesicFieldCPU, a bucket queue) before anything is timed.  Per case, medians over --rounds
calls in one process after one warm-up call: relaxation launches, tiles run summed over them, and device ms of init, relaxation
and summary (rto_last_geodesic_ms).
Comparators in the same run: `cpu_ms`, the host layer's bucket queue on one core, once; `label_ms`, rto_label_components of the same
set and connectivity (the same reachability without the values; the sum of its four phases); `copy_ms`, a device-to-device copy of
an int32 volume of the grid's size."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import ray_tracing_octrees_amd as rto
from oracle import orc   # the scene generator the tests and bench.py use
from ray_tracing_octrees_amd import hip
import geodesic_ref      # the maze generator only


def calgary():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_scene_cache.npz"))
    dims = tuple(int(x) for x in z["dims"])
    data = np.unpackbits(z["packed"])[: dims[0] * dims[1] * dims[2]].reshape(dims[2], dims[1], dims[0])
    return np.ascontiguousarray(data, np.uint8), z["min"].astype(np.float32), np.float32(z["voxel"])


def sphere(dim):
    g = orc.test_sphere_grid(dim)
    return np.ascontiguousarray(g.data, np.uint8), g.min, g.voxel_size


def maze(dim):
    return geodesic_ref.maze(dim, dim, dim), np.zeros(3, np.float32), np.float32(1.0 / dim)


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
    ap.add_argument("--scenes", default="sphere512,calgary,maze256")
    ap.add_argument("--limit", type=int, default=64, help="the limited field's limit on the sphere, in the metric's units")
    a = ap.parse_args()
    ctx = hip.Context(0)
    for name in a.scenes.split(","):
        if name == "calgary":
            data, gmin, vox = calgary()
            seed = int(np.flatnonzero(data[0].reshape(-1) == 0)[0])      # the first free voxel of the ground layer
            cases = [(hip.CONN_FACE, None), (hip.CONN_FULL, None)]
        elif name.startswith("maze"):
            data, gmin, vox = maze(int(name[4:]))
            seed = 0
            cases = [(hip.CONN_FACE, None)]
        else:
            data, gmin, vox = sphere(int(name[6:]))
            seed = 0
            cases = [(hip.CONN_FACE, None), (hip.CONN_FACE, a.limit), (hip.CONN_FULL, None), (hip.CONN_FULL, a.limit)]
        dims = data.shape[::-1]
        vg = rto.VoxelGrid.from_array(data, gmin, vox)
        floor = copy_ms(data.size, a.rounds)
        ctx.build_octree(data, gmin, vox)
        base = {"scene": name, "dims": list(dims), "seed": seed, "copy_ms": round(floor, 4)}
        label_ms = {}
        for conn, limit in cases:
            lim = hip.GEO_NO_LIMIT if limit is None else limit
            t0 = time.perf_counter()
            rc, want, want_summary = vg.geodesicField([seed], hip.SET_EMPTY, conn, lim)
            cpu = (time.perf_counter() - t0) * 1e3
            assert rc == 0
            got, gs = ctx.geodesic_field([seed], hip.SET_EMPTY, conn, limit)    # the warm-up call, and the comparison
            if not np.array_equal(got, want) or gs.tobytes() != want_summary.tobytes():
                raise SystemExit(f"{name} conn {conn} limit {limit}: the field differs from the CPU answer")
            del got, want
            s = np.asarray([seed], np.int64)
            ms, counts = [], []
            for k in range(a.rounds):
                ctx._check(ctx._L.rto_geodesic_field(ctx._h, hip.SET_EMPTY, conn, s.ctypes.data, 1, lim, gs.ctypes.data))
                ms.append(ctx.last_geodesic_ms())
                counts.append(ctx.geodesic_passes(tiles=True))
            m = np.median(np.asarray(ms, np.float64), axis=0)
            c = np.median(np.asarray(counts, np.float64), axis=0)
            if conn not in label_ms:
                ts = []
                for k in range(a.rounds + 1):
                    ctx.label_components(hip.SET_EMPTY, conn)
                    ts.append(sum(ctx.last_components_ms()))
                label_ms[conn] = float(np.median(ts[1:]))
            print(json.dumps(dict(base, case="field", medium="empty", connectivity=conn, limit=limit, passes=int(c[0]), tiles_run=int(c[1]),
                                  init_ms=round(float(m[0]), 4), relax_ms=round(float(m[1]), 4), summary_ms=round(float(m[2]), 4),
                                  cpu_ms=round(cpu, 1), label_ms=round(label_ms[conn], 4), max_g=int(gs["max_g"]),
                                  reached=int(gs["reached"]))), flush=True)


if __name__ == "__main__":
    main()
