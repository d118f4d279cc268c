#!/usr/bin/env python3
"""Component measures on one GPU (rto_measure_components): one JSON line per scene, set and connectivity.

Scenes: config 5's 512^3 test sphere and Calgary (tests/golden/ref_scene_cache.npz), both sets, both connectivities.  Every table
and total is compared with the CPU answer (the host layer's measureComponentsCPU on the downloaded labels) before anything is
timed.  Per case, medians over --rounds calls in one process after one warm-up call: device ms of the call's two phases
(rto_last_measure_ms: the memset and the measuring kernels; the Euler numbers and the total).  Yardsticks in the same run:
`copy_ms`, a device-to-device copy of an int32 volume of the grid's size: the traffic floor, since the kernel reads the label
volume once; `stats_ms`, the statistics phase of rto_last_components_ms on the same labelling (median over the same number of
labellings): the existing pass of the same kind; `cpu_ms`, measureComponentsCPU on one core, once."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from ray_tracing_octrees_amd import hip, host
from thickness_bench import calgary, copy_ms, sphere


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--scenes", default="sphere512,calgary")
    ap.add_argument("--no-cpu", action="store_true", help="skip the comparison with, and the timing of, the CPU form")
    a = ap.parse_args()
    ctx = hip.Context(0)
    for name in a.scenes.split(","):
        data, gmin, vox = calgary() if name == "calgary" else sphere(int(name[6:]))
        dims = data.shape[::-1]
        floor = copy_ms(data.size, a.rounds)
        ctx.build_octree(data, gmin, vox)
        base = {"scene": name, "dims": list(dims), "copy_ms": round(floor, 4)}
        for s in (hip.SET_SOLID, hip.SET_EMPTY):
            for conn in (hip.CONN_FACE, hip.CONN_FULL):
                stats = []
                for k in range(a.rounds):
                    comps = ctx.label_components(s, conn)
                    stats.append(ctx.last_components_ms()[3])
                table, total = ctx.measure_components()                    # the warm-up call, and the comparison
                cpu = None
                if not a.no_cpu:
                    labels = ctx.component_labels()
                    t0 = time.perf_counter()
                    rc, want, want_total = host.measureComponentsCPU(labels, len(comps), conn)
                    cpu = (time.perf_counter() - t0) * 1e3
                    if rc != 0 or want.tobytes() != table.tobytes() or want_total.tobytes() != total.tobytes():
                        raise SystemExit(f"{name} set {s} connectivity {conn}: the measures differ from the CPU answer")
                    del labels, want
                ms = []
                for k in range(a.rounds):
                    ctx._check(ctx._L.rto_measure_components(ctx._h, total.ctypes.data))
                    ms.append(ctx.last_measure_ms())
                m = np.median(np.asarray(ms, np.float64), axis=0)
                print(json.dumps(dict(base, case="measure", set="solid" if s == hip.SET_SOLID else "empty", connectivity=conn,
                                      components=len(comps), voxels=int(total["voxels"]), faces=int(total["faces"].sum()),
                                      euler=int(total["euler"]), measure_ms=round(float(m[0]), 4), total_ms=round(float(m[1]), 4),
                                      stats_ms=round(float(np.median(stats)), 4), cpu_ms=None if cpu is None else round(cpu, 1))),
                      flush=True)


if __name__ == "__main__":
    main()
