#!/usr/bin/env python3
"""Skeletons on one GPU (rto_skeleton_field): one JSON line per scene and case.

Scenes: config 5's 512^3 test sphere (the SOLID set under RTO_CONN_FULL: TOPOLOGY, CURVE, and TOPOLOGY with max_passes = 4) and
Calgary (tests/golden/ref_scene_cache.npz; its free space, the EMPTY set, under RTO_CONN_FULL and TOPOLOGY).  Every field and
summary is compared with the CPU answer (the host layer's skeletonFieldCPU) before anything is timed.  Per case, medians over
--rounds calls in one process after one warm-up call: passes that removed something, kernel launches, tiles run summed over the
sub-steps, and device ms of init, thinning and summary (rto_last_skeleton_ms).
Comparators in the same run: `cpu_ms`, host/Skeleton.cpp on one core, once; `label_ms`, rto_label_components of the same set and
connectivity (the sum of its four phases); `copy_ms`, a device-to-device copy of an int32 volume of the grid's size."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

import ray_tracing_octrees_amd as rto
from ray_tracing_octrees_amd import hip
from geodesic_bench import calgary, copy_ms, sphere      # the scenes and the copy floor of section 20's table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--scenes", default="sphere512,calgary")
    ap.add_argument("--limit", type=int, default=4, help="max_passes of the limited run on the sphere")
    a = ap.parse_args()
    ctx = hip.Context(0)
    for name in a.scenes.split(","):
        if name == "calgary":
            data, gmin, vox = calgary()
            cases = [(hip.SET_EMPTY, hip.SKEL_TOPOLOGY, None)]
        else:
            data, gmin, vox = sphere(int(name[6:]))
            cases = [(hip.SET_SOLID, hip.SKEL_TOPOLOGY, None), (hip.SET_SOLID, hip.SKEL_CURVE, None), (hip.SET_SOLID, hip.SKEL_TOPOLOGY, a.limit)]
        dims = data.shape[::-1]
        vg = rto.VoxelGrid.from_array(data, gmin, vox)
        floor = copy_ms(data.size, a.rounds)
        ctx.build_octree(data, gmin, vox)
        base = {"scene": name, "dims": list(dims), "copy_ms": round(floor, 4)}
        label_ms = {}
        for set, mode, limit in cases:
            lim = hip.SKEL_NO_LIMIT if limit is None else limit
            t0 = time.perf_counter()
            rc, want, want_summary = vg.skeletonField(set, hip.CONN_FULL, mode, (), lim)
            cpu = (time.perf_counter() - t0) * 1e3
            assert rc == 0
            got, gs = ctx.skeleton_field(set, hip.CONN_FULL, mode, (), limit)    # the warm-up call, and the comparison
            if not np.array_equal(got, want) or gs.tobytes() != want_summary.tobytes():
                raise SystemExit(f"{name} set {set} mode {mode} max_passes {limit}: the field differs from the CPU answer")
            del got, want
            ms, counts = [], []
            for k in range(a.rounds):
                ctx._check(ctx._L.rto_skeleton_field(ctx._h, set, hip.CONN_FULL, mode, None, 0, lim, gs.ctypes.data))
                ms.append(ctx.last_skeleton_ms())
                counts.append(ctx.skeleton_passes())
            m = np.median(np.asarray(ms, np.float64), axis=0)
            c = np.median(np.asarray(counts, np.float64), axis=0)
            if set not in label_ms:
                ts = []
                for k in range(a.rounds + 1):
                    ctx.label_components(set, hip.CONN_FULL)
                    ts.append(sum(ctx.last_components_ms()))
                label_ms[set] = float(np.median(ts[1:]))
            print(json.dumps(dict(base, case="field", set="solid" if set == hip.SET_SOLID else "empty", connectivity=hip.CONN_FULL,
                                  mode="curve" if mode == hip.SKEL_CURVE else "topology", max_passes=limit, passes=int(gs["passes"]),
                                  launches=int(c[0]), tiles_run=int(c[1]), init_ms=round(float(m[0]), 4), thin_ms=round(float(m[1]), 4),
                                  summary_ms=round(float(m[2]), 4), cpu_ms=round(cpu, 1), label_ms=round(label_ms[set], 4),
                                  kept=int(gs["kept"]), removed=int(gs["removed"]))), flush=True)


if __name__ == "__main__":
    main()
