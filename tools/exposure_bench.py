#!/usr/bin/env python3
"""Exposure fields on one GPU (rto_exposure_field): one JSON line per scene and case.

Scenes: config 5's 512^3 test sphere (SKIN) and Calgary (tests/golden/ref_scene_cache.npz; SKIN and ALL), each with 64 quantized
directions of the upper hemisphere weighted by their cosine, with no reach and with reach 16.  Every field and summary is compared
with the CPU answer (the host layer's exposureFieldCPU) before anything is timed.  Per case, medians over --rounds calls in one
process after one warm-up call: device ms of prepare (bit rows, selection, templates), march and summary (rto_last_exposure_ms);
`steps`, the template entries tested, counted by the CPU form (the timed kernel counts nothing), and `ns_per_step` = march / steps.
Comparators in the same run: `cpu_ms`, host/Exposure.cpp on one core, once; `copy_ms`, a device-to-device copy of an int32 volume
of the grid's size.  --cpu-only: the CPU form alone (steps and cpu_ms), on a machine without a GPU."""
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
from exposure_ref import hemisphere


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--scenes", default="sphere512,calgary")
    ap.add_argument("--dirs", type=int, default=64)
    ap.add_argument("--reach", type=int, default=16, help="the reach of the limited runs")
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--no-cpu", action="store_true", help="skip the comparison with, and the timing of, the CPU form (no steps, no ns_per_step)")
    a = ap.parse_args()
    from geodesic_bench import calgary, copy_ms, sphere      # the scenes and the copy floor of section 20's table
    dirs = hip.quantize_directions(hemisphere(a.dirs))
    weights = np.maximum(1, np.rint(100 * hemisphere(a.dirs)[:, 2])).astype(np.int32)
    ctx = None if a.cpu_only else hip.Context(0)
    for name in a.scenes.split(","):
        if name == "calgary":
            data, gmin, vox = calgary()
            modes = (hip.EXPO_SKIN, hip.EXPO_ALL)
        else:
            data, gmin, vox = sphere(int(name[6:]))
            modes = (hip.EXPO_SKIN,)
        dims = data.shape[::-1]
        vg = rto.VoxelGrid.from_array(data, gmin, vox)
        base = {"scene": name, "dims": list(dims), "dirs": a.dirs}
        if ctx:
            base["copy_ms"] = round(copy_ms(data.size, a.rounds), 4)
            ctx.build_octree(data, gmin, vox)
        for mode in modes:
            for reach in (None, a.reach):
                r = hip.EXPO_NO_LIMIT if reach is None else reach
                line = dict(base, mode="skin" if mode == hip.EXPO_SKIN else "all", reach=reach)
                want, steps = None, 0
                if not a.no_cpu:
                    t0 = time.perf_counter()
                    rc, want, ws, steps = vg.exposureField(dirs, weights, mode, r, withSteps=True)
                    cpu = (time.perf_counter() - t0) * 1e3
                    assert rc == 0
                    line.update(evaluated=int(ws["evaluated"]), steps=int(steps), dark=int(ws["dark"]), open=int(ws["open"]), cpu_ms=round(cpu, 1))
                if ctx:
                    got, gs = ctx.exposure_field(dirs, weights, mode, reach)          # the warm-up call, and the comparison
                    if want is not None and (not np.array_equal(got, want) or gs.tobytes() != ws.tobytes()):
                        raise SystemExit(f"{name} mode {mode} reach {reach}: the field differs from the CPU answer")
                    if want is None:
                        line.update(evaluated=int(gs["evaluated"]), dark=int(gs["dark"]), open=int(gs["open"]))
                    del got
                    ms = []
                    for k in range(a.rounds):
                        ctx._check(ctx._L.rto_exposure_field(ctx._h, dirs.ctypes.data, weights.ctypes.data, len(dirs), mode, r, gs.ctypes.data))
                        ms.append(ctx.last_exposure_ms())
                    m = np.median(np.asarray(ms, np.float64), axis=0)
                    line.update(prepare_ms=round(float(m[0]), 4), march_ms=round(float(m[1]), 4), summary_ms=round(float(m[2]), 4))
                    if steps:
                        line.update(ns_per_step=round(float(m[1]) * 1e6 / int(steps), 5))
                del want
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
