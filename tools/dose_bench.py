#!/usr/bin/env python3
"""Dose fields on one GPU (rto_dose_field): one JSON line per scene and case, appended to profiles/dose_bench.jsonl (--out).

Scenes: Calgary (tests/golden/ref_scene_cache.npz; ALL and SKIN) and config 5's 512^3 test sphere (SKIN), each with 1, 8 and 64
sources in seeded EMPTY voxels, with reach 64 and with none, under plain line of sight and under a 4-entry table, inverse-square
falloff.  Every field, coverage table and summary is compared with the CPU answer (the host layer's doseFieldCPU) before anything is
timed; the CPU form runs first, the sources dealt to --procs worker processes (a field is the sum of its sources' fields), and
`cpu_ms` is the sum of the workers' times: one core.  Per case, medians over --rounds calls in one process after one warm-up call:
device ms of prepare (bit rows, selection, uploads), march and summary (rto_last_dose_ms); `steps`, the crossed voxels tested,
counted by the CPU form (the timed kernel counts nothing), and `ns_per_step` = march / steps.  Comparators in the same run:
`copy_ms`, a device-to-device copy of an int32 volume of the grid's size, and per scene and mode one "yardstick" line: k_expo_march's
ns per step with 64 hemisphere directions and no reach, its steps counted by exposureFieldCPU."""
import argparse
import json
import multiprocessing as mp
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

TABLE4 = [65536, 32768, 8192, 1024]
_SCENE = {}


def scene(name):
    """(data, gmin, vox) of a scene by name, loaded once per process."""
    if name not in _SCENE:
        from geodesic_bench import calgary, sphere
        _SCENE[name] = calgary() if name == "calgary" else sphere(int(name[6:]))
    return _SCENE[name]


def sources_of(data, n):
    """n sources in seeded EMPTY voxels, the first n of one list of 64, weight 1,000,000 each."""
    empty = np.flatnonzero(data.reshape(-1) == 0)
    v = np.sort(np.random.default_rng(31).choice(empty, 64, replace=False))[np.random.default_rng(32).permutation(64)][:n]
    dz, dy, dx = data.shape
    return np.stack([v % dx, v // dx % dy, v // dx // dy, np.full(n, 1000000)], axis=1).astype(np.int32)


def cpu_part(job):
    """One worker's share: the CPU form for some of a case's sources."""
    name, src, table, mode, reach = job
    import ray_tracing_octrees_amd as rto
    data, gmin, vox = scene(name)
    vg = rto.VoxelGrid.from_array(data, gmin, vox)
    t0 = time.perf_counter()
    rc, e, cov, s, steps = vg.doseField(src, table, 1, mode, reach, withSteps=True)
    assert rc == 0
    at = np.flatnonzero(e.reshape(-1) >= 0)                            # the evaluated voxels alone travel back
    return at, e.reshape(-1)[at], cov, int(steps), (time.perf_counter() - t0) * 1e3


def cpu_case(pool, procs, name, src, table, mode, reach):
    parts = [src[i::procs] for i in range(min(procs, len(src)))]
    out = pool.map(cpu_part, [(name, p, table, mode, reach) for p in parts])
    e = (out[0][0], sum(o[1].astype(np.int64) for o in out).astype(np.int32))       # (the evaluated voxels, their values)
    cov = np.zeros(len(src), np.int64)
    for i, o in enumerate(out):
        cov[i::procs] = o[2]
    return e, cov, sum(o[3] for o in out), sum(o[4] for o in out), len(out[0][0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--scenes", default="calgary,sphere512")
    ap.add_argument("--sources", default="1,8,64")
    ap.add_argument("--reach", type=int, default=64, help="the reach of the limited runs")
    ap.add_argument("--procs", type=int, default=16, help="worker processes of the CPU form")
    ap.add_argument("--no-coverage", action="store_true", help="the library is an A/B build without the coverage atomics (tools/build_variants.sh "
                    "with -DRTO_DOSE_AB_NO_COVERAGE_ATOMIC, selected by RTO_HIP_LIB): the coverage table is not compared")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dose_bench.jsonl"), help="the file the lines are appended to")
    a = ap.parse_args()
    from exposure_ref import hemisphere
    pool = mp.get_context("spawn").Pool(a.procs)                        # before this process opens the GPU; the workers never do
    cases, yard = [], {}
    try:
        for name in a.scenes.split(","):
            data, gmin, vox = scene(name)
            for mode in ((0, 1) if name == "calgary" else (1,)):
                for n in (int(x) for x in a.sources.split(",")):
                    src = sources_of(data, n)
                    for reach in (a.reach, None):
                        for table in (None, TABLE4):
                            r = 0x7fffffff if reach is None else reach
                            want = cpu_case(pool, a.procs, name, src, table, mode, r)
                            cases.append((name, mode, n, reach, table, src, want))
                            print(f"# cpu {name} mode {mode} n {n} reach {reach} table {table is not None}: {want[3]:.0f} ms, {want[2]} steps", flush=True)
    finally:
        pool.close()
        pool.join()
    import ray_tracing_octrees_amd as rto
    from ray_tracing_octrees_amd import hip
    from geodesic_bench import copy_ms
    ctx = hip.Context(0)
    lines, built = [], None
    dirs = hip.quantize_directions(hemisphere(64))
    for name, mode, n, reach, table, src, (want, wcov, steps, cpu, evaluated) in cases:
        data, gmin, vox = scene(name)
        if built != name:
            ctx.build_octree(data, gmin, vox)
            built = name
            copy = round(copy_ms(data.size, a.rounds), 4)
        if (name, mode) not in yard:                                    # the yardstick: k_expo_march on the same scene and mode
            rc, ee, es, esteps = rto.VoxelGrid.from_array(data, gmin, vox).exposureField(dirs, None, mode, hip.EXPO_NO_LIMIT, withSteps=True)
            got, gs = ctx.exposure_field(dirs, None, mode, None)
            if rc != 0 or not np.array_equal(got, ee):
                raise SystemExit(f"{name} mode {mode}: the exposure field differs from the CPU answer")
            ms = []
            for k in range(a.rounds):
                ctx.exposure_field(dirs, None, mode, None)
                ms.append(ctx.last_exposure_ms()[1])
            yard[(name, mode)] = float(np.median(ms)) * 1e6 / int(esteps)
            lines.append({"scene": name, "mode": "skin" if mode else "all", "yardstick": "k_expo_march", "dirs": 64, "steps": int(esteps),
                          "march_ms": round(float(np.median(ms)), 4), "ns_per_step": round(yard[(name, mode)], 5)})
            print(json.dumps(lines[-1]), flush=True)
            del got, ee
        got, gs = ctx.dose_field(src, table, 1, mode, reach)            # the warm-up call, and the comparison
        flat = got.reshape(-1)
        if (not np.array_equal(flat[want[0]], want[1]) or int((flat >= 0).sum()) != evaluated or not (a.no_coverage or np.array_equal(ctx.dose_coverage(), wcov))
                or int(gs["evaluated"]) != evaluated or int(gs["total"]) != int(want[1].astype(np.int64).sum())):
            raise SystemExit(f"{name} mode {mode} n {n} reach {reach}: the field or the coverage differs from the CPU answer")
        del got, flat
        t = None if table is None else np.asarray(table, np.uint32)
        ms = []
        for k in range(a.rounds):
            ctx._check(ctx._L.rto_dose_field(ctx._h, src.ctypes.data, n, None if t is None else t.ctypes.data, 0 if t is None else t.size, 1, mode,
                                             hip.DOSE_NO_LIMIT if reach is None else reach, gs.ctypes.data))
            ms.append(ctx.last_dose_ms())
        m = np.median(np.asarray(ms, np.float64), axis=0)
        line = {"scene": name, "dims": list(data.shape[::-1]), "mode": "skin" if mode else "all", "sources": n, "reach": reach,
                "table": "sight" if table is None else "4-entry", "evaluated": evaluated, "seen": int(gs["seen"]), "steps": steps,
                "cpu_ms": round(cpu, 1), "copy_ms": copy, "prepare_ms": round(float(m[0]), 4), "march_ms": round(float(m[1]), 4),
                "summary_ms": round(float(m[2]), 4)}
        if a.no_coverage:
            line["coverage_atomics"] = False
        if steps:
            line["ns_per_step"] = round(float(m[1]) * 1e6 / steps, 5)
            line["vs_expo_march"] = round(line["ns_per_step"] / yard[(name, mode)], 2)
        lines.append(line)
        print(json.dumps(line), flush=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
