#!/usr/bin/env python3
"""Part segmentation on one GPU (rto_segment_parts): one JSON line per scene, set and connectivity.

Scenes: config 5's 512^3 test sphere (one part is expected: the pure cost of the per-voxel passes) and Calgary
(tests/golden/ref_scene_cache.npz), both sets, at --ratio (800).  Unless --no-cpu is given, labels, both tables and the summary are
compared with the CPU answer (the host layer's segmentPartsCPU, timed once on one core) before anything is timed.  Per case,
medians over --rounds calls in one process after one warm-up call of the five phases of rto_last_parts_ms (transform, ascent +
flatten, ranking + basin table, edges: device ms; host merge + relabel: the host's clock), with the basins, the basin edges and
bytes that came down, the flatten rounds, the edge table's slots and the host merge's share of the whole.  Comparator in the same
run: `copy_ms`, a device-to-device copy of an int32 volume of the grid's size; three of them are the floor of the per-voxel passes."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

import ray_tracing_octrees_amd as rto
from ray_tracing_octrees_amd import hip
from thickness_bench import calgary, copy_ms, sphere


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--scenes", default="sphere512,calgary")
    ap.add_argument("--ratio", type=int, default=800)
    ap.add_argument("--conns", default="6", help="comma-separated: 6, 26")
    ap.add_argument("--no-cpu", action="store_true", help="skip the comparison with, and the timing of, the CPU form")
    a = ap.parse_args()
    ctx = hip.Context(0)
    for name in a.scenes.split(","):
        data, gmin, vox = calgary() if name == "calgary" else sphere(int(name[6:]))
        dims = data.shape[::-1]
        vg = None if a.no_cpu else rto.VoxelGrid.from_array(data, gmin, vox)
        floor = copy_ms(data.size, a.rounds)
        ctx.build_octree(data, gmin, vox)
        base = {"scene": name, "dims": list(dims), "ratio": a.ratio, "copy_ms": round(floor, 4)}
        for s in (hip.SET_SOLID, hip.SET_EMPTY):
            for conn in (int(c) for c in a.conns.split(",")):
                summary = ctx.segment_parts(s, conn, a.ratio)                # the warm-up call, and the comparison
                cpu = None
                if vg is not None:
                    t0 = time.perf_counter()
                    labels, parts, necks, want = vg.segmentParts(s, conn, a.ratio)
                    cpu = (time.perf_counter() - t0) * 1e3
                    if not (np.array_equal(ctx.part_labels(), labels) and ctx.parts().tobytes() == parts.tobytes()
                            and ctx.necks().tobytes() == necks.tobytes() and summary.tobytes() == want.tobytes()):
                        raise SystemExit(f"{name} set {s} conn {conn}: the segmentation differs from the CPU answer")
                    del labels
                ms = []
                for _ in range(a.rounds):
                    ctx.segment_parts(s, conn, a.ratio)
                    ms.append(ctx.last_parts_ms())
                m = np.median(np.asarray(ms, np.float64), axis=0)
                basins, edges, rounds, cap = ctx.debug_parts()
                total = float(m.sum())
                print(json.dumps(dict(base, set="solid" if s == hip.SET_SOLID else "empty", conn=conn,
                                      transform_ms=round(float(m[0]), 4), ascent_ms=round(float(m[1]), 4), ranking_ms=round(float(m[2]), 4),
                                      edges_ms=round(float(m[3]), 4), merge_ms=round(float(m[4]), 4), total_ms=round(total, 4),
                                      merge_share=round(float(m[4]) / total, 4) if total > 0 else None,
                                      cpu_ms=None if cpu is None else round(cpu, 1), parts=int(summary["parts"]), basins=basins,
                                      necks=int(summary["necks"]), basin_edges=edges, bytes_down=24 * edges + 56 * basins,
                                      flatten_rounds=rounds, table_slots=cap)), flush=True)


if __name__ == "__main__":
    main()
