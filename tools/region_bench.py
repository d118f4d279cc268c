#!/usr/bin/env python3
"""Region-query throughput on one GPU (rto_query_regions_device, rto_query_points_device, rto_query_nearest_device): prints one
JSON line.

Scenes: config 5's 512^3 test sphere and config 4's Calgary grid (425 x 243 x 29), each built on the GPU.  Workloads:
  census     seeded spheres and boxes of three sizes: small (extent 2 voxels), medium (16), root (half the root's edge, centred
             in the grid: the whole tree is walked and the sphere is counted row by row where it cuts the grid's faces)
  locate     2^20 seeded points in the root cube
  nearest    the same points without a limit, and with max_dist = 8 voxels
Each GPU time is the median over `rounds` of device events around `reps` back-to-back launches on one stream.  Beside it, the CPU
statement on one core (tests/region_ref.py, on the first few records) and the dense numpy count over the grid (tests/edit_ref.py's
cover); for the census also the only route a caller had before: applying the brush with rto_edit_voxels (rto_last_edit_ms: brush
kernel + octree rebuild), the grid rebuilt afterwards outside the timing.  Before anything is timed the GPU records are compared
with both CPU answers on those records; exit status 1 on any difference."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import ray_tracing_octrees_amd as rto
from ray_tracing_octrees_amd import hip
import region_ref as rr


def timed_ms(fn, reps, rounds, stream):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(reps):
            fn()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return float(np.median(out))


def calgary():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_scene_cache.npz"))
    dims = tuple(int(x) for x in z["dims"])
    data = np.unpackbits(z["packed"])[: dims[0] * dims[1] * dims[2]].reshape(dims[2], dims[1], dims[0])
    return np.ascontiguousarray(data, np.uint8), z["min"].astype(np.float32), np.float32(z["voxel"])


def to_device(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cpu-records", type=int, default=8, help="records of each workload the CPU statement answers")
    ap.add_argument("--scenes", default="config5,config4")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    ctx = rto.Context(0)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    res, mismatches = {"points": a.points}, 0
    for name in a.scenes.split(","):
        if name == "config5":
            g = rto.VoxelGrid.test_sphere(512)
            data, gmin, vs = g.data, np.asarray(g.min, np.float32), np.float32(g.voxelSize)
        else:
            data, gmin, vs = calgary()
        ctx.build_octree(data, gmin, vs)
        info = ctx.info()
        dims = np.array([data.shape[2], data.shape[1], data.shape[0]], np.float64)
        root = float(info.root_size)
        r = {"nodes": int(info.num_nodes), "depth": int(info.depth), "dims": [int(x) for x in dims]}
        t0 = time.perf_counter()
        T = rr.Tree(ctx.download_nodes(), gmin, vs, dims.astype(np.int64))
        r["cpu_tree_setup_s"] = time.perf_counter() - t0
        rng = np.random.default_rng(1)
        world = lambda v: (gmin.astype(np.float64) + np.asarray(v, np.float64) * float(vs)).astype(np.float32)

        # ---- census
        for size, ext, n in (("small", 2.0, 1 << 16), ("medium", 16.0, 1 << 12), ("root", root / 2, 64)):
            for shape, sname in ((hip.BRUSH_SPHERE, "sphere"), (hip.BRUSH_BOX, "box")):
                cen = world(dims / 2 + rng.uniform(-0.5, 0.5, (n, 3))) if size == "root" else world(rng.uniform(0, dims, (n, 3)))
                b = hip.make_brushes(cen, np.float32(ext * float(vs)), shape)
                d_b, d_out = to_device(b), torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
                ctx.query_regions_device(d_b.data_ptr(), n, d_out.data_ptr(), sp)
                stream.synchronize()
                got = d_out.cpu().numpy().view(hip.REGION_DTYPE)
                k = a.cpu_records if size != "root" else 1
                e = {"regions": n, "mean_filled": float(got["filled"].mean()), "mean_leaves": float(got["solid_leaves"].mean())}
                t0 = time.perf_counter()
                dense = [rr.dense_census(data, b[i], gmin, vs) for i in range(k)]
                e["cpu_dense_ms_per_region"] = (time.perf_counter() - t0) / k * 1e3
                bad = sum((int(got[i]["filled"]), int(got[i]["covered"])) != dense[i] for i in range(k))
                if size != "root":                                   # the statement's Python loop over a root-sized region's leaves takes minutes
                    t0 = time.perf_counter()
                    want = rr.census(T, b[:k])
                    e["cpu_statement_ms_per_region"] = (time.perf_counter() - t0) / k * 1e3
                    bad += int((want.tobytes() != got[:k].tobytes()))
                mismatches += bad
                ms = timed_ms(lambda: ctx.query_regions_device(d_b.data_ptr(), n, d_out.data_ptr(), sp), a.reps, a.rounds, stream)
                e.update(gpu_ms=ms, regions_per_s=n / ms * 1e3, mismatches=bad)
                # the route without a census: carve with the brush, read the changed count, then put the grid back
                i = int(np.argmax(got["filled"][:64]))
                changed = ctx.edit_voxels(b[i:i + 1])
                e["edit_route_ms"] = float(sum(x for x in ctx.last_edit_ms()[:2] if x > 0))
                mismatches += int(changed != got[i]["filled"])
                if changed:
                    ctx.build_octree(data, gmin, vs)
                r[f"census_{size}_{sname}"] = e

        # ---- points
        n = a.points
        pts = world(rng.uniform(0, root, (n, 3)))
        d_p, d_hits = to_device(pts), torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        ctx.query_points_device(d_p.data_ptr(), n, d_hits.data_ptr(), sp)
        stream.synchronize()
        hits = d_hits.cpu().numpy().view(hip.POINT_HIT_DTYPE)
        k = a.cpu_records * 8
        t0 = time.perf_counter()
        want = rr.locate(T, pts[:k])
        cpu = (time.perf_counter() - t0) / k * 1e3
        bad = int(want.tobytes() != hits[:k].tobytes())
        ms = timed_ms(lambda: ctx.query_points_device(d_p.data_ptr(), n, d_hits.data_ptr(), sp), a.reps, a.rounds, stream)
        r["locate"] = {"gpu_ms": ms, "points_per_s": n / ms * 1e3, "cpu_statement_ms_per_point": cpu, "mismatches": bad,
                       "solid_fraction": float((hits["solid"] == 1).mean())}
        mismatches += bad
        for label, lim in (("nearest_unlimited", np.inf), ("nearest_8_voxels", 8.0 * float(vs))):
            nm = n if np.isfinite(lim) else min(n, 1 << 16)          # without a limit a point far from solid walks much of the tree
            d_n, d_near = to_device(hip.make_near_points(pts[:nm], lim)), torch.zeros(nm * 32, dtype=torch.uint8, device="cuda")
            ctx.query_nearest_device(d_n.data_ptr(), nm, d_near.data_ptr(), sp)
            stream.synchronize()
            near = d_near.cpu().numpy().view(hip.NEAREST_DTYPE)
            t0 = time.perf_counter()
            want = rr.nearest(T, pts[:k], lim)
            cpu = (time.perf_counter() - t0) / k * 1e3
            bad = int(want.tobytes() != near[:k].tobytes())
            ms = timed_ms(lambda: ctx.query_nearest_device(d_n.data_ptr(), nm, d_near.data_ptr(), sp), max(1, a.reps // 2), a.rounds, stream)
            r[label] = {"points": nm, "gpu_ms": ms, "points_per_s": nm / ms * 1e3, "cpu_statement_ms_per_point": cpu, "mismatches": bad,
                        "found_fraction": float((near["dist2"] >= 0).mean())}
            mismatches += bad
        res[name] = r
    res["mismatches"] = mismatches
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")
    ctx.close()
    sys.exit(1 if mismatches else 0)


if __name__ == "__main__":
    main()
