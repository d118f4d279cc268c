#!/usr/bin/env python3
"""Ray-query throughput on one GPU (rto_query_*_device): prints one JSON line.

Workloads, each in every mode (FIRST, CLOSEST, ANY) and on both kernels (the descriptor walk, k_query_desc, and the node-by-node
walk, k_query_nodes, forced by RTO_KERNEL_GENERIC), alternated on the same rays within one process:
  pixels      BASELINE config 2: every pixel of the 1920x1080 frame of the 256^3 test sphere, Camera(0.5, 0.7, 1.8), fov 45;
              the render kernels' frame times on the same frame for context (rto_render_device, rto_render_closest_device)
  incoherent  2^22 seeded rays, origins on a sphere around the scene, aimed at random points of the root box
  shadow      2^22 occlusion rays from config 2's hit points towards the light, t_min = voxel / 100
  hemisphere  2^22 rays from the same hit points into the hemisphere of the hit face, t_max = 4 voxels
Times are device events around `reps` back-to-back launches on one stream (median of `rounds`); Mrays/s = rays / time.
Kernel times for the profile: rocprofv3 --kernel-trace --stats -- python3 tools/query_bench.py --rounds 3"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import ray_tracing_octrees_amd as rto
from ray_tracing_octrees_amd import hip

MODES = {"first": hip.QUERY_FIRST, "closest": hip.QUERY_CLOSEST, "any": hip.QUERY_ANY}
KERNELS = {"desc": rto.KERNEL_AUTO, "nodes": rto.KERNEL_GENERIC}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    ctx = rto.Context(0)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    g = rto.VoxelGrid.test_sphere(256)
    ctx.build_octree(g.data, g.min, g.voxelSize)
    info = ctx.info()
    W, H = 1920, 1080
    cam = rto.Camera(0.5, 0.7, 1.8)
    f = rto.make_frame(cam.getView(), cam.getPos(), W / H, 45.0, W, H)
    y, x = np.mgrid[0:H, 0:W]
    xy = torch.from_numpy(np.stack([x.ravel(), y.ravel()], 1).astype(np.int32)).cuda()
    npix = W * H
    hits = torch.zeros(max(npix, a.rays) * 32, dtype=torch.uint8, device="cuda")
    res = {"scene": "config 2: 256^3 sphere", "nodes": int(info.num_nodes), "depth": int(info.depth), "rays": a.rays}

    # ---- pixel queries + the renders for context
    frame = torch.zeros(npix * 4, dtype=torch.float32, device="cuda")
    res["render_device_ms"] = timed_ms(lambda: ctx.render_device(f, frame.data_ptr(), None, sp), a.reps, a.rounds, stream)
    res["render_closest_device_ms"] = timed_ms(lambda: ctx.render_closest_device(f, frame.data_ptr(), None, sp), a.reps, a.rounds, stream)
    pix = {}
    for r in range(a.rounds):                                          # kernels alternate within each round
        for kn, kv in KERNELS.items():
            ctx.set_kernel(kv)
            for mn, mv in MODES.items():
                ms = timed_ms(lambda: ctx.query_pixels_device(mv, f, xy.data_ptr(), npix, hits.data_ptr(), sp), a.reps, 1, stream)
                pix.setdefault(f"{kn}_{mn}", []).append(ms)
    res["pixels"] = {k: {"ms": float(np.median(v)), "mrays_s": npix / float(np.median(v)) / 1e3} for k, v in pix.items()}

    # ---- closest hits of the frame: the origins of the secondary rays
    ctx.set_kernel(rto.KERNEL_AUTO)
    ctx.query_pixels_device(hip.QUERY_CLOSEST, f, xy.data_ptr(), npix, hits.data_ptr(), sp)
    stream.synchronize()
    rec = hits[: npix * 32].cpu().numpy().view(hip.HIT_DTYPE)
    rng = np.random.default_rng(1)
    # the hit points: on the entry face of the hit leaf (its centre, pushed out along the face's axis)
    hit = np.nonzero(rec["node"] >= 0)[0]
    vs = np.float32(g.voxelSize)
    gmin = np.asarray(g.min, np.float32)
    centre = gmin + (np.stack([rec["x"], rec["y"], rec["z"]], 1)[hit] + 0.5 * rec["size"][hit, None]).astype(np.float32) * vs
    face = rec["face"][hit]
    nrm = np.zeros((len(hit), 3), np.float32)
    ok = face >= 0
    nrm[np.nonzero(ok)[0], face[ok] // 2] = np.where(face[ok] % 2 == 1, 1.0, -1.0)   # entry face: the ray ran against this normal
    p = centre + nrm * (0.5 * rec["size"][hit, None] * vs)
    pick = rng.integers(0, len(hit), a.rays)
    light = np.full(3, 1.0 / np.sqrt(3.0), np.float32)

    def run_set(name, o, d, tmin, tmax):
        rays = hip.make_rays(o, d, tmin, tmax)
        dr = torch.from_numpy(rays.view(np.uint8)).cuda()
        n = len(rays)
        out = {}
        for r in range(a.rounds):
            for kn, kv in KERNELS.items():
                ctx.set_kernel(kv)
                for mn, mv in MODES.items():
                    ms = timed_ms(lambda: ctx.query_rays_device(mv, dr.data_ptr(), n, hits.data_ptr(), sp), max(1, a.reps // 2), 1, stream)
                    out.setdefault(f"{kn}_{mn}", []).append(ms)
        res[name] = {k: {"ms": float(np.median(v)), "mrays_s": n / float(np.median(v)) / 1e3} for k, v in out.items()}
        ctx.set_kernel(rto.KERNEL_AUTO)
        ctx.query_rays_device(hip.QUERY_ANY, dr.data_ptr(), n, hits.data_ptr(), sp)
        stream.synchronize()
        res[name]["hit_fraction"] = float((hits[: n * 32].cpu().numpy().view(hip.HIT_DTYPE)["node"] >= 0).mean())

    # incoherent: origins on a sphere around the root box, aimed into it
    ext = float(info.root_size) * float(vs)
    c0 = gmin + np.float32(0.5 * ext)
    u = rng.normal(size=(a.rays, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = (c0 + u * 1.5 * ext).astype(np.float32)
    tgt = (gmin + rng.random((a.rays, 3)) * ext).astype(np.float32)
    run_set("incoherent", o, tgt - o, 0.0, 1e30)
    # shadow rays from the hit points towards the light
    run_set("shadow", p[pick], np.broadcast_to(light, (a.rays, 3)), float(vs) / 100, 1e30)
    # hemisphere around the hit face's normal, short reach
    h = rng.normal(size=(a.rays, 3)).astype(np.float32)
    nn = nrm[pick].copy()                                             # outward
    nn[~ok[pick]] = light
    h = np.where(((h * nn).sum(1) < 0)[:, None], -h, h)
    run_set("hemisphere", p[pick], h, float(vs) / 100, 4 * float(vs))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
