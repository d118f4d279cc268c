#!/usr/bin/env python3
"""Triangle-query throughput on one GPU (rto_query_triangle*_device): prints one JSON line.

Config 5's scene (the 512^3 test sphere with its leaf triangles, rto_build_octree + rto_build_leaf_triangles), both kernels (the
descriptor walk, k_triq_desc, and the node-by-node walk, k_triq_nodes, forced by RTO_KERNEL_GENERIC) alternated on the same rays
within one process:
  pixels     FIRST on every pixel of the 3840x2160 frame, Camera(0.5, 0.7, 1.8), fov 45; the triangle render's frame time on the
             same frame, shadows off, for context (rto_render_triangles_device)
  shadow     ANY on 2^22 shadow rays built from those hits as the render builds them (tests/tri_query_ref.py shadow_rays), with
             t_max = 1e30 (the directional light) and with t_max = the distance to a point light
  incoherent CLOSEST on 2^22 seeded rays from a sphere around the scene aimed at random points of the root box
Times are device events around `reps` back-to-back launches on one stream (median of `rounds`); Mrays/s = rays / time.
Kernel times for the profile: rocprofv3 --kernel-trace --stats -- python3 tools/tri_query_bench.py --rounds 3"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import ray_tracing_octrees_amd as rto
import tri_query_ref as tq
from ray_tracing_octrees_amd import hip

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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    ctx = rto.Context(0)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    g = rto.VoxelGrid.test_sphere(512)
    ctx.build_octree(g.data, g.min, g.voxelSize)
    ctx.build_leaf_triangles()
    info = ctx.info()
    tris, _ = ctx.download_leaf_triangles()
    W, H = 3840, 2160
    cam = rto.Camera(0.5, 0.7, 1.8)
    pos = np.asarray(cam.getPos(), np.float32)
    f = rto.make_frame(cam.getView(), cam.getPos(), W / H, 45.0, W, H)
    y, x = np.mgrid[0:H, 0:W]
    xy = torch.from_numpy(np.stack([x.ravel(), y.ravel()], 1).astype(np.int32)).cuda()
    npix = W * H
    hits = torch.zeros(max(npix, a.rays) * 32, dtype=torch.uint8, device="cuda")
    res = {"scene": "config 5: 512^3 sphere, leaf triangles", "nodes": int(info.num_nodes), "depth": int(info.depth),
           "triangles": int(len(tris)), "rays": a.rays}

    # ---- FIRST on every pixel, and the render for context
    frame = torch.zeros(npix * 4, dtype=torch.float32, device="cuda")
    res["render_triangles_device_ms"] = timed_ms(lambda: ctx.render_triangles_device(f, frame.data_ptr(), False, None, sp),
                                                 a.reps, a.rounds, stream)
    pix = {}
    for _ in range(a.rounds):                                          # kernels alternate within each round
        for kn, kv in KERNELS.items():
            ctx.set_kernel(kv)
            ms = timed_ms(lambda: ctx.query_triangle_pixels_device(hip.QUERY_FIRST, f, xy.data_ptr(), npix, hits.data_ptr(), sp),
                          a.reps, 1, stream)
            pix.setdefault(kn, []).append(ms)
    res["pixels_first"] = {k: {"ms": float(np.median(v)), "mrays_s": npix / float(np.median(v)) / 1e3} for k, v in pix.items()}

    ctx.set_kernel(rto.KERNEL_AUTO)
    ctx.query_triangle_pixels_device(hip.QUERY_FIRST, f, xy.data_ptr(), npix, hits.data_ptr(), sp)
    stream.synchronize()
    rec = hits[: npix * 32].cpu().numpy().view(hip.TRI_HIT_DTYPE).copy()
    hit = np.nonzero(rec["tri"] >= 0)[0]
    res["pixels_hit_fraction"] = float(len(hit) / npix)
    rng = np.random.default_rng(1)
    pick = hit[rng.integers(0, len(hit), a.rays)]
    # the pixel rays of the picked hits: the render's own directions (the oracle's generateRay, bit-equal to the kernels')
    from oracle import orc
    dirs = orc.generate_rays(cam.getView(), cam.getPos(), W / H, 45.0, W, H).reshape(-1, 3)[pick]
    so, sd = tq.shadow_rays(pos, dirs, rec[pick], tris, float(g.voxelSize))

    def run_set(name, mode, o, d, tmin, tmax):
        rays = hip.make_rays(o, d, tmin, tmax)
        dr = torch.from_numpy(rays.view(np.uint8)).cuda()
        n = len(rays)
        out = {}
        for _ in range(a.rounds):
            for kn, kv in KERNELS.items():
                ctx.set_kernel(kv)
                ms = timed_ms(lambda: ctx.query_triangles_device(mode, dr.data_ptr(), n, hits.data_ptr(), sp), a.reps, 1, stream)
                out.setdefault(kn, []).append(ms)
        res[name] = {k: {"ms": float(np.median(v)), "mrays_s": n / float(np.median(v)) / 1e3} for k, v in out.items()}
        ctx.set_kernel(rto.KERNEL_AUTO)
        ctx.query_triangles_device(mode, dr.data_ptr(), n, hits.data_ptr(), sp)
        stream.synchronize()
        res[name]["hit_fraction"] = float((hits[: n * 32].cpu().numpy().view(hip.TRI_HIT_DTYPE)["tri"] >= 0).mean())

    run_set("shadow_any", hip.QUERY_ANY, so, sd, 0.0, 1e30)
    # a point light outside the sphere, 0.75 root-box edges from the centre towards the light: t_max = its distance (|d| = 1)
    ext = float(info.root_size) * float(g.voxelSize)
    gmin = np.asarray(g.min, np.float32)
    lp = (gmin + np.float32(0.5 * ext) + tq.LIGHT * np.float32(0.75 * ext)).astype(np.float32)
    to = lp - so
    dist = np.linalg.norm(to.astype(np.float64), axis=1)
    run_set("point_light_any", hip.QUERY_ANY, so, (to / dist[:, None]).astype(np.float32), 0.0, dist.astype(np.float32))
    c0 = gmin + np.float32(0.5 * ext)
    u = rng.normal(size=(a.rays, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = (c0 + u * 1.5 * ext).astype(np.float32)
    tgt = (gmin + rng.random((a.rays, 3)) * ext).astype(np.float32)
    run_set("incoherent_closest", hip.QUERY_CLOSEST, o, tgt - o, 0.0, 1e30)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
