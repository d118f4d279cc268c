#!/usr/bin/env python3
"""The lit render of the triangle surface (rto_render_lit_triangles_device) against the route integrators compose today; prints
one JSON line.

Frames: BASELINE config 5 (512^3 test sphere, Camera(0.5, 0.7, 1.8), 3840x2160) and the 256^3 sphere at 1920x1080, fov 45, light
(-1, -1, -1), triangles from rto_build_leaf_triangles.  Settings: the shadow ray alone, shadow + K = 8 and shadow + K = 32 AO rays
of 4 voxels.  Per frame and setting, alternated within every round of one process:
  render    rto_render_triangles_device (shadow on), for scale
  lit       rto_render_lit_triangles_device (compacted hits, secondary rays built in registers)
  composed  rto_query_triangle_pixels_device FIRST over every pixel; the hit pixels compacted (torch.nonzero) and their 1 + K rays
            built with torch on the device by the same rule into 32-byte rto_ray records;
            rto_query_triangles_device ANY on them; shading with torch.  Its frame is compared with the lit frame
            (`composed_equal`: share of equal pixels; `frames_equal`: every pixel of every setting, and the exit status is 1 when it is
            false).
Times are device events around `reps` frames on one stream, medians of `rounds` rounds.  Kernel times: rocprofv3 --kernel-trace
--stats -- python3 tools/tri_lit_bench.py --rounds 2"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import ray_tracing_octrees_amd as rto
from ray_tracing_octrees_amd import hip
from oracle import orc
from lit_bench import SETTINGS, timed_ms


class Composed:
    """The integrator's route, on the device with torch (one stream)."""

    def __init__(self, ctx, frame, view, pos, voxel, tris, light, K, radius, seed, stream):
        self.ctx, self.f, self.K, self.stream = ctx, frame, K, stream
        W, H = frame.width, frame.height
        self.npix = W * H
        y, x = np.mgrid[0:H, 0:W]
        dev = "cuda"
        self.xy = torch.from_numpy(np.stack([x.ravel(), y.ravel()], 1).astype(np.int32)).to(dev)
        self.px = torch.from_numpy(x.ravel().astype(np.int64)).to(dev)
        self.py = torch.from_numpy(y.ravel().astype(np.int64)).to(dev)
        self.dirs = torch.from_numpy(orc.generate_rays(view, pos, W / H, 45.0, W, H).reshape(-1, 3).astype(np.float32)).to(dev)
        self.pos = torch.from_numpy(np.asarray(pos, np.float32)).to(dev)
        self.v0 = torch.from_numpy(np.ascontiguousarray(tris[:, 0:3])).to(dev)
        self.vs = torch.tensor(np.float32(voxel), device=dev)
        v = np.asarray(light, np.float32)
        l = v * (np.float32(1) / np.sqrt(np.float32((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])))
        self.lneg = torch.from_numpy((-l).astype(np.float32)).to(dev)
        self.table = torch.from_numpy(hip.ao_directions()).to(dev)
        self.radius, self.seed = np.float32(radius), int(seed)
        self.hits = torch.zeros(self.npix * 8, dtype=torch.int32, device=dev)
        self.rgba = torch.zeros(self.npix, 4, dtype=torch.float32, device=dev)

    def _mix(self, v):
        m = 0xFFFFFFFF
        v = v ^ (v >> 16); v = (v * 0x7FEB352D) & m; v = v ^ (v >> 15); v = (v * 0x846CA68B) & m
        return v ^ (v >> 16)

    def __call__(self):
        sp = self.stream.cuda_stream
        K = self.K
        self.ctx.query_triangle_pixels_device(hip.QUERY_FIRST, self.f, self.xy.data_ptr(), self.npix, self.hits.data_ptr(), sp)
        with torch.cuda.stream(self.stream):
            rec = self.hits.view(self.npix, 8)
            hidx = torch.nonzero(rec[:, 1] >= 0).squeeze(1)
            r = rec[hidx]
            t = r[:, 0].view(torch.float32)
            nrm = r[:, 5:8].view(torch.float32)                    # the stored normal, already turned against the ray
            nx, ny, nz = nrm[:, 0], nrm[:, 1], nrm[:, 2]
            d = self.dirs[hidx]
            p = self.pos + d * t[:, None]
            dot = (nx * self.lneg[0] + ny * self.lneg[1]) + nz * self.lneg[2]
            ndotl = torch.where(dot > 0, dot, torch.zeros_like(dot))          # glm max(0, dot): 0 for a NaN
            q = p - self.v0[r[:, 1].long()]
            hm = p.abs().amax(1)
            h = (self.vs * 1e-3 + hm * 2.0 ** -18) - ((q[:, 0] * nx + q[:, 1] * ny) + q[:, 2] * nz)
            so = p + nrm * h[:, None]
            n = len(hidx)
            rays = torch.zeros(n, 1 + K, 8, dtype=torch.float32, device=p.device)
            rays[:, :, 0:3] = so[:, None, :]
            rays[:, 0, 4:7] = self.lneg
            rays[:, 0, 7] = torch.where(ndotl > 0, torch.tensor(1e30, device=p.device), torch.tensor(-1.0, device=p.device))
            if K:
                hh = self._mix(((self.px[hidx] * 0x8DA6B343) & 0xFFFFFFFF) ^ ((self.py[hidx] * 0xD8163841) & 0xFFFFFFFF)
                               ^ ((self.seed * 0xCB1AB31F) & 0xFFFFFFFF))
                s = torch.arange(K, device=p.device)
                e = (hh[:, None] + (64 * s)[None, :] // K) & 63
                tt = self.table[e]
                x = torch.where(((hh >> 6) & 1).bool()[:, None], -tt[..., 0], tt[..., 0])
                y = torch.where(((hh >> 7) & 1).bool()[:, None], -tt[..., 1], tt[..., 1])
                z = tt[..., 2]
                sg = torch.where(nz < 0, -torch.ones_like(nz), torch.ones_like(nz))
                a = -1.0 / (sg + nz)
                b = (nx * ny) * a
                U = torch.stack([1.0 + ((sg * nx) * nx) * a, sg * b, (-sg) * nx], 1)
                V = torch.stack([b, sg + (ny * ny) * a, -ny], 1)
                rays[:, 1:, 4:7] = (x[..., None] * U[:, None, :] + y[..., None] * V[:, None, :]) + z[..., None] * nrm[:, None, :]
                rays[:, 1:, 7] = float(self.radius)
            bad = ~(torch.isfinite(rays[:, :, 0:3]).all(2) & torch.isfinite(rays[:, :, 4:7]).all(2))
            rays[:, :, 7] = torch.where(bad, torch.tensor(-1.0, device=p.device), rays[:, :, 7])          # t_min > t_max: a miss
            out = torch.empty(n * (1 + K) * 8, dtype=torch.int32, device=p.device)
        self.ctx.query_triangles_device(hip.QUERY_ANY, rays.data_ptr(), n * (1 + K), out.data_ptr(), sp)
        with torch.cuda.stream(self.stream):
            hit = (out.view(n, 1 + K, 8)[:, :, 1] >= 0)
            S = ~hit[:, 0]
            occ = hit[:, 1:].sum(1)
            A = ((K - occ).float() / K) if K else torch.ones(n, device=p.device)
            dd = torch.where(S, ndotl, torch.zeros_like(ndotl))
            amb = 0.1 * A
            self.rgba.zero_()
            self.rgba[:, 3] = 1.0
            self.rgba[hidx] = torch.stack([1.0 * dd + amb, 0.8 * dd + amb, 0.6 * dd + amb, torch.ones_like(dd)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None, help="config5 or sphere256")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    ctx = rto.Context(0)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    res = {"rounds": a.rounds, "reps": a.reps, "configs": {}}
    scenes = {"config5": (512, 3840, 2160), "sphere256": (256, 1920, 1080)}
    for name, (dim, W, H) in scenes.items():
        if a.only and a.only != name:
            continue
        g = rto.VoxelGrid.test_sphere(dim)
        cam = rto.Camera(0.5, 0.7, 1.8)
        ctx.build_octree(g.data, g.min, g.voxelSize)
        ctx.build_leaf_triangles()
        tris, _ = ctx.download_leaf_triangles()
        view, pos = cam.getView(), cam.getPos()
        f = rto.make_frame(view, pos, W / H, 45.0, W, H)
        frame = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
        vis = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        radius = float(np.float32(4 * float(g.voxelSize)))
        runs = {"render": lambda: ctx.render_triangles_device(f, frame.data_ptr(), True, None, sp)}
        comps = {}
        for sname, sh, K in SETTINGS:
            L = hip.make_lighting((-1.0, -1.0, -1.0), bool(sh), K, radius, 1)
            runs[f"lit_{sname}"] = (lambda L=L: ctx.render_lit_triangles_device(f, L, frame.data_ptr(), vis.data_ptr(), sp))
            comps[sname] = Composed(ctx, f, view, pos, g.voxelSize, tris, (-1.0, -1.0, -1.0), K, radius, 1, stream)
            runs[f"composed_{sname}"] = comps[sname]
        for fn in runs.values():                                    # warm-up: tables, work buffers, allocator
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                times[k].append(timed_ms(fn, a.reps, stream))
        out = {"frame": [W, H]}
        out.update({k: float(np.median(v)) for k, v in times.items()})
        for sname, sh, K in SETTINGS:
            L = hip.make_lighting((-1.0, -1.0, -1.0), bool(sh), K, radius, 1)
            ctx.render_lit_triangles_device(f, L, frame.data_ptr(), vis.data_ptr(), sp)
            comps[sname]()
            stream.synchronize()
            out[f"composed_equal_{sname}"] = float((frame.view(-1, 4) == comps[sname].rgba).all(1).float().mean().item())
            out[f"speedup_{sname}"] = out[f"composed_{sname}"] / out[f"lit_{sname}"]
            out["hit_pixels"] = int((vis >= 0).sum().item())
        res["configs"][name] = out
        del comps, runs
        torch.cuda.empty_cache()
    cfg = res["configs"].values()
    res["lit_faster_everywhere"] = all(v[f"lit_{s}"] < v[f"composed_{s}"] for v in cfg for s, _, _ in SETTINGS)
    res["frames_equal"] = all(v[f"composed_equal_{s}"] == 1.0 for v in cfg for s, _, _ in SETTINGS)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    ctx.close()
    return 0 if res["frames_equal"] else 1                          # the check: both routes give the same frame on every pixel


if __name__ == "__main__":
    sys.exit(main())
