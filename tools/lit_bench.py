#!/usr/bin/env python3
"""The lit render (rto_render_lit_device) against the route integrators compose today; prints one JSON line.

Frames: BASELINE config 2 (256^3 test sphere, Camera(0.5, 0.7, 1.8)) and config 4 (the Calgary grid, the oblique camera
Camera(0.6, 0.5, 3500)), 1920x1080, fov 45, light (-1, -1, -1).  Settings: the shadow ray alone, shadow + K = 8 and shadow + K = 32
AO rays of 4 voxels.  Per frame and setting, alternated within every round of one process:
  render    rto_render_device (no terms), for context
  lit       rto_render_lit_device (compacted hits, secondary rays built in registers)
  composed  rto_query_pixels_device FIRST over every pixel; the hit pixels compacted (torch.nonzero) and their 1 + K rays built
            with torch on the device by the same rule into 32-byte rto_ray records; rto_query_rays_device
            ANY on them; shading with torch.  Its frame is compared with the lit frame (`composed_equal`: share of equal pixels).
Times are device events around `reps` frames on one stream, medians of `rounds` rounds.  Kernel times: rocprofv3 --kernel-trace
--stats -- python3 tools/lit_bench.py --rounds 2"""
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
from oracle import orc

SETTINGS = (("shadow", 1, 0), ("shadow_k8", 1, 8), ("shadow_k32", 1, 32))


def timed_ms(fn, reps, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / reps


class Composed:
    """The integrator's route, on the device with torch (one stream)."""

    def __init__(self, ctx, frame, view, pos, gmin, voxel, light, K, radius, seed, stream):
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
        self.gmin = torch.from_numpy(np.asarray(gmin, np.float32)).to(dev)
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
        self.ctx.query_pixels_device(hip.QUERY_FIRST, self.f, self.xy.data_ptr(), self.npix, self.hits.data_ptr(), sp)
        with torch.cuda.stream(self.stream):
            rec = self.hits.view(self.npix, 8)
            node, face = rec[:, 1], rec[:, 2]
            hidx = torch.nonzero(node >= 0).squeeze(1)
            r = rec[hidx]
            t = r[:, 0].view(torch.float32)
            size = r[:, 3].float()
            xyz = r[:, 4:7].float()
            d = self.dirs[hidx]
            p = self.pos + d * t[:, None]
            mn = self.gmin + xyz * self.vs
            mx = mn + (size * self.vs)[:, None]
            q = p - 0.5 * (mn + mx)
            nrm = q * (1.0 / torch.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]))[:, None]
            ndotl = torch.clamp((nrm[:, 0] * self.lneg[0] + nrm[:, 1] * self.lneg[1]) + nrm[:, 2] * self.lneg[2], min=0.0)
            fc = r[:, 2]
            ok = fc >= 0
            a = torch.where(ok, fc >> 1, torch.zeros_like(fc)).long()
            up = (fc & 1) == 1
            hm = p.abs().amax(1)
            eps = self.vs * 1e-3 + hm * 2.0 ** -18
            rows = torch.arange(len(hidx), device=p.device)
            plane = torch.where(up, mx[rows, a] + eps, mn[rows, a] - eps)
            so = p.clone()
            so[rows, a] = plane
            n = len(hidx)
            rays = torch.zeros(n, 1 + K, 8, dtype=torch.float32, device=p.device)
            rays[:, :, 0:3] = so[:, None, :]
            cast = ok & (ndotl > 0)
            rays[:, 0, 4:7] = self.lneg
            rays[:, 0, 7] = torch.where(cast, torch.tensor(1e30, device=p.device), torch.tensor(-1.0, device=p.device))
            if K:
                h = self._mix(((self.px[hidx] * 0x8DA6B343) & 0xFFFFFFFF) ^ ((self.py[hidx] * 0xD8163841) & 0xFFFFFFFF)
                              ^ ((self.seed * 0xCB1AB31F) & 0xFFFFFFFF))
                s = torch.arange(K, device=p.device)
                e = (h[:, None] + (64 * s)[None, :] // K) & 63
                tt = self.table[e]
                u = torch.where(((h >> 6) & 1).bool()[:, None], -tt[..., 0], tt[..., 0])
                v = torch.where(((h >> 7) & 1).bool()[:, None], -tt[..., 1], tt[..., 1])
                nz = torch.where(up[:, None], tt[..., 2], -tt[..., 2])
                ax = a[:, None]
                rays[:, 1:, 4] = torch.where(ax == 0, nz, torch.where(ax == 1, v, u))
                rays[:, 1:, 5] = torch.where(ax == 0, u, torch.where(ax == 1, nz, v))
                rays[:, 1:, 6] = torch.where(ax == 0, v, torch.where(ax == 1, u, nz))
                rays[:, 1:, 7] = torch.where(ok[:, None], torch.tensor(float(self.radius), device=p.device),
                                             torch.tensor(-1.0, device=p.device))
            out = torch.empty(n * (1 + K) * 8, dtype=torch.int32, device=p.device)
        self.ctx.query_rays_device(hip.QUERY_ANY, rays.data_ptr(), n * (1 + K), out.data_ptr(), sp)
        with torch.cuda.stream(self.stream):
            hit = (out.view(n, 1 + K, 8)[:, :, 1] >= 0)
            S = ~hit[:, 0]
            occ = hit[:, 1:].sum(1)
            A = ((K - occ).float() / K) if K else torch.ones(n, device=p.device)
            dd = torch.where(S, ndotl, torch.zeros_like(ndotl))
            amb = 0.1 * A
            self.rgba.zero_()
            self.rgba[:, 3] = 1.0
            col = torch.stack([1.0 * dd + amb, 0.8 * dd + amb, 0.6 * dd + amb, torch.ones_like(dd)], 1)
            self.rgba[hidx] = col


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    ctx = rto.Context(0)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    W, H = 1920, 1080
    res = {"frame": [W, H], "rounds": a.rounds, "reps": a.reps, "configs": {}}
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_scene_cache.npz"))
    dims = tuple(int(x) for x in z["dims"])
    cal = np.unpackbits(z["packed"])[: dims[0] * dims[1] * dims[2]].reshape(dims[2], dims[1], dims[0])
    scenes = {"config2": (rto.VoxelGrid.test_sphere(256), rto.Camera(0.5, 0.7, 1.8)),
              "config4": (rto.VoxelGrid.from_array(cal, z["min"].astype(np.float32), np.float32(z["voxel"])), rto.Camera(0.6, 0.5, 3500.0))}
    for name, (g, cam) in scenes.items():
        ctx.build_octree(g.data, g.min, g.voxelSize)
        view, pos = cam.getView(), cam.getPos()
        f = rto.make_frame(view, pos, W / H, 45.0, W, H)
        frame = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda")
        vis = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        radius = float(np.float32(4 * float(g.voxelSize)))
        runs = {"render": lambda: ctx.render_device(f, frame.data_ptr(), None, sp)}
        comps = {}
        for sname, sh, K in SETTINGS:
            L = hip.make_lighting((-1.0, -1.0, -1.0), bool(sh), K, radius, 1)
            runs[f"lit_{sname}"] = (lambda L=L: ctx.render_lit_device(f, L, frame.data_ptr(), vis.data_ptr(), sp))
            comps[sname] = Composed(ctx, f, view, pos, g.min, g.voxelSize, (-1.0, -1.0, -1.0), K, radius, 1, stream)
            runs[f"composed_{sname}"] = comps[sname]
        for fn in runs.values():                                    # warm-up: tables, work buffers, allocator
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                times[k].append(timed_ms(fn, a.reps, stream))
        out = {k: float(np.median(v)) for k, v in times.items()}
        for sname, sh, K in SETTINGS:
            L = hip.make_lighting((-1.0, -1.0, -1.0), bool(sh), K, radius, 1)
            ctx.render_lit_device(f, L, frame.data_ptr(), vis.data_ptr(), sp)
            comps[sname]()
            stream.synchronize()
            lit = frame.view(-1, 4)
            out[f"composed_equal_{sname}"] = float((lit == comps[sname].rgba).all(1).float().mean().item())
            out[f"speedup_{sname}"] = out[f"composed_{sname}"] / out[f"lit_{sname}"]
            out[f"hit_pixels"] = int((vis >= 0).sum().item())
        res["configs"][name] = out
    res["lit_faster_everywhere"] = all(v[f"lit_{s}"] < v[f"composed_{s}"] for v in res["configs"].values() for s, _, _ in SETTINGS)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
