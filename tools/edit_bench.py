#!/usr/bin/env python3
"""Voxel edits against a host rebuild, on one GPU (rto_edit_voxels): prints one JSON line per scene and brush radius.

Scenes: config 2's 256^3 test sphere (octree only) and config 5's 512^3 test sphere with its leaf triangles.  Brushes: a CARVE
sphere of radius 4, 16 and 64 voxels centred on the surface point a FIRST pixel query finds at the frame's centre
(Camera(0.5, 0.7, 1.8), fov 45).  Every round first restores the original scene (untimed), then alternates, in one process:
  edit     Context.edit_voxels([brush]): device ms of the brush kernel, the octree rebuild and the triangle rebuild
           (rto_last_edit_ms) and the wall time to its synchronised return
  rebuild  the comparator: rto_build_octree of the same edited grid from the host (+ rto_build_leaf_triangles for config 5),
           wall time to a synchronised return, with its device ms (rto_last_build_ms)
Medians over --rounds rounds.  Kernel times for the profile: rocprofv3 --kernel-trace --stats -- python3 tools/edit_bench.py"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from oracle import orc   # the scene generator the tests and bench.py use
from ray_tracing_octrees_amd import hip


def surface_point(ctx, dim, W=512, H=512):
    cam = orc.Camera(0.5, 0.7, 1.8)
    view, pos = cam.get_view(), cam.get_pos()
    f = hip.make_frame(view, pos, W / H, 45.0, W, H)
    h = ctx.query_pixels(f, [[W // 2, H // 2]], hip.QUERY_FIRST)[0]
    if h["node"] < 0:
        raise RuntimeError("the centre pixel misses the scene")
    d = orc.generate_rays(view, pos, W / H, 45.0, W, H).reshape(H, W, 3)[H // 2, W // 2]
    return (np.asarray(pos, np.float32) + d * np.float32(h["t"])).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--radii", default="4,16,64")
    ap.add_argument("--scenes", default="256,512")
    a = ap.parse_args()
    ctx = hip.Context(0)
    for dim in (int(x) for x in a.scenes.split(",")):
        tris = dim == 512
        g = orc.test_sphere_grid(dim)
        data = np.ascontiguousarray(g.data, np.uint8)

        def restore():
            ctx.build_octree(data, g.min, g.voxel_size)
            if tris:
                ctx.build_leaf_triangles(None)

        restore()
        point = surface_point(ctx, dim)
        for r in (float(x) for x in a.radii.split(",")):
            brush = hip.make_brushes([point], r * float(g.voxel_size), hip.BRUSH_SPHERE, hip.EDIT_CARVE)
            edited, changed = None, None
            ew, ems, hw, hms = [], [], [], []
            for k in range(a.rounds + 1):                   # round 0 warms both paths up and is dropped
                restore()
                ctx.synchronize()
                t0 = time.perf_counter()
                n = ctx.edit_voxels(brush)
                t1 = time.perf_counter()
                ms = ctx.last_edit_ms()
                if edited is None:
                    edited, changed = ctx.download_voxels(), n
                assert n == changed
                ctx.synchronize()
                t2 = time.perf_counter()
                ctx.build_octree(edited, g.min, g.voxel_size)
                bk, bu = ctx.last_build_ms()
                tk = 0.0
                if tris:
                    ctx.build_leaf_triangles(None)
                    tk = ctx.last_build_ms()[0]
                t3 = time.perf_counter()
                if k:
                    ew.append((t1 - t0) * 1e3); ems.append(ms)
                    hw.append((t3 - t2) * 1e3); hms.append((bk, bu, tk))
            ems, hms = np.array(ems), np.array(hms)
            print(json.dumps({
                "scene": f"sphere{dim}" + (" + triangles" if tris else ""), "radius_voxels": r, "changed": changed,
                "rounds": a.rounds,
                "edit_wall_ms": round(float(np.median(ew)), 4),
                "edit_device_ms": {"brushes": round(float(np.median(ems[:, 0])), 4), "octree": round(float(np.median(ems[:, 1])), 4),
                                   "triangles": round(float(np.median(ems[:, 2])), 4) if tris else None},
                "host_rebuild_wall_ms": round(float(np.median(hw)), 4),
                "host_rebuild_device_ms": {"octree_kernels": round(float(np.median(hms[:, 0])), 4), "upload": round(float(np.median(hms[:, 1])), 4),
                                           "triangles": round(float(np.median(hms[:, 2])), 4) if tris else None},
                "speedup_wall": round(float(np.median(hw) / np.median(ew)), 2),
            }), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
