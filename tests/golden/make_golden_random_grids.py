"""Generates tests/golden/ref_random_grids.npz.  Run ONLY where the reference checkout is present (oracle/Makefile REF):

    make -C oracle ref refvr && python tests/golden/make_golden_random_grids.py

Inputs and outputs of the REFERENCE'S OWN compiled code, so that the suite pins the oracle (and the HIP path) to it on
machines without the reference checkout:
  octree_<i>_*   random grids (the draws of the former live test, seed 99) and the flat octree the reference builds from
                 each: createOctreeFromVoxelGrid + setOctree's BFS numbering (orc.ref_build_flat_octree)
  skip_<i>_*     random grids, rays and visibility maps (seed 321) and the reference's octreeRaySkip distances for them,
                 without (`out`) and with (`out_vis`) the visibility map
  dropin_*       what the reference host stack hands the HIP path in main.cpp's sphere scene: the 64^3 shell sphere's flat
                 octree and Camera(0.5, 0.7, 1.8)'s view matrix and position
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import orc  # noqa: E402

OCTREE_GRIDS = (((7, 5, 3), 0.5), ((16, 16, 16), 0.1), ((33, 9, 20), 0.9), ((1, 1, 1), 1.0), ((2, 3, 1), 0.0))
SKIP_GRIDS = (((7, 5, 3), 0.5), ((16, 16, 16), 0.1), ((33, 9, 20), 0.7), ((2, 3, 1), 1.0))
GRID_MIN = np.array([0.5, -2.0, 3.0], np.float32)
VOXEL = np.float32(0.3)


def main():
    assert orc.ref_available() and orc.refvr_available(), "make -C oracle ref refvr first"
    out = {}
    rng = np.random.default_rng(99)
    for i, (dims, p) in enumerate(OCTREE_GRIDS):
        data = (rng.random((dims[2], dims[1], dims[0])) < p).astype(np.uint8)
        g = orc.Grid(dims, GRID_MIN, VOXEL, data)
        out[f"octree_{i}_data"] = data
        out[f"octree_{i}_nodes"] = orc.ref_build_flat_octree(g)

    rng = np.random.default_rng(321)
    for i, (dims, p) in enumerate(SKIP_GRIDS):
        data = (rng.random((dims[2], dims[1], dims[0])) < p).astype(np.uint8)
        g = orc.Grid(dims, GRID_MIN, VOXEL, data)
        nodes = orc.build_flat_octree(g)
        ro = np.array([4.0, 1.5, -3.0], np.float32)
        rd = rng.normal(size=(200, 3)).astype(np.float32)
        rd /= np.linalg.norm(rd, axis=1, keepdims=True).astype(np.float32)
        rd[:6] = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [1e-11, 1, 0], [-0.0, 0, -1], [1, 1e-9, -1e-11]], np.float32)
        flags = (rng.random(len(nodes)) < 0.8).astype(np.uint8)
        flags[0] = 1
        out[f"skip_{i}_data"] = data
        out[f"skip_{i}_ro"] = ro
        out[f"skip_{i}_rd"] = rd
        out[f"skip_{i}_flags"] = flags
        out[f"skip_{i}_out"] = orc.ref_octree_ray_skip(g, ro, rd, 0.0, 1e30, visible=None)
        out[f"skip_{i}_out_vis"] = orc.ref_octree_ray_skip(g, ro, rd, 0.0, 1e30, visible=flags)

    g = orc.test_sphere_grid(64)
    view, pos, _ = orc.ref_camera(0.5, 0.7, 1.8)
    out["dropin_nodes"] = orc.ref_build_flat_octree(g)
    out["dropin_min"] = g.min
    out["dropin_voxel"] = np.float32(g.voxel_size)
    out["dropin_view"] = view
    out["dropin_pos"] = pos

    path = os.path.join(HERE, "ref_random_grids.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
