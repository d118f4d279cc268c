"""The voxel-edit rule (rto_edit_voxels) restated in numpy: the reference the GPU edits are checked against.

Quantisation in float64 from the float32 inputs, one IEEE operation at a time (what rto_brush_quantize computes):
    cq = floor((centre - gridMin) / voxelSize * 64 + 0.5),  eq = floor(extent / voxelSize * 64 + 0.5),  |cq|, eq <= 2^27.
Coverage in int64 with D[a] = 64 (2 i[a] + 1) - 2 cq[a]: a sphere covers voxel i when sum D^2 <= (2 eq[0])^2, a box when
|D[a]| <= 2 eq[a] on every axis.  Brushes apply in order; changed = voxels whose final value differs from the first.
"""
from __future__ import annotations

import numpy as np

SPHERE, BOX = 0, 1
CARVE, FILL = 0, 1
LIMIT = 1 << 27


def quantize(centre, extent, shape, op, grid_min, voxel_size):
    """(cq, eq) as int64 (3,) arrays, or None when the brush is invalid."""
    if shape not in (SPHERE, BOX) or op not in (CARVE, FILL):
        return None
    c = np.asarray(centre, np.float32).astype(np.float64)
    e = np.asarray(extent, np.float32).astype(np.float64)
    g = np.asarray(grid_min, np.float32).astype(np.float64)
    vs = np.float64(np.float32(voxel_size))
    if not (np.isfinite(vs) and vs > 0):
        return None
    if not (np.isfinite(c).all() and np.isfinite(e).all() and np.isfinite(g).all()) or (e < 0).any():
        return None
    with np.errstate(over="ignore", invalid="ignore"):
        fc = np.floor((c - g) / vs * 64.0 + 0.5)
        fe = np.floor(e / vs * 64.0 + 0.5)
    if not ((np.abs(fc) <= LIMIT).all() and (fe <= LIMIT).all()):
        return None
    return fc.astype(np.int64), fe.astype(np.int64)


def cover(dims, shape, cq, eq):
    """Boolean (dimZ, dimY, dimX) mask of the voxels the quantised brush covers."""
    D = [64 * (2 * np.arange(n, dtype=np.int64) + 1) - 2 * cq[a] for a, n in enumerate(dims)]
    bound = [2 * eq[0]] * 3 if shape == SPHERE else [2 * eq[a] for a in range(3)]
    # each term of either test alone must pass: that picks the sub-box worth evaluating (the answer is the same without it)
    idx = [np.nonzero(np.abs(D[a]) <= bound[a])[0] for a in range(3)]
    out = np.zeros((dims[2], dims[1], dims[0]), bool)
    if not all(len(i) for i in idx):
        return out
    sl = tuple(slice(i[0], i[-1] + 1) for i in idx[::-1])
    dx, dy, dz = D[0][sl[2]][None, None, :], D[1][sl[1]][None, :, None], D[2][sl[0]][:, None, None]
    if shape == SPHERE:
        out[sl] = dx * dx + dy * dy + dz * dz <= (2 * eq[0]) ** 2
    else:
        out[sl] = (np.abs(dx) <= bound[0]) & (np.abs(dy) <= bound[1]) & (np.abs(dz) <= bound[2])
    return out


def apply(grid: np.ndarray, brushes, grid_min, voxel_size):
    """(edited copy of the uint8 (dimZ, dimY, dimX) grid, changed).  brushes: BRUSH_DTYPE records; ValueError on an invalid one."""
    out = np.array(grid, np.uint8, copy=True)
    dims = (grid.shape[2], grid.shape[1], grid.shape[0])
    qs = []
    for b in brushes:
        q = quantize(b["centre"], b["extent"], int(b["shape"]), int(b["op"]), grid_min, voxel_size)
        if q is None:
            raise ValueError(f"invalid brush {b}")
        qs.append(q)
    for b, (cq, eq) in zip(brushes, qs):
        out[cover(dims, int(b["shape"]), cq, eq)] = 1 if int(b["op"]) == FILL else 0
    return out, int((out != grid).sum())
