"""Field projections (include/rto_hip.h, rto_project_field_*) restated for the tests: numpy float32 for the
plane parameters, Python integers for everything else.  Written from the rule, not from the kernel: every event is collected, the
events are sorted by (T, axis, order), the walk is filtered by the box and reduced.  No bricks, no entry by rank, no jump.

    planes   P_a(j) = gridMin[a] + float(j) voxel, T_a(j) = (P_a(j) - o[a]) inv[a], inv = 1 / d, each one float32 operation
    still    inv[a] not finite: the coordinate is floor((o[a] - gridMin[a]) / voxel), no events
    events   (T, a, k) for T > 0, k the plane's place in the axis' direction of travel; sorted
    states   crossed - 1 (inv > 0) or dim - crossed, from the planes with T <= 0 on
    visited  the states inside [lo, hi) on every axis, in walk order
    value    MISS (nothing visited), NONE (nothing valued), else MAX, MIN, floor(sum / count), count or the first valued value"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import field_view_ref as fr

F = np.float32
MISS, NONE = fr.MISS, fr.NONE
MAX, MIN, MEAN, COUNT, FIRST = 0, 1, 2, 3, 4
OPS = (MAX, MIN, MEAN, COUNT, FIRST)


def plane_t(grid_min, voxel, dim, o, inv, a) -> np.ndarray:
    """T_a(j) for j = 0 .. dim[a], float32."""
    j = np.arange(dim[a] + 1, dtype=np.float32)
    with np.errstate(all="ignore"):
        p = (F(grid_min[a]) + (j * F(voxel)).astype(np.float32)).astype(np.float32)
        return ((p - F(o[a])).astype(np.float32) * F(inv[a])).astype(np.float32)


def walk(grid_min, voxel, dim, o, d, lo=None, hi=None):
    """The visited voxels (x, y, z) of one ray in walk order."""
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    lo = (0, 0, 0) if lo is None else lo
    hi = tuple(dim) if hi is None else hi
    with np.errstate(all="ignore"):
        inv = (F(1) / d).astype(np.float32)
    if not np.isfinite(o).all() or not np.isfinite(inv).any():
        return []
    c, step, events = [0, 0, 0], [0, 0, 0], []
    for a in range(3):
        if not np.isfinite(inv[a]):
            with np.errstate(all="ignore"):
                q = np.floor(((o[a] - F(grid_min[a])).astype(np.float32) / F(voxel)).astype(np.float32))
            if not (q >= lo[a] and q < hi[a]):
                return []
            c[a] = int(q)
            continue
        T = plane_t(grid_min, voxel, dim, o, inv, a)
        up = bool(inv[a] > 0)
        crossed = int((T <= 0).sum())
        c[a] = crossed - 1 if up else dim[a] - crossed
        step[a] = 1 if up else -1
        order = range(dim[a] + 1) if up else range(dim[a], -1, -1)
        events += [(float(T[j]), a, k) for k, j in enumerate(order) if T[j] > 0]
    events.sort()
    inside = lambda: all(lo[a] <= c[a] < hi[a] for a in range(3))
    out = [tuple(c)] if inside() else []
    for _, a, _ in events:
        c[a] += step[a]
        if inside():
            out.append(tuple(c))
    return out


def reduce(cells, volume, op, valid_lo, valid_hi):
    """(value, voxel, sum, count) of one ray's visited voxels; volume is (dimZ, dimY, dimX)."""
    if not cells:
        return MISS, -1, 0, 0
    dz, dy, dx = volume.shape
    valued = []
    for x, y, z in cells:
        v = int(volume[z, y, x])
        if valid_lo <= v <= valid_hi:
            valued.append((v, (z * dy + y) * dx + x))
    if not valued:
        return NONE, -1, 0, 0
    vals = [v for v, _ in valued]
    total, n = sum(vals), len(vals)
    if op == MAX:
        value = max(vals)
    elif op == MIN:
        value = min(vals)
    elif op == MEAN:
        value = total // n                       # Python's // floors towards minus infinity
    elif op == COUNT:
        value = n
    else:
        value = vals[0]
    voxel = valued[vals.index(value)][1] if op in (MAX, MIN) else valued[0][1]
    return value, voxel, total, n


def colour_view(proj):
    """What field_view_ref.colour reads of a view, from an rto_field_projection: the same rules, unshaded."""
    return SimpleNamespace(range_lo=proj.range_lo, range_hi=proj.range_hi, scale=proj.scale, shade=0,
                           miss_rgba=list(proj.miss_rgba), none_rgba=list(proj.none_rgba))


def walks(grid_min, voxel, dim, pos, rd, proj=None):
    """The visited voxels of every ray of rd ((n, 3)), under proj's clip box; a frame's walks do not depend on the volume."""
    lo = tuple(proj.clip_lo) if proj is not None and proj.clip else None
    hi = tuple(proj.clip_hi) if proj is not None and proj.clip else None
    return [walk(grid_min, voxel, dim, pos, d, lo, hi) for d in np.asarray(rd, np.float32).reshape(-1, 3)]


def frame_of(cells, W, H, volume, proj, lut):
    """The projection of a W x H frame from its rays' walks (row-major): (rgba (H, W, 4), values, voxels, sums, counts (H, W
    each), summary, bins)."""
    res = [reduce(c, volume, proj.op, proj.valid_lo, proj.valid_hi) for c in cells]
    values = np.array([r[0] for r in res], np.int64).astype(np.int32)
    voxels = np.array([r[1] for r in res], np.int32)
    sums = np.array([r[2] for r in res], np.int64)
    counts = np.array([r[3] for r in res], np.int32)
    rgba, s, bins = fr.colour(values, None, colour_view(proj), lut)
    return rgba.reshape(H, W, 4), values.reshape(H, W), voxels.reshape(H, W), sums.reshape(H, W), counts.reshape(H, W), s, bins


def frame(grid_min, voxel, pos, rd, W, H, volume, proj, lut):
    """The same from the pixel rays rd ((H W, 3), row-major)."""
    dz, dy, dx = volume.shape
    return frame_of(walks(grid_min, voxel, (dx, dy, dz), pos, rd, proj), W, H, volume, proj, lut)


def degenerate(values, proj) -> bool:
    return fr.degenerate(values, colour_view(proj))
