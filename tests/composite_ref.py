"""Field compositing (include/rto_hip.h, rto_composite_field_*) restated for the tests, written from the
rule: projection_ref's sort-everything walk for the visited voxels, field_view_ref.lut_index for the index, Python integers for T, R,
G and B, numpy float32 for the six final operations.  No bricks, no tables, no thresholds in the frame.

    valued    valid_lo <= v <= valid_hi
    entry     bytes r, g, b, a of lut[index]; a' = a + (a >> 7); the voxel contributes when a' != 0
    composite T = 65536, R = G = B = 0; per contributing voxel c = (T a') >> 8, R += c r, G += c g, B += c b, T -= c, count += 1
    end       occluded (occlude and the grid's byte is 1: before the voxel contributes), saturated (T <= stop_q16 after a
              contribution) or through
    colour    bg = under[pix], or background_rgba for a visiting pixel and miss_rgba unblended for a miss; tf = float(T) / 65536,
              out = float(R) / 16711680 + tf bg, alpha float(65536 - T) / 65536 + tf bg.a"""
from __future__ import annotations

import numpy as np

import field_view_ref as fr
import projection_ref as pr

F = np.float32
THROUGH, SATURATED, OCCLUDED = 0, 1, 2
SUMMARY_DTYPE = np.dtype([("visited", "<i8"), ("contributing", "<i8"), ("saturated", "<i8"), ("occluded", "<i8")])


def alpha(lut) -> np.ndarray:
    """a' of the 256 entries."""
    a = (np.ascontiguousarray(lut, dtype="<u4") >> np.uint32(24)).astype(np.int64)
    return a + (a >> 7)


def thresholds(s: int, scale: int) -> list:
    """thr[k], k = 0 .. 255, for the span s = hi - lo: LINEAR ceil(k s / 255), SQRT ceil(k k s / 65025), in Python integers."""
    if scale == fr.LINEAR:
        return [-((-k * s) // 255) for k in range(256)]
    return [-((-k * k * s) // 65025) for k in range(256)]


def index_of_thresholds(thr, w) -> np.ndarray:
    """The index of w = clamp(v) - lo from the thresholds: how many of thr[1 .. 255] are <= w."""
    return np.searchsorted(np.asarray(thr[1:], np.int64), np.asarray(w, np.int64), side="right")


def ray(cells, volume, index, grid, comp, lut):
    """One ray's (T, R, G, B, first, stop, count, end, trace) from its visited voxels.  index: the LUT index of every voxel of the
    volume (lut_index over the whole volume, made once per frame); grid: the resident bytes, read when comp.occlude; trace: T
    after every contribution."""
    dz, dy, dx = volume.shape
    ap = alpha(lut)
    b = np.ascontiguousarray(lut, dtype="<u4").view(np.uint8).reshape(256, 4)
    T, R, G, B, first, stop, count, end, trace = 65536, 0, 0, 0, -1, -1, 0, THROUGH, []
    for x, y, z in cells:
        lin = (z * dy + y) * dx + x
        if comp.occlude and int(grid[z, y, x]) == 1:
            end, stop = OCCLUDED, lin
            break
        v = int(volume[z, y, x])
        if not comp.valid_lo <= v <= comp.valid_hi:
            continue
        k = int(index[z, y, x])
        a = int(ap[k])
        if a == 0:
            continue
        c = (T * a) >> 8
        R, G, B, T = R + c * int(b[k, 0]), G + c * int(b[k, 1]), B + c * int(b[k, 2]), T - c
        if count == 0:
            first = lin
        count += 1
        trace.append(T)
        if T <= comp.stop_q16:
            end, stop = SATURATED, lin
            break
    return T, R, G, B, first, stop, count, end, trace


def colour(T, R, G, B, visited, comp, under=None) -> np.ndarray:
    """(n, 4) float32 from the integer states (arrays of n) by the rule's six float32 operations."""
    T, visited = np.asarray(T, np.int64), np.asarray(visited, bool)
    n = len(T)
    if under is not None:
        bg = np.asarray(under, np.float32).reshape(n, 4)
    else:
        bg = np.broadcast_to(np.array(list(comp.background_rgba), np.float32), (n, 4))
    with np.errstate(all="ignore"):
        tf = (T.astype(np.float32) / F(65536)).astype(np.float32)
        out = np.empty((n, 4), np.float32)
        for k, S in enumerate((R, G, B)):
            own = (np.asarray(S, np.int64).astype(np.float32) / F(16711680)).astype(np.float32)
            out[:, k] = (own + (tf * bg[:, k]).astype(np.float32)).astype(np.float32)
        own = ((65536 - T).astype(np.float32) / F(65536)).astype(np.float32)
        out[:, 3] = (own + (tf * bg[:, 3]).astype(np.float32)).astype(np.float32)
    if under is None:
        out[~visited] = np.array(list(comp.miss_rgba), np.float32)
    return out


def index_volume(volume, comp) -> np.ndarray:
    return fr.lut_index(volume, comp.range_lo, comp.range_hi, comp.scale)


def frame_of(cells, W, H, volume, grid, comp, lut, under=None):
    """The composite of a W x H frame from its rays' walks (row-major): (rgba (H, W, 4), transmittance (H, W) uint32, first, stops,
    counts (H, W) int32, summary) and, last, the per-ray ends."""
    index = index_volume(volume, comp)
    res = [ray(c, volume, index, grid, comp, lut) for c in cells]
    visited = np.array([bool(c) for c in cells])
    T = np.array([r[0] for r in res], np.int64)
    rgba = colour(T, [r[1] for r in res], [r[2] for r in res], [r[3] for r in res], visited, comp, under)
    first = np.array([r[4] for r in res], np.int32)
    stops = np.array([r[5] for r in res], np.int32)
    counts = np.array([r[6] for r in res], np.int32)
    ends = np.array([r[7] for r in res], np.int32)
    s = np.zeros(1, SUMMARY_DTYPE)[0]
    s["visited"], s["contributing"] = int(visited.sum()), int((counts > 0).sum())
    s["saturated"], s["occluded"] = int((ends == SATURATED).sum()), int((ends == OCCLUDED).sum())
    return rgba.reshape(H, W, 4), T.astype(np.uint32).reshape(H, W), first.reshape(H, W), stops.reshape(H, W), counts.reshape(H, W), s, ends


def walks(grid_min, voxel, dim, pos, rd, comp=None):
    """projection_ref.walks under the composite's clip box."""
    return pr.walks(grid_min, voxel, dim, pos, rd, comp)
