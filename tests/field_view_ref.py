"""Field views (include/rto_hip.h, rto_render_field_*) restated in numpy for the tests, on top of query_ref
(the box query in a window) and lit_ref (the Lambert term, mix32).  Every float operation is one float32 operation in the rule's
order; everything behind the sampled value is int64.

    window   (0, below 1e30), or the clip box's slab test: planes gridMin + float(i) voxel, t_lo = max(0, tNear), t_hi = min(below
             1e30, tFar); a ray that fails tNear <= tFar && tFar > 0 is a miss
    hit      query32's FIRST or CLOSEST record in that window
    voxel    q = floor((p - gridMin) / voxel) of p = o + d tHit, clamped as a float into the leaf, as an int into the clip box; the
             entry face's axis takes the leaf's own boundary voxel; FRONT moves one voxel out across that face
    value    MISS, NONE (no voxel, or outside [valid_lo, valid_hi]) or the volume's value
    index    CATEGORY mix32(v) & 255; else 0 when hi == lo; LINEAR (w 255) // s; SQRT the largest k with k k s <= w 65025
    colour   LUT bytes / 255, times (0.25 + 0.75 ndotl) on r, g, b when shaded; miss_rgba, none_rgba unshaded"""
from __future__ import annotations

import numpy as np

import lit_ref as lr
import query_ref as q

F = np.float32
MISS, NONE = -2 ** 31, -2 ** 31 + 1
HIT, FRONT = 0, 1
LINEAR, SQRT, CATEGORY = 0, 1, 2
SUMMARY_DTYPE = np.dtype([("hits", "<i8"), ("valued", "<i8"), ("vmin", "<i4"), ("vmax", "<i4"), ("lo", "<i4"), ("hi", "<i4")])


def lut_index(v, lo, hi, scale) -> np.ndarray:
    """The LUT index of values v (any integers that fit int32) under the range (lo, hi), in int64."""
    v = np.asarray(v, np.int64)
    if scale == CATEGORY:
        return (lr.mix32((v & 0xFFFFFFFF).astype(np.uint32)) & np.uint32(255)).astype(np.int64)
    lo, hi = int(lo), int(hi)
    s = hi - lo
    if s == 0:
        return np.zeros(v.shape, np.int64)
    w = np.clip(v, lo, hi) - lo
    if scale == LINEAR:
        return (w * 255) // s
    k = np.arange(1, 256, dtype=np.int64)
    return (k[None, :] * k[None, :] * s <= (w.reshape(-1, 1) * 65025)).sum(1).reshape(v.shape)


def lut_colours(lut) -> np.ndarray:
    """(256, 4) float32: each byte of an entry, r g b a in memory order, as float(byte) / 255."""
    b = np.ascontiguousarray(lut, dtype="<u4").view(np.uint8).reshape(256, 4)
    return (b.astype(np.float32) / F(255)).astype(np.float32)


def window(grid_min, voxel, o, inv, view):
    """(t_lo, t_hi, passes) of every ray."""
    n = len(inv)
    tlo, thi, ok = np.zeros(n, np.float32), np.full(n, q.BELOW_1E30, np.float32), np.ones(n, bool)
    if view.clip:
        g, vs = np.asarray(grid_min, np.float32).reshape(3), F(voxel)
        lo = (g + (np.array(list(view.clip_lo), np.float32) * vs).astype(np.float32)).astype(np.float32)
        hi = (g + (np.array(list(view.clip_hi), np.float32) * vs).astype(np.float32)).astype(np.float32)
        with np.errstate(all="ignore"):
            t1 = ((lo[None, :] - o).astype(np.float32) * inv).astype(np.float32)
            t2 = ((hi[None, :] - o).astype(np.float32) * inv).astype(np.float32)
            tmin, tmax = q.gmin(t1, t2), q.gmax(t1, t2)
            tn = q.gmax(q.gmax(tmin[:, 0], tmin[:, 1]), tmin[:, 2])
            tf = q.gmin(q.gmin(tmax[:, 0], tmax[:, 1]), tmax[:, 2])
            ok = (tn <= tf) & (tf > 0)
            tlo = q.gmax(F(0), tn).astype(np.float32)
            thi = q.gmin(q.BELOW_1E30, tf).astype(np.float32)
    return tlo, thi, ok


def sample(T: q.Tree32, grid_min, voxel, pos, rd, volume, view):
    """(values (n,) int32, ndotl (n,) float32, the hit records) of the rays (pos, rd)."""
    d = np.asarray(rd, np.float32).reshape(-1, 3)
    n = len(d)
    o = np.broadcast_to(np.asarray(pos, np.float32).reshape(-1, 3), d.shape)
    g, vs = np.asarray(grid_min, np.float32).reshape(3), F(voxel)
    with np.errstate(all="ignore"):
        inv = (F(1) / d).astype(np.float32)
    tlo, thi, ok = window(g, vs, o, inv, view)
    # rays outside the clip box get a window no leaf can meet
    hits = q.query32(T, o, d, np.where(ok, tlo, F(1)), np.where(ok, thi, F(0)))[view.mode]
    hit = hits["node"] >= 0
    values = np.full(n, MISS, np.int64)
    h = np.nonzero(hit)[0]
    leaf_lo = np.stack([hits["x"][h], hits["y"][h], hits["z"][h]], 1).astype(np.int64)
    leaf_hi = leaf_lo + hits["size"][h].astype(np.int64)[:, None] - 1
    t = hits["t"][h].astype(np.float32)
    with np.errstate(all="ignore"):
        p = (o[h] + (d[h] * t[:, None]).astype(np.float32)).astype(np.float32)
        qf = np.floor(((p - g[None, :]).astype(np.float32) / vs).astype(np.float32))
    flo, fhi = leaf_lo.astype(np.float32), leaf_hi.astype(np.float32)
    qf = np.where(qf >= flo, qf, flo)
    qf = np.where(qf > fhi, fhi, qf)
    vox = qf.astype(np.int64)
    if view.clip:
        vox = np.clip(vox, np.array(list(view.clip_lo), np.int64)[None, :], np.array(list(view.clip_hi), np.int64)[None, :] - 1)
    face = hits["face"][h].astype(np.int64)
    onface = face >= 0
    a = np.where(onface, face >> 1, 0)
    up = (face & 1) == 1
    rows = np.arange(len(h))
    edge = np.where(up, leaf_hi[rows, a], leaf_lo[rows, a])
    if view.sample == FRONT:
        edge = edge + np.where(up, 1, -1)
    vox[rows, a] = np.where(onface, edge, vox[rows, a])
    have = np.ones(len(h), bool) if view.sample == HIT else onface.copy()
    dz, dy, dx = volume.shape
    have &= (vox >= 0).all(1) & (vox[:, 0] < dx) & (vox[:, 1] < dy) & (vox[:, 2] < dz)
    val = np.full(len(h), NONE, np.int64)
    vv = volume[vox[have, 2], vox[have, 1], vox[have, 0]].astype(np.int64)
    val[have] = np.where((vv >= view.valid_lo) & (vv <= view.valid_hi), vv, NONE)
    values[h] = val
    # shade_term: the leaf's own tHit = max(0, tNear of its box), whatever the window did
    own = hits.copy()
    if len(h):
        tn = T.slab(o[h], inv[h], hits["node"][h])[0]
        own["t"][h] = q.gmax(F(0), tn).astype(np.float32)
    ndotl = lr.ndotl32(T, o, d, own, lr.light_neg((-1.0, -1.0, -1.0)))
    return values.astype(np.int32), ndotl, hits


def colour(values, ndotl, view, lut):
    """(rgba (n, 4) float32, summary record, bins (256,) int64) of sampled values."""
    values = np.asarray(values, np.int32).astype(np.int64)
    hit = values != MISS
    valued = hit & (values != NONE)
    v = values[valued]
    s = np.zeros(1, SUMMARY_DTYPE)[0]
    s["hits"], s["valued"] = int(hit.sum()), int(valued.sum())
    if len(v):
        s["vmin"], s["vmax"] = int(v.min()), int(v.max())
    auto = view.range_lo == view.range_hi
    s["lo"], s["hi"] = (s["vmin"], s["vmax"]) if auto else (view.range_lo, view.range_hi)
    k = lut_index(v, s["lo"], s["hi"], view.scale)
    bins = np.bincount(k, minlength=256).astype(np.int64)
    rgba = np.empty((len(values), 4), np.float32)
    rgba[~hit] = np.array(list(view.miss_rgba), np.float32)
    rgba[hit & ~valued] = np.array(list(view.none_rgba), np.float32)
    c = lut_colours(lut)[k]
    if view.shade:
        m = (F(0.25) + (F(0.75) * np.asarray(ndotl, np.float32)[valued]).astype(np.float32)).astype(np.float32)
        c = c.copy()
        c[:, :3] = (c[:, :3] * m[:, None]).astype(np.float32)
    rgba[valued] = c
    return rgba, s, bins


def frame(T: q.Tree32, grid_min, voxel, pos, rd, W, H, volume, view, lut):
    """The field view of a W x H frame whose pixel rays are rd ((H W, 3), row-major): (rgba (H, W, 4), values (H, W), summary,
    bins)."""
    values, ndotl, _ = sample(T, grid_min, voxel, pos, rd, volume, view)
    rgba, s, bins = colour(values, ndotl, view, lut)
    return rgba.reshape(H, W, 4), values.reshape(H, W), s, bins


def degenerate(values, view) -> bool:
    """Fewer than 20 valued pixels, or fewer than two distinct LUT indices among them."""
    v = np.asarray(values, np.int64).ravel()
    v = v[(v != MISS) & (v != NONE)]
    if len(v) < 20:
        return True
    auto = view.range_lo == view.range_hi
    lo, hi = (v.min(), v.max()) if auto else (view.range_lo, view.range_hi)
    return len(np.unique(lut_index(v, lo, hi, view.scale))) < 2
