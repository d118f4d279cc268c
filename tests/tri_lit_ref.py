"""The lit render of the triangle surface (include/rto_hip.h, rto_render_lit_triangles_*) restated in numpy
float32 for the tests, written from the rule, not from the kernels: the primary hit is tri_query_ref's FIRST record on the frame's
pixel ray, the shadow and AO rays are its ANY rule, and hash, table, light and colour are lit_ref's.  Every operation is one
float32 operation, in the order the header writes it.

    n = the record's normal (stored, turned against the ray); ndotl = max(0, (n.x l.x + n.y l.y) + n.z l.z), l = lightNeg
    so = tri_query_ref.shadow_rays' origin: p = o + d t, eps = voxelSize 1e-3 + 2^-18 max|p|, so = p + n (eps - (p - v0) . n)
    shadow (shadow, ndotl > 0): ANY from so along lightNeg, (0, 1e30); S = 0 on a hit
    AO (K > 0): K ANY rays from so, (0, radius]; entry T[(h + 64 s // K) & 63], x' = -T.x if h bit 6, y' = -T.y if h bit 7, z' = T.z
        s = -1 if n.z < 0 else 1; a = -1 / (s + n.z); b = (n.x n.y) a
        U = (1 + ((s n.x) n.x) a, s b, (-s) n.x); V = (b, s + (n.y n.y) a, -n.y); dir = (x' U + y' V) + z' n, per component
    a secondary ray with a NaN or infinite component in its origin or direction is a miss
    colour: d = S ? ndotl : 0, amb = 0.1 A, A = (K - occ) / K; (d + amb, 0.8 d + amb, 0.6 d + amb, 1); a miss is (0, 0, 0, 1)
    vis: -1 for a miss, else occ + 256 (shadow ray cast and blocked)"""
from __future__ import annotations

import numpy as np

import lit_ref as lr
import query_ref as q
import tri_query_ref as tq

F = np.float32
U32 = np.uint32


def ndotl32(hits, lneg) -> np.ndarray:
    """max(0, n . lightNeg) of records (tri_query_ref.lambert with the caller's light); 0 for a miss."""
    n = np.stack([hits["nx"], hits["ny"], hits["nz"]], 1).astype(np.float32)
    l = np.asarray(lneg, np.float32)
    with np.errstate(all="ignore"):
        dot = ((n[:, 0] * l[0] + n[:, 1] * l[1]).astype(np.float32) + n[:, 2] * l[2]).astype(np.float32)
    nl = np.where(F(0) < dot, dot, F(0)).astype(np.float32)              # glm max(0, dot): 0 unless 0 < dot (NaN gives 0)
    return np.where(hits["tri"] >= 0, nl, F(0)).astype(np.float32)


def tangent_frame(n):
    """(U, V) of Duff et al.'s branch-free basis around n (m, 3), float32, one operation per operator."""
    n = np.asarray(n, np.float32).reshape(-1, 3)
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(all="ignore"):
        s = np.where(nz < 0, F(-1), F(1)).astype(np.float32)
        a = (F(-1) / (s + nz).astype(np.float32)).astype(np.float32)
        b = ((nx * ny).astype(np.float32) * a).astype(np.float32)
        ux = (F(1) + (((s * nx).astype(np.float32) * nx).astype(np.float32) * a).astype(np.float32)).astype(np.float32)
        uy = (s * b).astype(np.float32)
        uz = ((-s) * nx).astype(np.float32)
        vx = b
        vy = (s + ((ny * ny).astype(np.float32) * a).astype(np.float32)).astype(np.float32)
        vz = (-ny).astype(np.float32)
    return np.stack([ux, uy, uz], 1), np.stack([vx, vy, vz], 1)


def ao_dirs(table, h, n, K) -> np.ndarray:
    """(m, K, 3) AO directions of m hits with hashes h and turned normals n."""
    table = np.asarray(table, np.float32).reshape(lr.AO_MAX, 3)
    s = np.arange(K, dtype=np.int64)
    e = (h.astype(np.int64)[:, None] + (64 * s)[None, :] // K) & 63
    t = table[e]                                                          # (m, K, 3)
    x = np.where(((h >> U32(6)) & U32(1)).astype(bool)[:, None], -t[..., 0], t[..., 0]).astype(np.float32)
    y = np.where(((h >> U32(7)) & U32(1)).astype(bool)[:, None], -t[..., 1], t[..., 1]).astype(np.float32)
    z = t[..., 2]
    Uv, Vv = tangent_frame(n)
    n = np.asarray(n, np.float32).reshape(-1, 3)
    out = np.empty(t.shape, np.float32)
    with np.errstate(all="ignore"):
        for c in range(3):
            xy = ((x * Uv[:, None, c]).astype(np.float32) + (y * Vv[:, None, c]).astype(np.float32)).astype(np.float32)
            out[..., c] = (xy + (z * n[:, None, c]).astype(np.float32)).astype(np.float32)
    return out


def _any(T, tris, off, o, d, t_max):
    """ANY's hit mask; rays with a non-finite origin or direction component miss."""
    ok = np.isfinite(o).all(1) & np.isfinite(d).all(1)
    hit = np.zeros(len(d), bool)
    if ok.any():
        hit[ok] = tq.query_tri32(T, tris, off, o[ok], d[ok], 0.0, t_max)[tq.ANY]["tri"] >= 0
    return hit


def tri_lit32(T: q.Tree32, tris, off, voxel, o, d, x, y, table, light_dir=(-1.0, -1.0, -1.0), shadow=True, K=0, radius=1.0, seed=0,
              rays_out=None, first=None):
    """The lit pixels (x, y) whose pixel rays are (o, d): (rgba (n, 4) float32, vis (n,) int32).  rays_out (a dict) receives the
    primary records ("first") and the secondary rays ("shadow": (origins, dirs, blocked, pixel rows), "ao": (origins, dirs, hit)).
    first: FIRST records computed before (the same for every lighting)."""
    tris = np.asarray(tris, np.float32).reshape(-1, 12)
    d = np.asarray(d, np.float32).reshape(-1, 3)
    n = len(d)
    lneg = lr.light_neg(light_dir)
    hits = tq.query_tri32(T, tris, off, o, d)[tq.FIRST] if first is None else first
    hit = hits["tri"] >= 0
    ndotl = ndotl32(hits, lneg)
    so, _ = tq.shadow_rays(o, d, hits, tris, voxel)
    nrm = np.stack([hits["nx"], hits["ny"], hits["nz"]], 1).astype(np.float32)
    occ = np.zeros(n, np.int64)
    blocked = np.zeros(n, bool)
    cast = bool(shadow) & hit & (ndotl > 0)
    if rays_out is not None:
        rays_out["first"] = hits
    if cast.any():
        ci = np.nonzero(cast)[0]
        sd = np.broadcast_to(lneg, (len(ci), 3)).copy()
        blocked[ci] = _any(T, tris, off, so[ci], sd, 1e30)
        if rays_out is not None:
            rays_out["shadow"] = (so[ci], sd, blocked[ci], ci)
    if K > 0 and hit.any():
        ai = np.nonzero(hit)[0]
        h = lr.pixel_hash(np.asarray(x)[ai], np.asarray(y)[ai], seed)
        dirs = ao_dirs(table, h, nrm[ai], K).reshape(-1, 3)
        orig = np.repeat(so[ai], K, axis=0)
        ah = _any(T, tris, off, orig, dirs, F(radius))
        occ[ai] = ah.reshape(len(ai), K).sum(1)
        if rays_out is not None:
            rays_out["ao"] = (orig, dirs, ah)
    A = ((K - occ).astype(np.float32) / F(K)).astype(np.float32) if K > 0 else np.ones(n, np.float32)
    dd = np.where(~blocked, ndotl, F(0)).astype(np.float32)
    amb = (F(0.1) * A).astype(np.float32)
    rgba = np.zeros((n, 4), np.float32)
    rgba[:, 3] = 1
    with np.errstate(all="ignore"):
        rgba[hit, 0] = (F(1) * dd + amb)[hit]
        rgba[hit, 1] = (F(0.8) * dd + amb)[hit]
        rgba[hit, 2] = (F(0.6) * dd + amb)[hit]
    vis = np.where(hit, occ + 256 * blocked, -1).astype(np.int32)
    return rgba, vis


def tri_lit_frame(T: q.Tree32, tris, off, voxel, pos, rd, W, H, table, **kw):
    """tri_lit32 over a whole W x H frame (rd: the (H W, 3) pixel rays, row-major): ((H, W, 4), (H, W))."""
    yy, xx = np.mgrid[0:H, 0:W]
    rgba, vis = tri_lit32(T, tris, off, voxel, pos, rd, xx.ravel(), yy.ravel(), table, **kw)
    return rgba.reshape(H, W, 4), vis.reshape(H, W)


def shadow_verdicts(T: q.Tree32, tris, off, voxel, o, d, first=None):
    """For the identity with rto_render_triangles(shadow = 1) under the renders' light: per pixel (casts, FIRST verdict, ANY verdict)
    of its shadow ray; the render uses FIRST (its walk, with the 512-pop cap), the lit render ANY."""
    tris = np.asarray(tris, np.float32).reshape(-1, 12)
    d = np.asarray(d, np.float32).reshape(-1, 3)
    hits = tq.query_tri32(T, tris, off, o, d)[tq.FIRST] if first is None else first
    so, sd = tq.shadow_rays(o, d, hits, tris, voxel)
    h = np.nonzero(hits["tri"] >= 0)[0]
    r = tq.query_tri32(T, tris, off, so[h], sd[h])
    f = np.zeros(len(d), bool); a = np.zeros(len(d), bool)
    f[h] = r[tq.FIRST]["tri"] >= 0
    a[h] = r[tq.ANY]["tri"] >= 0
    return hits["tri"] >= 0, f, a
