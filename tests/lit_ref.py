"""The lit render (include/rto_hip.h, rto_render_lit_*) restated in numpy float32 for the tests, on top of
query_ref: the primary hit is query32's FIRST record on the frame's pixel ray, the shadow and AO rays are query32's ANY rule, and
the Lambert term is shade32's arithmetic with the caller's light.  Every operation is one float32 operation in the kernels' order.

    a = face >> 1, sigma = +1 if face & 1 else -1; p = o + d tHit; eps = voxelSize 1e-3 + 2^-18 max|p|;
    so = p with so[a] = (leaf max plane + eps if sigma > 0 else leaf min plane - eps)
    shadow (shadow, face >= 0, ndotl > 0): ANY from so along lightNeg, (0, 1e30); S = 0 on a hit
    AO (K > 0, face >= 0): K ANY rays from so, (0, radius]; A = (K - occ) / K
    colour: d = S ? ndotl : 0, amb = 0.1 A, (d + amb, 0.8 d + amb, 0.6 d + amb, 1); a miss is (0, 0, 0, 1)
    vis: -1 for a miss, else occ + 256 (shadow ray cast and blocked)"""
from __future__ import annotations

import math

import numpy as np

import query_ref as q

F = np.float32
U = np.uint32
AO_MAX = 64


def bitrev6(i: int) -> int:
    return int(format(i, "06b")[::-1], 2)


def ao_table64() -> np.ndarray:
    """The AO directions by the formula, in float64 (64, 3): u = (i + 0.5) / 64, phi = 2 pi (bitrev6(i) + 0.5) / 64,
    (sqrt(u) cos phi, sqrt(u) sin phi, sqrt(1 - u))."""
    out = np.zeros((AO_MAX, 3))
    for i in range(AO_MAX):
        u = (i + 0.5) / 64
        ph = 2 * math.pi * (bitrev6(i) + 0.5) / 64
        out[i] = (math.sqrt(u) * math.cos(ph), math.sqrt(u) * math.sin(ph), math.sqrt(1 - u))
    return out


def light_neg(light_dir) -> np.ndarray:
    """-normalize(light_dir) in the host's order: dot = (x x + y y) + z z, inv = 1 / sqrt(dot), l = v inv."""
    v = np.asarray(light_dir, np.float32).reshape(3)
    dot = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    inv = F(1) / np.sqrt(F(dot))
    return (-(v * inv)).astype(np.float32)


def mix32(v):
    v = np.asarray(v, U)
    v = v ^ (v >> U(16))
    v = (v * U(0x7FEB352D)).astype(U)
    v = v ^ (v >> U(15))
    v = (v * U(0x846CA68B)).astype(U)
    return v ^ (v >> U(16))


def pixel_hash(x, y, seed) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = np.asarray(x).astype(U)
        y = np.asarray(y).astype(U)
        return mix32((x * U(0x8DA6B343)) ^ (y * U(0xD8163841)) ^ (U(int(seed) & 0xFFFFFFFF) * U(0xCB1AB31F)))


def ndotl32(T: q.Tree32, o, d, hits, lneg) -> np.ndarray:
    """shade_term for every record (0 for a miss): the centre pseudo-normal of shade32, dotted with lneg."""
    d = np.asarray(d, np.float32).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(o, np.float32).reshape(-1, 3), d.shape)
    out = np.zeros(len(d), np.float32)
    h = np.nonzero(hits["node"] >= 0)[0]
    leaf = hits["node"][h]
    c = (F(0.5) * (T.bmin[leaf] + T.bmax[leaf])).astype(np.float32)
    t = hits["t"][h].astype(np.float32)
    p = (o[h] + d[h] * t[:, None]).astype(np.float32)
    qv = (p - c).astype(np.float32)
    dot = lambda a, b: ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]).astype(np.float32) + a[..., 2] * b[..., 2]).astype(np.float32)
    inv = (F(1) / np.sqrt(dot(qv, qv))).astype(np.float32)
    nv = (qv * inv[:, None]).astype(np.float32)
    out[h] = q.gmax(F(0), dot(nv, np.asarray(lneg, np.float32)[None, :]))
    return out


def secondary_origins(T: q.Tree32, o, d, hits, voxel) -> np.ndarray:
    """so for every record with face >= 0 (rows of the others are undefined)."""
    d = np.asarray(d, np.float32).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(o, np.float32).reshape(-1, 3), d.shape)
    t = hits["t"].astype(np.float32)
    p = (o + (d * t[:, None]).astype(np.float32)).astype(np.float32)
    ap = np.abs(p)
    hm = q.gmax(q.gmax(ap[:, 0], ap[:, 1]), ap[:, 2]).astype(np.float32)
    eps = (F(voxel) * F(1e-3) + hm * F(2.0 ** -18)).astype(np.float32)
    face = hits["face"]
    ok = face >= 0
    a = np.where(ok, face >> 1, 0)
    up = (face & 1) == 1
    node = np.where(ok, hits["node"], 0)
    rows = np.arange(len(d))
    plane = np.where(up, (T.bmax[node, a] + eps).astype(np.float32), (T.bmin[node, a] - eps).astype(np.float32))
    so = p.copy()
    so[rows, a] = np.where(ok, plane, p[rows, a])
    return so


def ao_dirs(table, h, face, K) -> np.ndarray:
    """(n, K, 3) AO directions of n hits with hashes h and entry faces face."""
    table = np.asarray(table, np.float32).reshape(AO_MAX, 3)
    s = np.arange(K, dtype=np.int64)
    e = ((h.astype(np.int64)[:, None] + (64 * s)[None, :] // K) & 63)
    t = table[e]                                                    # (n, K, 3)
    a = (face >> 1)[:, None]
    u = np.where(((h >> U(6)) & U(1)).astype(bool)[:, None], -t[..., 0], t[..., 0])
    v = np.where(((h >> U(7)) & U(1)).astype(bool)[:, None], -t[..., 1], t[..., 1])
    n = np.where(((face & 1) == 1)[:, None], t[..., 2], -t[..., 2])
    out = np.empty(t.shape, np.float32)
    out[..., 0] = np.where(a == 0, n, np.where(a == 1, v, u))
    out[..., 1] = np.where(a == 0, u, np.where(a == 1, n, v))
    out[..., 2] = np.where(a == 0, v, np.where(a == 1, u, n))
    return out


def lit32(T: q.Tree32, voxel, o, d, x, y, table, light_dir=(-1.0, -1.0, -1.0), shadow=True, K=0, radius=1.0, seed=0,
          rays_out=None):
    """The lit pixels (x, y) whose pixel rays are (o, d): (rgba (n, 4) float32, vis (n,) int32).  rays_out (a dict): receives
    the secondary rays ("shadow": (origins, dirs, blocked), "ao": (origins, dirs, hit)) for the float64 comparison."""
    d = np.asarray(d, np.float32).reshape(-1, 3)
    n = len(d)
    lneg = light_neg(light_dir)
    hits = q.query32(T, o, d)[q.FIRST]
    hit = hits["node"] >= 0
    face = hits["face"]
    ndotl = ndotl32(T, o, d, hits, lneg)
    so = secondary_origins(T, o, d, hits, voxel)
    S = np.ones(n, bool)
    occ = np.zeros(n, np.int64)
    cast = bool(shadow) & (face >= 0) & (ndotl > 0)
    blocked = np.zeros(n, bool)
    if cast.any():
        ci = np.nonzero(cast)[0]
        sd = np.broadcast_to(lneg, (len(ci), 3)).copy()
        sh = q.query32(T, so[ci], sd)[q.ANY]["node"] >= 0
        blocked[ci] = sh
        S = ~blocked
        if rays_out is not None:
            rays_out["shadow"] = (so[ci], sd, sh)
    if K > 0:
        ai = np.nonzero(face >= 0)[0]
        if len(ai):
            h = pixel_hash(np.asarray(x)[ai], np.asarray(y)[ai], seed)
            dirs = ao_dirs(table, h, face[ai], K).reshape(-1, 3)
            orig = np.repeat(so[ai], K, axis=0)
            ah = q.query32(T, orig, dirs, 0.0, F(radius))[q.ANY]["node"] >= 0
            occ[ai] = ah.reshape(len(ai), K).sum(1)
            if rays_out is not None:
                rays_out["ao"] = (orig, dirs, ah)
    A = np.ones(n, np.float32)
    if K > 0:
        A = ((K - occ).astype(np.float32) / F(K)).astype(np.float32)
    dd = np.where(S, ndotl, F(0)).astype(np.float32)
    amb = (F(0.1) * A).astype(np.float32)
    rgba = np.zeros((n, 4), np.float32)
    rgba[:, 3] = 1
    rgba[hit, 0] = (F(1) * dd + amb)[hit]
    rgba[hit, 1] = (F(0.8) * dd + amb)[hit]
    rgba[hit, 2] = (F(0.6) * dd + amb)[hit]
    vis = np.where(hit, occ + 256 * blocked, -1).astype(np.int32)
    return rgba, vis


def lit_frame(T: q.Tree32, voxel, pos, rd, W, H, table, **kw):
    """lit32 over a whole W x H frame (rd: the (H W, 3) pixel rays, row-major): ((H, W, 4), (H, W))."""
    yy, xx = np.mgrid[0:H, 0:W]
    rgba, vis = lit32(T, voxel, pos, rd, xx.ravel(), yy.ravel(), table, **kw)
    return rgba.reshape(H, W, 4), vis.reshape(H, W)
