"""Triangle queries (include/rto_hip.h, rto_query_triangles_*) restated for the tests in float32 numpy, written from the rule, not
from the kernels.

A leaf is reachable when its box and every ancestor's pass the oracle's slab test with tNear < 1e30 (query_ref.Tree32.slab: the
triangle render's box rule; boxes see no window).  A triangle of a reachable leaf is accepted when Moeller-Trumbore in the
operation order of the renders' ray_triangle (oracle/rto_oracle.c, one float32 operation per source operator: the builds use
-ffp-contract=off) reports a hit, t > 0, and t_min <= t <= min(t_max, largest float below 1e30).
  FIRST    the first leaf in the reference's LIFO pop order (query_ref's rank) with an accepted triangle, unless more than 512
           nodes are popped up to it; in it the least t, ties to the lowest triangle index;
  CLOSEST  least t over every accepted triangle, ties to the lowest index;
  ANY      CLOSEST's hit mask (which triangle is unspecified; the records here are CLOSEST's).
Also: the records' shading (orc_render_triangles' Lambert term and colour) and the shadow ray the render derives from a hit."""
from __future__ import annotations

import numpy as np

import query_ref as q

F = np.float32
FIRST, CLOSEST, ANY = q.FIRST, q.CLOSEST, q.ANY
MISS_T = q.MISS_T
MAX_POPS = q.MAX_POPS
TRI_HIT_DTYPE = np.dtype([("t", "<f4"), ("tri", "<i4"), ("node", "<i4"), ("u", "<f4"), ("v", "<f4"),
                          ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")])
# the light of the renders: -normalize(vec3(-1)), normalize = v * (1 / sqrt(dot(v, v)))
_S = F(1) / np.sqrt(F(3))
LIGHT = np.array([-(F(-1) * _S)] * 3, np.float32)


def _dot(a, b):
    """(x + y) + z of the products, float32 (v3_dot and the kernels' spelled-out sums)."""
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(np.float32)


def _cross(a, b):
    """glm cross: (a.y b.z - b.y a.z, a.z b.x - b.z a.x, a.x b.y - b.x a.y)."""
    return np.stack([a[:, 1] * b[:, 2] - b[:, 1] * a[:, 2], a[:, 2] * b[:, 0] - b[:, 2] * a[:, 0],
                     a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]], 1).astype(np.float32)


def ray_triangle(o, d, tris):
    """Moeller-Trumbore over (ray, triangle) pairs: o, d (m, 3) float32, tris (m, 12) float32 -> (hit, t, u, v)."""
    v0, v1, v2 = tris[:, 0:3], tris[:, 3:6], tris[:, 6:9]
    with np.errstate(all="ignore"):
        e1, e2 = (v1 - v0).astype(np.float32), (v2 - v0).astype(np.float32)
        p = _cross(d, e2)
        det = _dot(e1, p)
        ok = ~(np.abs(det) < F(1e-12))
        inv = (F(1) / det).astype(np.float32)
        tv = (o - v0).astype(np.float32)
        u = (_dot(tv, p) * inv).astype(np.float32)
        ok &= ~((u < 0) | (u > 1))
        qq = _cross(tv, e1)
        v = (_dot(d, qq) * inv).astype(np.float32)
        ok &= ~((v < 0) | ((u + v).astype(np.float32) > 1))
        t = (_dot(e2, qq) * inv).astype(np.float32)
        ok &= t > 0
    return ok, t, u, v


def _reach(T: q.Tree32, o, inv, valid):
    """Every (ray, node) pair the LIFO walk pops (rank), and the reachable leaves among them."""
    rays = np.nonzero(valid)[0]
    nds = np.zeros(len(rays), np.int64)
    pop_r, pop_n, leaf_r, leaf_n = [], [], [], []
    while len(rays):
        pop_r.append(rays); pop_n.append(nds)
        _, _, _, ok = T.slab(o[rays], inv[rays], nds)
        lf = ok & T.leafy[nds]
        leaf_r.append(rays[lf]); leaf_n.append(nds[lf])
        go = ok & ~T.leafy[nds]
        c = T.child[nds[go]]
        has = c >= 0
        rays = np.repeat(rays[go], has.sum(1)); nds = c[has]
    cat = np.concatenate
    return cat(pop_r), cat(pop_n), cat(leaf_r), cat(leaf_n)


def query_tri32(T: q.Tree32, tris, tri_offset, o, d, t_min=0.0, t_max=1e30):
    """The three rules over rays (o, d): {FIRST, CLOSEST, ANY} -> TRI_HIT_DTYPE records."""
    tris = np.asarray(tris, np.float32).reshape(-1, 12)
    off = np.asarray(tri_offset, np.int64)
    d = np.asarray(d, np.float32).reshape(-1, 3)
    R = len(d)
    o = np.ascontiguousarray(np.broadcast_to(np.asarray(o, np.float32).reshape(-1, 3), d.shape))
    tmn, tmx, tlo, thi = q.windows(t_min, t_max, R)
    with np.errstate(all="ignore"):
        inv = (F(1) / d).astype(np.float32)
    valid = ~(np.isnan(o).any(1) | np.isnan(d).any(1)) & (tmn <= tmx)
    pr, pn, lr, ln = _reach(T, o, inv, valid)
    cnt = off[ln + 1] - off[ln]
    pi = np.repeat(np.arange(len(lr)), cnt)
    k = np.repeat(off[ln] - np.cumsum(cnt) + cnt, cnt) + np.arange(int(cnt.sum()))
    ray, leaf = lr[pi], ln[pi]
    hit, t, u, v = ray_triangle(o[ray], d[ray], tris[k])
    acc = hit & (t >= tlo[ray]) & (t <= thi[ray])
    ray, leaf, k, t, u, v = ray[acc], leaf[acc], k[acc], t[acc], u[acc], v[acc]
    NONE = np.iinfo(np.int64).max
    out = {}
    # FIRST: the first leaf in pop order with an accepted triangle, within the cap; least t in it, ties to the lowest index
    first = np.full(R, NONE)
    np.minimum.at(first, ray, T.rank[leaf])
    prank = T.rank[pn]
    pops = np.bincount(pr[prank <= first[pr]], minlength=R)
    sel = T.rank[leaf] == first[ray]
    out[FIRST] = _records(tris, R, d, ray[sel], leaf[sel], k[sel], t[sel], u[sel], v[sel], (first != NONE) & (pops <= MAX_POPS))
    out[CLOSEST] = _records(tris, R, d, ray, leaf, k, t, u, v, np.ones(R, bool))
    out[ANY] = out[CLOSEST].copy()
    return out


def _records(tris, R, d, ray, leaf, k, t, u, v, allowed):
    """Per ray the candidate of least (t, k), if `allowed`; the normal turned as the renders turn it."""
    h = miss_records(R)
    order = np.lexsort((k, t, ray))
    ray, leaf, k, t, u, v = ray[order], leaf[order], k[order], t[order], u[order], v[order]
    top = np.ones(len(ray), bool)
    top[1:] = ray[1:] != ray[:-1]
    top &= allowed[ray]
    r = ray[top]
    n = tris[k[top], 9:12].copy()
    turn = _dot(n, d[r]) > 0
    n[turn] = -n[turn]
    h["t"][r] = t[top]; h["tri"][r] = k[top]; h["node"][r] = leaf[top]; h["u"][r] = u[top]; h["v"][r] = v[top]
    h["nx"][r], h["ny"][r], h["nz"][r] = n[:, 0], n[:, 1], n[:, 2]
    return h


def miss_records(n):
    h = np.zeros(n, TRI_HIT_DTYPE)
    h["t"] = MISS_T
    h["tri"] = -1
    h["node"] = -1
    return h


def _gmax(x, y):
    return np.where(x < y, y, x)


def lambert(hits):
    """orc_render_triangles' ndotl of records: max(0, dot(n, -light)) with the record's (turned) normal; 0 for a miss."""
    n = np.stack([hits["nx"], hits["ny"], hits["nz"]], 1).astype(np.float32)
    nl = _gmax(F(0), _dot(n, np.broadcast_to(LIGHT, n.shape))).astype(np.float32)
    return np.where(hits["tri"] >= 0, nl, F(0)).astype(np.float32)


def shade(hits, shadowed=None):
    """RGBA float32 (n, 4) of orc_render_triangles from the primary records (and the shadow verdicts, if any)."""
    nl = lambert(hits)
    if shadowed is not None:
        nl = np.where(shadowed, F(0), nl).astype(np.float32)
    out = np.zeros((len(hits), 4), np.float32)
    h = hits["tri"] >= 0
    for c, w in enumerate((F(1.0), F(0.8), F(0.6))):
        out[:, c] = np.where(h, (w * nl).astype(np.float32) + F(0.1), F(0))
    out[:, 3] = F(1)
    return out


def shadow_rays(o, d, hits, tris, voxel_size):
    """The shadow ray orc_render_triangles traces from each hit: p = o + d t put back on the triangle's plane and offset along the
    turned normal by max-norm-relative bias; direction -light.  Returns (origins, directions) float32 (n, 3); rows of misses are
    meaningless."""
    tris = np.asarray(tris, np.float32).reshape(-1, 12)
    d = np.asarray(d, np.float32).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(o, np.float32).reshape(-1, 3), d.shape)
    t = hits["t"].astype(np.float32)
    n = np.stack([hits["nx"], hits["ny"], hits["nz"]], 1).astype(np.float32)
    with np.errstate(all="ignore"):
        p = (o + (d * t[:, None]).astype(np.float32)).astype(np.float32)
        v0 = tris[np.maximum(hits["tri"], 0), 0:3]
        bias = (F(voxel_size) * F(1e-3)).astype(np.float32)
        pm = _gmax(_gmax(np.abs(p[:, 0]), np.abs(p[:, 1])), np.abs(p[:, 2])).astype(np.float32)
        hh = ((bias + (pm * F(2.0 ** -18)).astype(np.float32)).astype(np.float32) - _dot((p - v0).astype(np.float32), n)).astype(np.float32)
        so = (p + (n * hh[:, None]).astype(np.float32)).astype(np.float32)
    return so, np.broadcast_to(LIGHT, so.shape).copy()
