"""Ray queries (include/rto_hip.h, rto_query_*) restated for the tests: a float32 numpy statement of the acceptance rule, and a
float64 statement with robust flags.

float32 (`query32`), written from the rule, not from the kernels: for a ray (o, d, t_min, t_max), t_lo = max(t_min, 0) and
t_hi = min(t_max, largest float below 1e30).  The slab test is the oracle's (oracle/rto_oracle.c intersect_aabb: invDir = 1 / d,
t1 = (bmin - o) * invDir, t2 = (bmax - o) * invDir, glm's min(x, y) = (y < x) ? y : x and max(x, y) = (x < y) ? y : x, tNear =
max(max(x, y), z), tFar = min(min(x, y), z), passes when tNear <= tFar and tFar > 0), on the node box of the oracle's walk
(bmin = gridMin + float(x) * voxel, bmax = bmin + float(size) * voxel), with tNear < 1e30 as the renders' closestT prune.  Every
operation is one float32 operation.  A solid leaf is accepted when it and all its ancestors pass and tHit = max(t_lo, tNear)
satisfies tHit <= tFar and tHit <= t_hi.  FIRST: the accepted leaf popped first by the reference's LIFO walk (children 7 .. 0),
unless more than 512 nodes are popped up to it; CLOSEST: least tHit, ties to the leaf popped first; ANY: CLOSEST's hit mask.
The walk is brute force over the (ray, node) pairs it reaches; nothing is pruned by t.

float64 (`Octree64Q`, a subclass of ref64.Octree64): the same rule on the float64 boxes, with first-order error bounds of the
float32 decisions; a ray is robust when none of the decisions its answer depends on lies within its bound."""
from __future__ import annotations

import numpy as np

import ref64

F = np.float32
BELOW_1E30 = np.frombuffer(np.uint32(0x7149F2C9).tobytes(), np.float32)[0]
MISS_T = F(1e30)
MAX_POPS = 512
FIRST, CLOSEST, ANY = 0, 1, 2
HIT_DTYPE = np.dtype([("t", "<f4"), ("node", "<i4"), ("face", "<i4"), ("size", "<i4"),
                      ("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("reserved", "<i4")])


def gmin(x, y):
    return np.where(y < x, y, x)


def gmax(x, y):
    return np.where(x < y, y, x)


class Tree32:
    """Node boxes in float32 with the oracle's arithmetic, the child table and the LIFO pop rank of every node."""

    def __init__(self, nodes, grid_min, voxel_size):
        self.nodes = nodes
        n = len(nodes)
        vs = F(voxel_size)
        g = np.asarray(grid_min, np.float32).reshape(3)
        xyz = np.stack([nodes["x"], nodes["y"], nodes["z"]], 1)
        self.bmin = (g[None, :] + xyz.astype(np.float32) * vs).astype(np.float32)
        ext = (nodes["size"].astype(np.float32) * vs).astype(np.float32)
        self.bmax = (self.bmin + ext[:, None]).astype(np.float32)
        self.leafy = (nodes["isLeaf"] == 1) | (nodes["isUniform"] == 1)
        self.solid = self.leafy & (nodes["isSolid"] == 1)
        self.child = np.where(self.leafy[:, None], -1, np.asarray(nodes["child"], np.int64).reshape(n, 8))
        self.rank = ref64.Octree64(nodes, grid_min, voxel_size).rank

    def slab(self, o, inv, nd):
        """(tNear, tFar, per-axis entry parameters, passes) of (ray, node) pairs, float32."""
        with np.errstate(all="ignore"):
            t1 = (self.bmin[nd] - o) * inv
            t2 = (self.bmax[nd] - o) * inv
            tmin, tmax = gmin(t1, t2), gmax(t1, t2)
            tn = gmax(gmax(tmin[:, 0], tmin[:, 1]), tmin[:, 2])
            tf = gmin(gmin(tmax[:, 0], tmax[:, 1]), tmax[:, 2])
            ok = (tn <= tf) & (tf > 0) & ~(tn >= F(1e30))
        return tn, tf, tmin, ok


def windows(t_min, t_max, n):
    tmn = np.broadcast_to(np.asarray(t_min, np.float32), n).astype(np.float32)
    tmx = np.broadcast_to(np.asarray(t_max, np.float32), n).astype(np.float32)
    tlo = np.where(tmn > 0, tmn, F(0)).astype(np.float32)
    thi = gmin(tmx, BELOW_1E30).astype(np.float32)
    return tmn, tmx, tlo, thi


def query32(T: Tree32, o, d, t_min=0.0, t_max=1e30):
    """The three rules over rays (o, d) (float32 (n, 3) arrays): {FIRST, CLOSEST, ANY} -> HIT_DTYPE records.  ANY's leaf is
    CLOSEST's (the rule leaves it open; compare masks only)."""
    o = np.asarray(o, np.float32).reshape(-1, 3)
    d = np.asarray(d, np.float32).reshape(-1, 3)
    R = len(d)
    o = np.broadcast_to(o, d.shape)
    tmn, tmx, tlo, thi = windows(t_min, t_max, R)
    with np.errstate(all="ignore"):
        inv = (F(1) / d).astype(np.float32)
    valid = ~(np.isnan(o).any(1) | np.isnan(d).any(1)) & (tmn <= tmx)
    # the walk: every child of a passing internal node is popped
    rays = np.nonzero(valid)[0]
    nds = np.zeros(len(rays), np.int64)
    pop_r, pop_rank = [], []
    acc_r, acc_n, acc_t, acc_face = [], [], [], []
    while len(rays):
        pop_r.append(rays); pop_rank.append(T.rank[nds])
        tn, tf, tmin, ok = T.slab(o[rays], inv[rays], nds)
        sol = ok & T.solid[nds]
        th = gmax(tlo[rays], tn)
        acc = sol & (th <= tf) & (th <= thi[rays])
        a = np.nonzero(acc)[0]
        face = np.full(len(a), -1, np.int64)
        for ax in (2, 1, 0):                                   # the lowest axis whose entry parameter is tNear wins
            face = np.where(tmin[a, ax] == tn[a], 2 * ax + (d[rays[a], ax] < 0), face)
        face = np.where(th[a] > tn[a], -1, face)
        acc_r.append(rays[a]); acc_n.append(nds[a]); acc_t.append(th[a]); acc_face.append(face)
        go = ok & ~T.leafy[nds]
        c = T.child[nds[go]]
        has = c >= 0
        rays = np.repeat(rays[go], has.sum(1)); nds = c[has]
    cat = np.concatenate
    pr, prank = cat(pop_r), cat(pop_rank)
    ar, an, at, af = cat(acc_r), cat(acc_n), cat(acc_t).astype(np.float32), cat(acc_face)
    NONE = np.iinfo(np.int64).max
    out = {}
    # FIRST
    first = np.full(R, NONE)
    np.minimum.at(first, ar, T.rank[an])
    pops = np.bincount(pr[prank <= first[pr]], minlength=R)
    fhit = (first != NONE) & (pops <= MAX_POPS)
    sel = np.nonzero(T.rank[an] == first[ar])[0]
    out[FIRST] = _records(T, R, ar[sel], an[sel], at[sel], af[sel], fhit)
    # CLOSEST
    best = np.full(R, np.inf, np.float32)
    np.minimum.at(best, ar, at)
    win = at == best[ar]
    wrank = np.full(R, NONE)
    np.minimum.at(wrank, ar[win], T.rank[an[win]])
    sel = np.nonzero(win & (T.rank[an] == wrank[ar]))[0]
    chit = wrank != NONE
    out[CLOSEST] = _records(T, R, ar[sel], an[sel], at[sel], af[sel], chit)
    out[ANY] = out[CLOSEST].copy()
    return out


def _records(T, R, r, n, t, face, hit):
    h = np.zeros(R, HIT_DTYPE)
    h["t"] = MISS_T
    h["node"] = -1
    h["face"] = -1
    keep = hit[r]
    r, n, t, face = r[keep], n[keep], t[keep], face[keep]
    h["t"][r] = t
    h["node"][r] = n
    h["face"][r] = face
    for f in ("size", "x", "y", "z"):
        h[f][r] = T.nodes[f][n]
    return h


def shade32(T: Tree32, o, d, hits):
    """The oracle's shade_store for records (leaf, t): centre = 0.5 (bmin + bmax), p = o + d t, n = normalize(p - centre),
    ndotl = max(0, dot(n, -normalize(-1, -1, -1))), RGBA = (ndotl + .1, .8 ndotl + .1, .6 ndotl + .1, 1); misses (0, 0, 0, 1)."""
    o = np.broadcast_to(np.asarray(o, np.float32).reshape(-1, 3), np.asarray(d).reshape(-1, 3).shape)
    d = np.asarray(d, np.float32).reshape(-1, 3)
    out = np.zeros((len(d), 4), np.float32)
    out[:, 3] = 1
    h = np.nonzero(hits["node"] >= 0)[0]
    leaf = hits["node"][h]
    c = (F(0.5) * (T.bmin[leaf] + T.bmax[leaf])).astype(np.float32)
    t = hits["t"][h].astype(np.float32)
    p = (o[h] + d[h] * t[:, None]).astype(np.float32)
    q = (p - c).astype(np.float32)
    dot = lambda a, b: ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]).astype(np.float32) + a[..., 2] * b[..., 2]).astype(np.float32)
    inv = (F(1) / np.sqrt(dot(q, q))).astype(np.float32)
    nv = (q * inv[:, None]).astype(np.float32)
    lv = np.full(3, F(-1), np.float32)
    li = F(1) / np.sqrt(dot(lv, lv))
    nl = -(lv * li).astype(np.float32)
    nd = gmax(F(0), dot(nv, nl[None, :])).astype(np.float32)
    out[h, 0] = F(1) * nd + F(0.1)
    out[h, 1] = F(0.8) * nd + F(0.1)
    out[h, 2] = F(0.6) * nd + F(0.1)
    return out


class Octree64Q(ref64.Octree64):
    """Octree64 with [t_min, t_max] windows: the three rules in float64 and per ray a robust flag (no decision within the
    float32 error bound of its threshold: slab tests on the path, tHit <= tFar, tNear <= t_hi, the CLOSEST winner's margin, the
    pops up to the FIRST leaf).  t_lo = max(t_min, 0) and t_hi = min(t_max, largest float below 1e30) as in float32."""

    def _slab(self, o, d, nodes):
        """Octree64's slab test, and one more borderline case that arbitrary rays reach: a direction with a zero component and an
        origin within float32's error of one of the box's planes on that axis (the float32 plane may lie on the other side)."""
        passes, amb = super()._slab(o, d, nodes)
        near = (np.abs(o - self.bmin[nodes]) <= ref64.K * ref64.EPS * (self.bmag[nodes][:, None] + np.abs(o))) | \
               (np.abs(o - self.bmax[nodes]) <= ref64.K * ref64.EPS * (self.bmag[nodes][:, None] + np.abs(o)))
        return passes, amb | ((d == 0.0) & near).any(1)

    def trace_windows(self, o, d, t_min=0.0, t_max=1e30):
        o = np.asarray(o, np.float64).reshape(-1, 3)
        d = np.asarray(d, np.float64).reshape(-1, 3)
        R = len(d)
        tmn, tmx, tlo, thi = windows(t_min, t_max, R)
        valid = ~(np.isnan(o).any(1) | np.isnan(d).any(1)) & (tmn <= tmx)
        tlo, thi = tlo.astype(np.float64), thi.astype(np.float64)
        (lr, ln, lnom, lamb), (pr, prank, pamb, _) = self._walk(o, d, R)
        sol = self.solid[ln]
        lr, ln, lnom, lamb = lr[sol], ln[sol], lnom[sol], lamb[sol]
        tn, tf, en, ef = self._slab_terms(o[lr], d[lr], ln)
        with np.errstate(invalid="ignore"):
            th = np.maximum(tlo[lr], tn)
            terr = np.where(tn > tlo[lr] - en, en, 0.0)                  # tHit is tNear's float, or t_lo's exactly
            acc = lnom & (th <= tf) & (th <= thi[lr])
            amb = lamb | (np.abs(th - tf) <= terr + ef) | (np.abs(tn - thi[lr]) <= en) | np.isnan(th)
        NONE = np.iinfo(np.int64).max
        node_of = np.zeros(self.n, np.int64)
        node_of[self.rank[::-1]] = np.arange(self.n)[::-1]
        # CLOSEST
        best = np.full(R, np.inf)
        np.minimum.at(best, lr[acc], th[acc])
        win = acc & (th == best[lr])
        wrank = np.full(R, NONE)
        np.minimum.at(wrank, lr[win], self.rank[ln[win]])
        chit = wrank != NONE
        is_w = win & (self.rank[ln] == wrank[lr])
        werr = np.zeros(R)
        werr[lr[is_w]] = terr[is_w]
        with np.errstate(invalid="ignore"):
            rival = ~is_w & (acc | amb) & ((th <= best[lr] + werr[lr] + terr) | np.isnan(th))
        crob = np.ones(R, bool)
        crob[lr[rival | (is_w & amb)]] = False
        closest = dict(hit=chit, leaf=np.where(chit, node_of[np.where(chit, wrank, 0)], -1), robust=crob,
                       t=np.where(chit, best, np.inf))
        # ANY: a hit when some leaf is accepted beyond doubt; a miss when no leaf is even borderline
        sure = np.zeros(R, bool)
        sure[lr[acc & ~amb]] = True
        anyamb = np.zeros(R, bool)
        anyamb[lr[amb]] = True
        anyr = dict(hit=chit, robust=np.where(chit, sure, ~anyamb))
        # FIRST: pops counted over the nominal walk up to the first accepted leaf
        first = np.full(R, NONE)
        np.minimum.at(first, lr[acc], self.rank[ln[acc]])
        upto = prank <= first[pr]
        pops = np.bincount(pr[upto], minlength=R)
        nab = np.bincount(pr[upto & pamb], minlength=R)
        fhit = (first != NONE) & (pops <= ref64.MAX_POPS)
        frob = nab == 0
        early = np.zeros(R, bool)
        early[lr[amb & (self.rank[ln] <= first[lr])]] = True
        frob &= ~early
        firstd = dict(hit=fhit, leaf=np.where(fhit, node_of[np.where(fhit, first, 0)], -1), robust=frob)
        out = {FIRST: firstd, CLOSEST: closest, ANY: anyr}
        for rule in out.values():                                     # NaN input or t_min > t_max: a miss, for certain
            rule["hit"] = rule["hit"] & valid
            rule["robust"] = rule["robust"] | ~valid
            if "leaf" in rule:
                rule["leaf"] = np.where(valid, rule["leaf"], -1)
        return out


def seeded_rays(T: Tree32, n, seed, windows_too=True):
    """Rays of every kind the tests need, over the root box of T: origins outside, inside the volume and inside solid leaves,
    axis-aligned rays and rays with zero components, grazing rays along leaf faces, t_max windows that end before the nearest
    hit, t_min windows that start past it, NaN rays and t_min > t_max.  Returns (o, d, t_min, t_max) float32 arrays."""
    rng = np.random.default_rng(seed)
    lo, hi = T.bmin[0].astype(np.float64), T.bmax[0].astype(np.float64)
    ext = hi - lo
    centre = 0.5 * (lo + hi)
    k = n // 8
    o = np.empty((n, 3)); d = np.empty((n, 3))
    # 0: outside, on a sphere around the root box, aimed into it
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    o[:] = centre + u * ext.max() * rng.uniform(0.9, 2.0, (n, 1))
    tgt = lo + rng.random((n, 3)) * ext
    d[:] = tgt - o
    # 1: inside the volume, any direction
    s = slice(k, 2 * k)
    o[s] = lo + rng.random((k, 3)) * ext
    d[s] = rng.normal(size=(k, 3))
    # 2: inside solid leaves
    s = slice(2 * k, 3 * k)
    sl = np.nonzero(T.solid)[0]
    if len(sl):
        pick = sl[rng.integers(0, len(sl), k)]
        o[s] = T.bmin[pick] + rng.random((k, 3)) * (T.bmax[pick] - T.bmin[pick])
    d[s] = rng.normal(size=(k, 3))
    # 3: axis-aligned, from outside and inside
    s = slice(3 * k, 4 * k)
    ax = rng.integers(0, 3, k)
    d[s] = 0.0
    d[np.arange(3 * k, 4 * k), ax] = rng.choice([-1.0, 1.0], k) * rng.uniform(0.5, 3.0, k)
    o[s] = lo + rng.uniform(-0.2, 1.2, (k, 3)) * ext
    # 4: one zero component
    s = slice(4 * k, 5 * k)
    d[np.arange(4 * k, 5 * k), rng.integers(0, 3, k)] = 0.0
    # 5: grazing: origin on a leaf face plane, direction inside that plane (or nearly)
    s = slice(5 * k, 6 * k)
    if len(sl):
        pick = sl[rng.integers(0, len(sl), k)]
        ax = rng.integers(0, 3, k)
        p = T.bmin[pick].astype(np.float64) + rng.random((k, 3)) * (T.bmax[pick] - T.bmin[pick])
        p[np.arange(k), ax] = T.bmin[pick][np.arange(k), ax]
        dd = rng.normal(size=(k, 3))
        dd[np.arange(k), ax] = rng.choice([0.0, 1e-7], k)
        o[s] = p - dd * ext.max()
        d[s] = dd
    o = o.astype(np.float32); d = d.astype(np.float32)
    t_min = np.zeros(n, np.float32); t_max = np.full(n, 1e30, np.float32)
    if windows_too:
        T0 = query32(T, o, d)[CLOSEST]
        hitt = np.where(T0["node"] >= 0, T0["t"], np.float32(1.0)).astype(np.float32)
        w = rng.integers(0, 4, n)
        # 1: t_max cuts the nearest hit; 2: t_min skips past it; 3: a window around it
        t_max = np.where(w == 1, hitt * rng.uniform(0.3, 0.999, n).astype(np.float32), t_max).astype(np.float32)
        t_min = np.where(w == 2, hitt * rng.uniform(1.001, 1.5, n).astype(np.float32), t_min).astype(np.float32)
        t_min = np.where(w == 3, hitt * np.float32(0.9), t_min).astype(np.float32)
        t_max = np.where(w == 3, hitt * np.float32(1.2), t_max).astype(np.float32)
        t_min[rng.random(n) < 0.03] = np.float32(-1.0)
    # invalid rays at the end: a NaN in each field, t_min > t_max; then the degenerate window t_min == t_max (valid)
    if n >= 16:
        o[n - 7, 0] = np.nan
        o[n - 6, 2] = np.nan
        d[n - 5, 1] = np.nan
        t_min[n - 4] = np.nan
        t_max[n - 3] = np.nan
        t_min[n - 2], t_max[n - 2] = 2.0, 1.0
        t_min[n - 1] = t_max[n - 1] = 0.5
    return o, d, t_min, t_max
