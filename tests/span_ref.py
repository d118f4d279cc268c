"""Span queries (include/rto_hip.h, rto_query_spans_*) restated for the tests: a float32 numpy statement of the rule, bit for bit,
and a float64 statement of `length` with a per-ray error bound.

float32 (`span32`), written from the rule, not from the kernels.  Window and acceptance are query_ref.query32's: t_lo = max(t_min,
0), t_hi = min(t_max, largest float below 1e30); a solid leaf is accepted when its box and every ancestor's pass the float32 slab
test with tNear < 1e30 and tIn = max(t_lo, tNear) satisfies tIn <= tFar and tIn <= t_hi.  Its contribution is tOut - tIn with tOut
= min(tFar, t_hi) (glm's min), one float32 subtraction.  The walk is brute force over the (ray, node) pairs it reaches, nothing is
cut by t.  The accepted leaves of a ray are then sorted by the visit key -- the digits slot ^ flip of the path from the root, 3
bits per level, most significant first (flip = (d.x < 0) | (d.y < 0) << 1 | (d.z < 0) << 2; the slot is the column of the child
table, whatever box sits in it) -- and `length` is a sequential float32 np.add in that order from 0.0.  t_enter = least tIn, t_exit
= greatest tOut, leaves = the count, (node, face) = the leaf of least tIn, ties to the leaf the reference's LIFO order pops first
as pops_before states it, by the leaves' positions: at the highest bit in which two positions differ the greater octant digit
x | y << 1 | z << 2 wins, which is the greater Morton code; leaves at one position (no octree has them) go by visit order.  On an
array whose child slots are the octants of the children's boxes this is the LIFO pop order itself, and CLOSEST's tie rule.

float64 (`Octree64S`, a subclass of query_ref.Octree64Q): the same sum over the float64 boxes, and per ray a bound of what the
float32 record's length may differ from it (see `span_windows`)."""
from __future__ import annotations

import numpy as np

import query_ref as q
import ref64

F = np.float32
SPAN_DTYPE = np.dtype([("length", "<f4"), ("t_enter", "<f4"), ("t_exit", "<f4"), ("leaves", "<i4"),
                       ("node", "<i4"), ("face", "<i4"), ("reserved", "<i4", (2,))])
MAX_LEVELS = 20                 # 3 bits per level: 60 bits of an int64


def miss_records(n):
    s = np.zeros(n, SPAN_DTYPE)
    s["t_enter"] = q.MISS_T
    s["t_exit"] = q.MISS_T
    s["node"] = -1
    s["face"] = -1
    return s


def _morton(nodes, idx):
    """Octant digits x | y << 1 | z << 2 of the nodes' positions, 3 bits per coordinate bit, most significant first."""
    x, y, z = (nodes[f][idx].astype(np.int64) for f in ("x", "y", "z"))
    m = np.zeros(len(idx), np.int64)
    for b in range(20, -1, -1):
        m = (m << 3) | ((x >> b) & 1) | (((y >> b) & 1) << 1) | (((z >> b) & 1) << 2)
    return m


def span32(T: q.Tree32, o, d, t_min=0.0, t_max=1e30, ties=False):
    """SPAN_DTYPE records of rays (o, d) (float32 (n, 3) arrays, or one origin) with scalar or per-ray windows.  ties=True: also
    the mask of rays on which more than one accepted leaf has the least tIn."""
    d = np.asarray(d, np.float32).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(o, np.float32).reshape(-1, 3), d.shape)
    R = len(d)
    tmn, tmx, tlo, thi = q.windows(t_min, t_max, R)
    with np.errstate(all="ignore"):
        inv = (F(1) / d).astype(np.float32)
    valid = ~(np.isnan(o).any(1) | np.isnan(d).any(1)) & (tmn <= tmx)
    flip = ((d[:, 0] < 0).astype(np.int64) | ((d[:, 1] < 0).astype(np.int64) << 1) | ((d[:, 2] < 0).astype(np.int64) << 2))
    rays = np.nonzero(valid)[0]
    nds = np.zeros(len(rays), np.int64)
    keys = np.zeros(len(rays), np.int64)
    level = 0
    acc = [[] for _ in range(6)]                                   # ray, node, key, tIn, tOut, face
    while len(rays):
        assert level <= MAX_LEVELS
        tn, tf, tmin, ok = T.slab(o[rays], inv[rays], nds)
        tin = q.gmax(tlo[rays], tn)
        a = np.nonzero(ok & T.solid[nds] & (tin <= tf) & (tin <= thi[rays]))[0]
        face = np.full(len(a), -1, np.int64)
        for ax in (2, 1, 0):                                       # the lowest axis whose entry parameter is tNear wins
            face = np.where(tmin[a, ax] == tn[a], 2 * ax + (d[rays[a], ax] < 0), face)
        face = np.where(tin[a] > tn[a], -1, face)
        tout = q.gmin(tf[a], thi[rays[a]])
        for lst, v in zip(acc, (rays[a], nds[a], keys[a] << (3 * (MAX_LEVELS - level)), tin[a], tout, face)):
            lst.append(v)
        go = ok & ~T.leafy[nds]
        c = T.child[nds[go]]
        has = c >= 0
        cnt = has.sum(1)
        slot = np.broadcast_to(np.arange(8), c.shape)[has]
        rays = np.repeat(rays[go], cnt)
        keys = (np.repeat(keys[go], cnt) << 3) | (slot ^ flip[rays])
        nds = c[has]
        level += 1
    ar, an, ak, ain, aout, af = (np.concatenate(x) for x in acc)
    ain, aout = ain.astype(np.float32), aout.astype(np.float32)
    out = miss_records(R)
    if not len(ar):
        return out
    order = np.lexsort((ak, ar))
    ar, an, ak, ain, aout, af = ar[order], an[order], ak[order], ain[order], aout[order], af[order]
    with np.errstate(all="ignore"):
        contrib = np.subtract(aout, ain, dtype=np.float32)
    cnt = np.bincount(ar, minlength=R)
    start = np.cumsum(cnt) - cnt
    length = np.zeros(R, np.float32)
    for k in range(int(cnt.max())):                                # the k-th accepted leaf of every ray that has one
        r = np.nonzero(cnt > k)[0]
        length[r] = np.add(length[r], contrib[start[r] + k], dtype=np.float32)
    hit = cnt > 0
    tent = np.full(R, np.inf, np.float32)
    np.minimum.at(tent, ar, ain)
    tex = np.full(R, -np.inf, np.float32)
    np.maximum.at(tex, ar, aout)
    w = np.nonzero(ain == tent[ar])[0]                             # the leaves of least tIn, in (ray, visit) order
    pick = w[np.lexsort((ak[w], -_morton(T.nodes, an[w]), ar[w]))]   # per ray: greatest Morton code, then first visited
    sel = pick[np.concatenate([[True], ar[pick][1:] != ar[pick][:-1]])]
    out["length"][hit] = length[hit]
    out["t_enter"][hit] = tent[hit]
    out["t_exit"][hit] = tex[hit]
    out["leaves"] = cnt
    out["node"][ar[sel]] = an[sel]
    out["face"][ar[sel]] = af[sel]
    if ties:
        return out, np.bincount(ar[w], minlength=R) > 1
    return out


class Octree64S(q.Octree64Q):
    """Octree64Q with the span rule's `length` in float64 and a bound of the float32 record's distance from it."""

    def _terms(self, o, d, nodes):
        """ref64.Octree64._slab_terms with one addition: an axis on which the direction is zero and the origin lies within
        float32's error of one of the box's planes (Octree64Q._slab's borderline case) is left out of tNear / tFar -- on it the
        float32 box may hold the origin or not, whatever float64 says -- and reported as `flat`."""
        bmin, bmax = self.bmin[nodes], self.bmax[nodes]
        zero = d == 0.0
        mag = self.bmag[nodes][:, None] + np.abs(o)
        near = (np.abs(o - bmin) <= ref64.K * ref64.EPS * mag) | (np.abs(o - bmax) <= ref64.K * ref64.EPS * mag)
        flat = zero & near
        with np.errstate(all="ignore"):
            inv = 1.0 / d
            t1 = (bmin - o) * inv
            t2 = (bmax - o) * inv
            tmin = np.where(flat, -np.inf, np.minimum(t1, t2))
            tmax = np.where(flat, np.inf, np.maximum(t1, t2))
            tn, tf = tmin.max(1), tmax.min(1)
            ea = np.where(zero, 0.0, ref64.K * ref64.EPS * (mag * np.abs(inv) + np.maximum(np.abs(t1), np.abs(t2))))
            en = np.where(np.isfinite(tn), (tmin + ea).max(1) - tn, 0.0)
            ef = np.where(np.isfinite(tf), tf - (tmax - ea).min(1), 0.0)
        return tn, tf, en, ef, flat.any(1)

    def span_windows(self, o, d, t_min=0.0, t_max=1e30):
        """dict(length, tol, leaves, flat) per ray; every ray is covered, none is excluded.  flat: the ray's bound carries a
        whole chord (see below).

        length: sum of max(0, min(tFar, t_hi) - max(t_lo, tNear)) over the solid leaves float64 accepts (the rule of span32 on the
        float64 boxes); the order of a float64 sum is immaterial at the tolerance below.

        tol: `length` is continuous in the decisions.  Let e(v) = en(v) + ef(v) be the float32 slab test's first-order error in
        tNear and tFar of box v (ref64's per-axis terms, safety factor K).  For a leaf both sides accept, the float32 chord tOut -
        tIn differs from the float64 one by at most e(leaf): t_lo and t_hi are the same floats on both sides, max and min do not
        amplify.  For a leaf one side accepts and the other does not, some decision on its path came out differently: a slab test
        (tNear <= tFar, tFar > 0) of the leaf or of an ancestor a, or the leaf's tIn <= tFar or tIn <= t_hi.  Each such decision can
        only flip when its two sides lie within e of each other, and each bounds the chord: the leaf's chord lies inside a's, which
        is tFar(a) - tNear(a) <= e(a) at a flipped slab test; tFar - tIn <= e(leaf) and t_hi - tIn <= en(leaf) at the leaf's own.
        So every leaf that either side may accept contributes at most E(leaf) = max(e(leaf), max over ancestors e(a)) to the
        difference, and tol sums E over these leaves: the ones float64 accepts and the ones reached through boxes that pass or are
        borderline whose own acceptance holds when every threshold is relaxed by its error.  One case has no small bound: a ray
        with a zero direction component whose origin lies within float32's error of a box plane on that axis (`flat`) is inside the
        float32 slab or outside it as the rounding of the plane falls, and so is its whole chord; for such a leaf its chord over
        the other axes is added to E.  (An ancestor that is flat on a plane the leaf does not share holds the origin outside the
        leaf's slab on both sides.)  Last, the float32 sum of n contributions in sequence is off by at most (n - 1) 2^-24 of the
        largest partial sum, and each subtraction by 2^-24 of its result: together under leaves 2^-23 length."""
        o = np.asarray(o, np.float64).reshape(-1, 3)
        d = np.asarray(d, np.float64).reshape(-1, 3)
        R = len(d)
        tmn, tmx, tlo, thi = q.windows(t_min, t_max, R)
        valid = ~(np.isnan(o).any(1) | np.isnan(d).any(1)) & (tmn <= tmx)
        tlo, thi = tlo.astype(np.float64), thi.astype(np.float64)
        length, tol = np.zeros(R), np.zeros(R)
        leaves, maybe = np.zeros(R, np.int64), np.zeros(R, np.int64)
        flat_ray = np.zeros(R, bool)
        rays = np.nonzero(valid)[0]
        nds = np.zeros(len(rays), np.int64)
        nom = np.ones(len(rays), bool)                               # every ancestor passed in float64
        perr = np.zeros(len(rays))                                   # max e over the ancestors
        while len(rays):
            ok, amb = self._slab(o[rays], d[rays], nds)
            tn, tf, en, ef, flat = self._terms(o[rays], d[rays], nds)
            e = en + ef
            with np.errstate(invalid="ignore"):
                tin = np.maximum(tlo[rays], tn)
                tout = np.minimum(tf, thi[rays])
                chord = np.where(np.isfinite(tout - tin), np.maximum(0.0, tout - tin), 0.0)
                a64 = nom & ok & (tin <= tf) & (tin <= thi[rays])
                loose = (tn <= tf + e) & (tf > -ef) & (tin <= tf + e) & (tn <= thi[rays] + en)
            sol = self.solid[nds]
            E = np.maximum(e, perr) + np.where(flat, chord, 0.0)
            cand = sol & (a64 | ((ok | amb | flat) & loose))
            np.add.at(length, rays[sol & a64], chord[sol & a64])
            np.add.at(tol, rays[cand], E[cand])
            np.add.at(leaves, rays[sol & a64], 1)
            np.add.at(maybe, rays[cand], 1)
            flat_ray[rays[cand & flat & (chord > 0)]] = True
            go = (ok | amb | flat) & ~self.leafy[nds]
            c = self.child[nds[go]]
            has = c >= 0
            cnt = has.sum(1)
            rays = np.repeat(rays[go], cnt)
            nom = np.repeat((nom & ok)[go], cnt)
            perr = np.repeat(np.maximum(perr, e)[go], cnt)
            nds = c[has]
        return dict(length=length, leaves=leaves, tol=tol + maybe * 2.0 ** -23 * length, flat=flat_ray)


def slab_scene():
    """A 16^3 grid (voxel 2^-4, origin -0.5: every plane is an exact float) of solid z-slabs 1, 2 and 5 voxels thick with gaps
    between: z in [2, 3), [5, 7), [9, 14).  Returns (dense (z, y, x) uint8 grid, grid_min, voxel)."""
    g = np.zeros((16, 16, 16), np.uint8)
    for z0, z1 in SLABS:
        g[z0:z1] = 1
    return g, np.array([-0.5, -0.5, -0.5], np.float32), F(2.0 ** -4)


SLABS = ((2, 3), (5, 7), (9, 14))
