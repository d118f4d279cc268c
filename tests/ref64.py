"""Float64 references of the box renderer (Octree64.trace_boxes: first hit, closest hit, stack depth) and of config 5's
leaf-triangle renderer (TriScene64; test code only).

Written from the rules of the path, not from the oracle's source:
  * primary ray: the float32 ray of generate_rays (pinned elsewhere); the octree is walked depth-first with a LIFO
    stack (children pushed 0..7, so child 7 is popped first), at most 512 pops; a popped node whose box the ray misses
    (slab test: tNear <= tFar, tFar > 0) is dropped; a popped leaf (isLeaf or isUniform) that passes is tested against
    its triangles (Moeller-Trumbore, t > 0); the first such leaf with any hit ends the ray, with its nearest triangle.
  * shading: the triangle's stored normal turned towards the viewer, Lambert term max(0, n . normalize(1, 1, 1)).
  * shadow: from the hit point p, offset by voxelSize * 1e-3 + 2^-18 max|p| along that normal, a ray towards the light through the same
    walk; any triangle hit darkens the pixel to the ambient term.  The hit point lies on the hit triangle's plane: its
    float32 form may only carry rounding errors of the size of p's own coordinates, never ones that grow with the
    distance travelled by the ray.
  * brute force (`any_hits`): every triangle against every ray.  The tree only prunes the candidate pairs: each
    triangle lies inside its own leaf's closed box, which a ray must then enter (`test_triangles_lie_inside_their_leaves`).

Every decision is evaluated in float64 together with a first-order bound of the error the float32 kernels may make in
it; a pixel is *robust* when no decision it depends on lies within that bound of its threshold.  Tests compare robust
pixels only and bound the share of the others.
"""
from __future__ import annotations

import numpy as np

EPS = 2.0 ** -24                # unit roundoff of float32
K = 4.0                         # safety factor on the first-order error bounds
DET_MIN = 1e-12                 # Moeller-Trumbore's degenerate-triangle threshold
MAX_POPS = 512
LIGHT = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)


def _dot(a, b):
    return (a * b).sum(-1)


def _norm(a):
    return np.sqrt((a * a).sum(-1))


class Octree64:
    """The node boxes in float64 and the walk order; shared by the box and the triangle renderers."""

    def __init__(self, nodes, grid_min, voxel_size):
        n = len(nodes)
        self.n = n
        self.child = np.asarray(nodes["child"], np.int64).reshape(n, 8)
        self.leafy = (nodes["isLeaf"] == 1) | (nodes["isUniform"] == 1)
        self.solid = self.leafy & (nodes["isSolid"] == 1)
        vs = float(np.float32(voxel_size))
        gmin = np.asarray(grid_min, np.float64).reshape(3)
        xyz = np.stack([nodes["x"], nodes["y"], nodes["z"]], 1).astype(np.float64)
        self.bmin = gmin + xyz * vs
        self.bmax = self.bmin + nodes["size"].astype(np.float64)[:, None] * vs
        self.bmag = np.maximum(np.abs(self.bmin), np.abs(self.bmax)).max(1)
        self.bias = vs * 1e-3
        self.rank = self._preorder_rank()
        self.below, self.pushes = self._stack_depths()

    def _preorder_rank(self):
        """Pop position of every node in a walk that enters everything (LIFO, child 7 first)."""
        n = self.n
        if n == 0:
            return np.zeros(0, np.int64)
        ch = np.where(self.leafy[:, None], -1, self.child)
        parent = np.full(n, -1, np.int64)
        p_idx, _ = np.nonzero(ch >= 0)
        parent[ch[ch >= 0]] = p_idx
        depth = np.zeros(n, np.int64)
        level = [np.array([0])]
        while True:
            c = ch[level[-1]]
            c = c[c >= 0]
            if not len(c):
                break
            depth[c] = len(level)
            level.append(c)
        size = np.ones(n, np.int64)
        for lv in reversed(level[1:]):
            np.add.at(size, parent[lv], size[lv])
        rank = np.zeros(n, np.int64)
        for lv in level:
            c = ch[lv]
            cs = np.where(c >= 0, size[np.maximum(c, 0)], 0)
            after = np.cumsum(cs[:, ::-1], 1)[:, ::-1] - cs          # sizes of the siblings popped before child j (j+1..7)
            r = rank[lv][:, None] + 1 + after
            ok = c >= 0
            rank[c[ok]] = r[ok]
        return rank

    # ---------------------------------------------------------------- slab test over (ray, node) pairs
    def _slab_terms(self, o, d, nodes):
        """tNear, tFar of (ray, box) pairs and first-order bounds of the float32 slab test's errors in them.  Each axis
        has its own bound; tNear = max over the axes can only move by as much as an axis whose interval comes within
        its own bound of it (likewise tFar)."""
        bmin, bmax = self.bmin[nodes], self.bmax[nodes]
        zero = d == 0.0
        with np.errstate(all="ignore"):
            inv = 1.0 / d
            t1 = (bmin - o) * inv
            t2 = (bmax - o) * inv
            tmin, tmax = np.minimum(t1, t2), np.maximum(t1, t2)
            tn, tf = tmin.max(1), tmax.min(1)
            ea = np.where(zero, 0.0, K * EPS * ((self.bmag[nodes][:, None] + np.abs(o)) * np.abs(inv) + np.maximum(np.abs(t1), np.abs(t2))))
            en = np.where(np.isfinite(tn), (tmin + ea).max(1) - tn, 0.0)
            ef = np.where(np.isfinite(tf), tf - (tmax - ea).min(1), 0.0)
        return tn, tf, en, ef

    def _slab(self, o, d, nodes):
        tn, tf, en, ef = self._slab_terms(o, d, nodes)
        zero = d == 0.0
        with np.errstate(all="ignore"):
            passes = (tn <= tf) & (tf > 0) & (tn < 1e30)
            amb = np.isnan(tn) | np.isnan(tf) | (np.abs(tn - tf) <= en + ef) | (np.abs(tf) <= ef)
            amb |= zero.any(1) & ((o == self.bmin[nodes]) | (o == self.bmax[nodes])).any(1)
        return passes & ~np.isnan(tn), amb

    def _walk(self, o, d, R):
        """All (ray, leaf) pairs a walk can reach when every nominal or borderline slab decision is taken as a pass.
        Per pair: nominal (every box on the way, the leaf's included, passes in float64), path_amb (one of them is
        borderline), and the nodes the nominal walk pops (ray, rank, borderline, passes) for the pop count."""
        rays = np.arange(R)
        nds = np.zeros(R, np.int64)
        nom_reach = np.ones(R, bool)           # every ancestor passed nominally: the node is popped in the nominal walk
        amb_path = np.zeros(R, bool)
        leaf_r, leaf_n, leaf_nom, leaf_amb = [], [], [], []
        pop_r, pop_rank, pop_amb, pop_ok = [], [], [], []
        while len(rays):
            ok, amb = self._slab(o[rays], d[rays], nds)
            pop_r.append(rays[nom_reach]); pop_rank.append(self.rank[nds[nom_reach]]); pop_amb.append(amb[nom_reach])
            pop_ok.append(ok[nom_reach])
            go = ok | amb
            nom = nom_reach & ok
            pa = amb_path | amb
            lf = self.leafy[nds]
            sel = go & lf
            leaf_r.append(rays[sel]); leaf_n.append(nds[sel]); leaf_nom.append(nom[sel]); leaf_amb.append(pa[sel])
            sel = go & ~lf
            c = self.child[nds[sel]]
            has = c >= 0
            cnt = has.sum(1)
            rays = np.repeat(rays[sel], cnt); nds = c[has]
            nom_reach = np.repeat(nom[sel], cnt); amb_path = np.repeat(pa[sel], cnt)
        cat = np.concatenate
        return (cat(leaf_r), cat(leaf_n), cat(leaf_nom), cat(leaf_amb)), (cat(pop_r), cat(pop_rank), cat(pop_amb), cat(pop_ok))

    def _stack_depths(self):
        """below[v]: entries under v on the stack when v is popped (the siblings pushed before each node on its path);
        pushes[v]: children v pushes.  An internal node that passes leaves below + pushes entries on the stack."""
        ch = np.where(self.leafy[:, None], -1, self.child)
        has = ch >= 0
        pos = np.cumsum(has, 1) - has
        below = np.zeros(self.n, np.int64)
        level = np.array([0])
        while len(level):
            c, p = ch[level], pos[level]
            ok = c >= 0
            below[c[ok]] = np.repeat(below[level], ok.sum(1)) + p[ok]
            level = c[ok]
        return below, has.sum(1)


    def _entry(self, o, d, nodes):
        """Float64 tNear of (ray, box) pairs and a first-order bound of the float32 slab test's error in it."""
        tn, _, en, _ = self._slab_terms(o, d, nodes)
        return tn, en

    def _shade(self, o, d, leaf, tn, terr):
        """n . l of the hit on a leaf box (n = normalize(p - centre), p = o + d max(0, tNear)) and a bound of its float32 error."""
        t = np.maximum(0.0, tn)
        p = o + d * t[:, None]
        v = p - 0.5 * (self.bmin[leaf] + self.bmax[leaf])
        nv = _norm(v)
        n = v / nv[:, None]
        perr = terr * _norm(d) + 2 * EPS * (np.abs(p).max(1) + self.bmag[leaf])
        return np.maximum(0.0, _dot(n, LIGHT)), 2.0 * perr / nv + 16 * EPS

    def trace_boxes(self, o, d):
        """The box renderer's two rules over rays (o, d), float64.
        first: the first solid leaf in pop order whose box passes (tHit = max(0, tNear) <= tFar), under the 512-pop cap.
        closest: the solid leaf with the smallest tHit among all whose box the ray meets (brute force over the leaves the
        walk reaches when nothing is pruned: boxes nest, so a leaf's box passes only when its ancestors' do); ties go to
        the leaf popped first.
        Per rule a dict: hit, leaf, shade (n . l), tol (float32 error bound of the shade), robust; first also `need`, the
        stack entries the nominal walk holds at most (a passed internal node leaves below + pushes entries)."""
        R = len(o)
        NONE = np.iinfo(np.int64).max
        (lr, ln, lnom, _), (pr, prank, pamb, pok) = self._walk(o, d, R)
        node_of = np.zeros(self.n, np.int64)
        node_of[self.rank[::-1]] = np.arange(self.n)[::-1]          # rank 0: the root (unreachable nodes share it)
        pnode = node_of[prank]
        live = ~self.leafy[pnode] | self.solid[pnode]                     # a borderline empty leaf changes nothing
        # ---- first hit
        sol = self.solid[ln]
        first = np.full(R, NONE)
        np.minimum.at(first, lr[sol & lnom], self.rank[ln[sol & lnom]])
        order = np.lexsort((prank, pr))
        pr_s, prank_s = pr[order], prank[order]
        start = np.searchsorted(pr_s, np.arange(R))
        cnt = np.bincount(pr_s, minlength=R)
        cap_rank = np.where(cnt >= MAX_POPS, prank_s[np.minimum(start + MAX_POPS - 1, len(pr_s) - 1)], NONE)
        stop = np.minimum(first, cap_rank)                                # the last node the walk pops
        upto = prank <= stop[pr]
        capped = (first != NONE) & (first > cap_rank)
        amb_before = np.zeros(R, bool)
        amb_before[pr[upto & pamb & live]] = True
        pushes = upto & pok & ~self.leafy[pnode]
        need = np.ones(R, np.int64)
        np.maximum.at(need, pr[pushes], self.below[pnode[pushes]] + self.pushes[pnode[pushes]])
        hit = (first != NONE) & ~capped
        leaf = np.where(hit, node_of[np.where(hit, first, 0)], -1)
        out_first = dict(hit=hit, leaf=leaf, need=need, robust=~amb_before, shade=np.zeros(R), tol=np.zeros(R))
        # ---- closest hit
        cand = sol
        cr, cl = lr[cand], ln[cand]
        tn, terr = self._entry(o[cr], d[cr], cl)
        th = np.maximum(0.0, tn)
        ok, amb = self._slab(o[cr], d[cr], cl)
        best = np.full(R, np.inf)
        np.minimum.at(best, cr[ok], th[ok])
        win = ok & (th == best[cr])
        wrank = np.full(R, NONE)
        np.minimum.at(wrank, cr[win], self.rank[cl[win]])
        chit = wrank != NONE
        cleaf = np.where(chit, node_of[np.where(chit, wrank, 0)], -1)
        is_w = win & (self.rank[cl] == wrank[cr])
        werr = np.zeros(R)
        werr[cr[is_w]] = terr[is_w]
        rival = ~is_w & (ok | amb) & ((th <= best[cr] + werr[cr] + terr) | np.isnan(th))
        crob = np.ones(R, bool)
        crob[cr[rival | (is_w & amb)]] = False
        out_close = dict(hit=chit, leaf=cleaf, robust=crob, shade=np.zeros(R), tol=np.zeros(R))
        for rule in (out_first, out_close):
            h = np.nonzero(rule["hit"])[0]
            t_, e_ = self._entry(o[h], d[h], rule["leaf"][h])
            rule["shade"][h], rule["tol"][h] = self._shade(o[h], d[h], rule["leaf"][h], t_, e_)
        return out_first, out_close


def render_boxes64(S: Octree64, ro, rd):
    """ro (3,) float32 eye, rd (N, 3) float32 directions: trace_boxes on the float64 rays."""
    d = np.asarray(rd, np.float64).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(ro, np.float64).reshape(1, 3), d.shape).copy()
    return S.trace_boxes(o, d)


class TriScene64(Octree64):
    def __init__(self, nodes, tris, tri_offset, grid_min, voxel_size):
        super().__init__(nodes, grid_min, voxel_size)
        t = np.asarray(tris, np.float64).reshape(-1, 12)
        self.v0, self.v1, self.v2, self.nrm = t[:, 0:3], t[:, 3:6], t[:, 6:9], t[:, 9:12]
        self.e1, self.e2 = self.v1 - self.v0, self.v2 - self.v0
        self.vmag = np.abs(t[:, 0:9]).max(1)
        self.off = np.asarray(tri_offset, np.int64)

    # ---------------------------------------------------------------- Moeller-Trumbore over (ray, triangle) pairs
    def _mt(self, o, d, k):
        v0, e1, e2 = self.v0[k], self.e1[k], self.e2[k]
        p = np.cross(d, e2)
        det = _dot(e1, p)
        tv = o - v0
        q = np.cross(tv, e1)
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            u = _dot(tv, p) * inv
            v = _dot(d, q) * inv
            t = _dot(e2, q) * inv
            ad = np.abs(det)
            ntv, ne1, ne2, nq, npp = _norm(tv), _norm(e1), _norm(e2), _norm(q), _norm(p)
            A = K * EPS * ntv                                                # float32 error of tv = ro - v0 and of its products
            ddet = K * EPS * ne1 * ne2
            du = (A * npp) / ad + np.abs(u) * ddet / ad
            dq = A * ne1
            dv = dq / ad + np.abs(v) * ddet / ad
            dt = (ne2 * dq + K * EPS * ne2 * nq) / ad + np.abs(t) * ddet / ad
            conds = [(ad - DET_MIN, ddet), (u, du), (1.0 - u, du), (v, dv), (1.0 - u - v, du + dv), (t, dt)]
            hit = np.ones(len(k), bool); sure_hit = np.ones(len(k), bool); sure_miss = np.zeros(len(k), bool)
            for x, e in conds:
                hit &= x >= 0
                sure_hit &= x > e
                sure_miss |= x < -e
            hit &= t > 0
        amb = ~sure_hit & ~sure_miss
        return hit, amb, t, dt

    def _pairs(self, leaf_r, leaf_n):
        lo, hi = self.off[leaf_n], self.off[leaf_n + 1]
        cnt = hi - lo
        pr = np.repeat(np.arange(len(leaf_r)), cnt)
        k = np.repeat(lo - np.cumsum(cnt) + cnt, cnt) + np.arange(cnt.sum())
        return pr, k

    # ---------------------------------------------------------------- the renderer's rule
    def _inside(self, o, d, t, leaf):
        """The hit point o + d t lies inside the leaf's box by more than the float32 slab test's error: every box
        on the way to the leaf then passes in float32 too."""
        pnt = o + d * t[:, None]
        slack = np.minimum(pnt - self.bmin[leaf], self.bmax[leaf] - pnt)
        err = K * EPS * (self.bmag[leaf][:, None] + np.abs(o) + np.abs(d * t[:, None]))
        with np.errstate(invalid="ignore"):
            return (slack > err).all(1)

    def trace_dfs(self, o, d):
        """The path's rule: first leaf in pop order with a triangle hit, under the 512-pop cap.
        Returns a dict: hit, tri, t, dt (error bound of t), robust (hit and triangle decided beyond float32's
        error), hit_robust (hit or miss decided beyond it, whichever triangle is taken)."""
        R = len(o)
        hit = np.zeros(R, bool); tri = np.full(R, -1, np.int64); tt = np.full(R, np.inf); dtt = np.zeros(R)
        robust = np.ones(R, bool)
        out = dict(hit=hit, tri=tri, t=tt, dt=dtt, robust=robust, hit_robust=robust.copy())
        if self.n == 0 or R == 0:
            return out
        (lr, ln, lnom, _), (pr, prank, pamb, _) = self._walk(o, d, R)
        pi, k = self._pairs(lr, ln)
        ray = lr[pi]
        h, a, t, dt = self._mt(o[ray], d[ray], k)
        rk = self.rank[ln[pi]]
        nominal = h & lnom[pi]
        NONE = np.iinfo(np.int64).max
        first = np.full(R, NONE)
        np.minimum.at(first, ray[nominal], rk[nominal])
        # pops up to the first hit leaf; past the cap the hit is never seen
        before = prank <= first[pr]
        pops = np.bincount(pr[before], minlength=R)
        nab = np.bincount(pr[before & pamb], minlength=R)
        capped = (first != NONE) & (pops > MAX_POPS)
        cap_robust = (first == NONE) | (pops + nab <= MAX_POPS) | (pops - nab > MAX_POPS)
        # borderline decisions up to the first hit leaf could move that leaf or the triangle chosen in it
        inside = np.zeros(len(k), bool)
        hs = np.nonzero(h | a)[0]
        inside[hs] = self._inside(o[ray[hs]], d[ray[hs]], np.where(np.isfinite(t[hs]), t[hs], 0.0), ln[pi][hs])
        upto = rk <= first[ray]
        bad = upto & (a | (h & ~inside))
        robust[ray[bad]] = False
        win = nominal & (rk == first[ray])
        order = np.lexsort((k[win], t[win], ray[win]))
        wr, wk, wt, wdt = ray[win][order], k[win][order], t[win][order], dt[win][order]
        firstrow = np.ones(len(wr), bool); firstrow[1:] = wr[1:] != wr[:-1]
        hit[wr[firstrow]] = True; tri[wr[firstrow]] = wk[firstrow]; tt[wr[firstrow]] = wt[firstrow]; dtt[wr[firstrow]] = wdt[firstrow]
        # a runner-up in the same leaf within the error of t (and with another normal) makes the choice borderline
        close = ~firstrow & (wt - tt[wr] <= wdt + dtt[wr]) & (np.abs(self.nrm[wk] - self.nrm[tri[wr]]).max(1) > 0)
        robust[wr[close]] = False
        # hit or miss alone: a hit ray is a hit in float32 too when some triangle is hit beyond doubt inside its
        # leaf (that leaf or an earlier one ends the walk); a miss ray must have no borderline pair at all
        sure = np.zeros(R, bool); sure[ray[h & ~a & inside]] = True
        amb_any = np.zeros(R, bool); amb_any[ray[a | (h & ~inside)]] = True
        hit_robust = np.where(hit, sure, ~amb_any) & cap_robust
        robust &= cap_robust & hit_robust
        hit &= ~capped
        tri[capped] = -1
        out["hit_robust"] = hit_robust
        return out

    def any_hits(self, o, d):
        """Brute force: every (ray, triangle, t) that float64 or float32 may call a hit (borderline pairs included),
        and per ray whether some triangle is hit beyond
        doubt (every decision clear of float32's error, the hit point inside its leaf's box by more than that)."""
        R = len(o)
        sure = np.zeros(R, bool)
        if self.n == 0 or R == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0), sure
        (lr, ln, _, _), _ = self._walk(o, d, R)
        pi, k = self._pairs(lr, ln)
        ray = lr[pi]
        h, a, t, _ = self._mt(o[ray], d[ray], k)
        hs = np.nonzero(h & ~a)[0]
        ins = self._inside(o[ray[hs]], d[ray[hs]], t[hs], ln[pi][hs])
        sure[ray[hs[ins]]] = True
        m = h | a
        return ray[m], k[m], t[m], sure


def _tangents(n):
    a = np.where(np.abs(n[:, :1]) < 0.6, np.array([1.0, 0, 0]), np.array([0, 1.0, 0]))
    t1 = np.cross(n, a); t1 /= _norm(t1)[:, None]
    return t1, np.cross(n, t1)


def render64(S: TriScene64, ro, rd, shadow=True):
    """ro (3,) float32 eye, rd (N, 3) float32 directions.  Per ray: hit, tri, robust, shade (the Lambert term before
    the shadow), shadowed, and R - 0.1 as the renderer must produce it."""
    o = np.broadcast_to(np.asarray(ro, np.float64).reshape(1, 3), rd.shape).copy()
    d = np.asarray(rd, np.float64).reshape(-1, 3)
    N = len(d)
    r = S.trace_dfs(o, d)
    hit, tri, t, dt, robust = r["hit"], r["tri"], r["t"], r["dt"], r["robust"]
    shadow_robust = r["hit_robust"].copy()
    shade = np.zeros(N)
    shadowed = np.zeros(N, bool)
    hi = np.nonzero(hit)[0]
    n = S.nrm[tri[hi]]
    nd = _dot(n, d[hi])
    robust[hi[np.abs(nd) <= K * EPS * 4]] = False                         # the normal's turn is borderline
    n = np.where((nd > 0)[:, None], -n, n)
    nl = _dot(n, LIGHT)
    shade[hi] = np.maximum(0.0, nl)
    if shadow and len(hi):
        lit = nl > 1e-6                                                   # darker than that, the verdict cannot show
        hl, nlit = hi[lit], n[lit]
        p = o[hl] + d[hl] * t[hl][:, None]
        bias = S.bias + 2.0 ** -18 * np.abs(p).max(1)                   # the offset never drops below 2^-18 max|p|
        so = p + nlit * bias[:, None]
        # float32 error of the shadow origin: along the plane, that of p (t's error plus the rounding of ro + rd t);
        # across it, a few ulps of p's and the triangle's coordinates
        e_lat = dt[hl] + K * EPS * (np.abs(o[hl]).max(1) + t[hl])
        e_h = 4 * EPS * (np.abs(p).max(1) + S.vmag[tri[hl]])
        shadow_robust[hl[bias <= 2 * e_h]] = False
        a, b = _tangents(nlit)
        L = np.broadcast_to(LIGHT, so.shape)
        verdicts = []
        for off in (0 * a, e_lat[:, None] * a, -e_lat[:, None] * a, e_lat[:, None] * b, -e_lat[:, None] * b,
                    e_h[:, None] * nlit, -e_h[:, None] * nlit):
            sr = S.trace_dfs(so + off, L)
            shadow_robust[hl[~sr["hit_robust"]]] = False
            verdicts.append(sr["hit"])
        verdicts = np.stack(verdicts)
        shadow_robust[hl[(verdicts != verdicts[0]).any(0)]] = False
        shadowed[hl] = verdicts[0]
    robust &= shadow_robust
    value = np.where(shadowed, 0.0, shade)
    return dict(hit=hit, tri=tri, t=t, robust=robust, hit_robust=r["hit_robust"], shadow_robust=shadow_robust,
                shade=shade, shadowed=shadowed, value=value)
