"""The region-query rules (rto_query_points_*, rto_query_regions_*, rto_query_nearest_*) restated in
numpy int64 as a walk over a node array: the reference the GPU results are compared with byte for byte.  Below it, the same
three answers from the dense voxel grid alone, with no octree involved, which pin this file.

Quantisation in float64 from the float32 inputs, one IEEE operation at a time:
    pq = floor((p - gridMin) / voxelSize * 64 + 0.5), |pq| <= 2^27;  cq, eq: the edit rule's (edit_ref.quantize, op ignored);
    mq = floor(max_dist / voxelSize * 64 + 0.5) <= 2^28, max_dist >= 0, +inf: no limit.
Reach: from node 0 through nodes with isLeaf == 0 and isUniform == 0; every other reached node is a leaf, solid when isSolid == 1.
Nothing is pruned here: every reached leaf is looked at.  The one shortcut is in the count of a sphere inside one box: a box
whose farthest voxel is covered counts whole (a leaf of a deep tree holds 2^54 voxels)."""
from __future__ import annotations

import numpy as np

import edit_ref as er

POINT_HIT_DTYPE = np.dtype([("node", "<i4"), ("solid", "<i4"), ("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("size", "<i4"),
                            ("depth", "<i4"), ("reserved", "<i4")])
REGION_DTYPE = np.dtype([("filled", "<i8"), ("covered", "<i8"), ("solid_leaves", "<i4"), ("first_node", "<i4"),
                         ("reserved", "<i4", (2,))])
NEAR_POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("max_dist", "<f4")])
NEAREST_DTYPE = np.dtype([("dist2", "<i8"), ("node", "<i4"), ("size", "<i4"), ("cq", "<i4", (3,)), ("reserved", "<i4")])
LIMIT, MQ_LIMIT = 1 << 27, 1 << 28


def point_quantize(p, grid_min, voxel_size):
    """pq as an int64 (3,) array, or None for an invalid point."""
    p = np.asarray(p, np.float32).astype(np.float64)
    g = np.asarray(grid_min, np.float32).astype(np.float64)
    vs = np.float64(np.float32(voxel_size))
    if not (np.isfinite(vs) and vs > 0 and np.isfinite(p).all() and np.isfinite(g).all()):
        return None
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.floor((p - g) / vs * 64.0 + 0.5)
    if not (np.abs(f) <= LIMIT).all():
        return None
    return f.astype(np.int64)


def dist_quantize(max_dist, voxel_size):
    """mq as an int, None for no limit (+inf), or -1 for an invalid max_dist."""
    d = np.float64(np.float32(max_dist))
    vs = np.float64(np.float32(voxel_size))
    if np.isposinf(d):
        return None
    if not (np.isfinite(vs) and vs > 0) or np.isnan(d) or d < 0:
        return -1
    f = np.floor(d / vs * 64.0 + 0.5)
    return int(f) if f <= MQ_LIMIT else -1


class Tree:
    """The reached leaves of a node array and the domain: dims of the resident grid, or None for node 0's cube."""

    def __init__(self, nodes, grid_min, voxel_size, dims=None):
        self.nodes, self.min, self.voxel = nodes, np.asarray(grid_min, np.float32), np.float32(voxel_size)
        reached, stack = [], [0]
        while stack:
            i = stack.pop()
            nd = nodes[i]
            if nd["isLeaf"] == 0 and nd["isUniform"] == 0:
                stack.extend(int(c) for c in nd["child"] if c >= 0)
            else:
                reached.append(i)
        self.leaf = np.array(sorted(reached), np.int64)
        L = nodes[self.leaf]
        self.lo = np.stack([L["x"], L["y"], L["z"]], 1).astype(np.int64)
        self.size = L["size"].astype(np.int64)
        self.solid = L["isSolid"] == 1
        r = nodes[0]
        if dims is None:
            self.dom_lo = np.array([r["x"], r["y"], r["z"]], np.int64)
            self.dom_hi = self.dom_lo + int(r["size"])
        else:
            self.dom_lo, self.dom_hi = np.zeros(3, np.int64), np.asarray(dims, np.int64)
        self.root_log2 = int(r["size"]).bit_length() - 1


def locate(T: Tree, points):
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    out = np.zeros(len(pts), POINT_HIT_DTYPE)
    out["node"] = -1
    for k, p in enumerate(pts):
        pq = point_quantize(p, T.min, T.voxel)
        if pq is None:
            continue
        v = pq >> 6
        m = np.nonzero(((v >= T.lo) & (v < T.lo + T.size[:, None])).all(1))[0]
        if len(m):
            j = m[0]                                             # T.leaf ascends: the lowest node index
            out[k] = (T.leaf[j], int(T.solid[j]), T.lo[j, 0], T.lo[j, 1], T.lo[j, 2], T.size[j],
                      T.root_log2 - (int(T.size[j]).bit_length() - 1), 0)
    return out


def _count_box(shape, cq, eq, lo, hi):
    """Covered voxels of the quantised brush inside the voxel box [lo, hi] (inclusive), already inside the brush's bounding box."""
    n = hi - lo + 1
    if (n <= 0).any():
        return 0
    if shape == er.BOX:
        return int(n[0]) * int(n[1]) * int(n[2])
    r2 = (2 * int(eq[0])) ** 2
    D = [64 * (2 * np.arange(lo[a], hi[a] + 1, dtype=np.int64) + 1) - 2 * int(cq[a]) for a in range(3)]
    far2 = sum(int(max(abs(int(d[0])), abs(int(d[-1])))) ** 2 for d in D)
    if far2 <= r2:
        return int(n[0]) * int(n[1]) * int(n[2])
    dx2 = np.sort(D[0] * D[0])
    rem = r2 - (D[1] * D[1])[:, None] - (D[2] * D[2])[None, :]
    return int(np.searchsorted(dx2, rem.ravel(), side="right").sum())


def census(T: Tree, brushes):
    out = np.zeros(len(brushes), REGION_DTYPE)
    for k, b in enumerate(brushes):
        shape = int(b["shape"])
        q = er.quantize(b["centre"], b["extent"], shape, er.CARVE, T.min, T.voxel)      # the op is ignored
        if q is None:
            out[k]["filled"] = out[k]["covered"] = -1
            out[k]["first_node"] = -1
            continue
        cq, eq = q
        e = np.array([eq[0]] * 3 if shape == er.SPHERE else eq, np.int64)
        blo = np.maximum(-((-(cq - e - 32)) // 64), T.dom_lo)
        bhi = np.minimum((cq + e - 32) // 64, T.dom_hi - 1)
        covered = _count_box(shape, cq, eq, blo, bhi)
        filled, leaves, first = 0, 0, -1
        if covered:
            lo = np.maximum(T.lo, blo)
            hi = np.minimum(T.lo + T.size[:, None] - 1, bhi)
            for j in np.nonzero(T.solid & (lo <= hi).all(1))[0]:
                c = _count_box(shape, cq, eq, lo[j], hi[j])
                if c:
                    filled += c
                    leaves += 1
                    first = int(T.leaf[j]) if first < 0 else first
        out[k] = (filled, covered, leaves, first, (0, 0))
    return out


def nearest(T: Tree, points, max_dist=np.inf):
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    md = np.broadcast_to(np.asarray(max_dist, np.float32), (len(pts),))
    out = np.zeros(len(pts), NEAREST_DTYPE)
    out["dist2"], out["node"] = -1, -1
    s = np.nonzero(T.solid)[0]
    lo, hi = 64 * T.lo[s], 64 * (T.lo[s] + T.size[s, None])
    for k, p in enumerate(pts):
        pq = point_quantize(p, T.min, T.voxel)
        mq = dist_quantize(md[k], T.voxel)
        if pq is None or mq == -1 or not len(s):
            continue
        c = np.clip(pq, lo, hi)
        d2 = ((pq - c) ** 2).sum(1)
        j = int(np.argmin(d2))                                   # the first of the least: s ascends with the node index
        if mq is None or int(d2[j]) <= mq * mq:
            out[k] = (d2[j], T.leaf[s[j]], T.size[s[j]], c[j], 0)
    return out


# ================================================================ the same from the dense grid alone
def dense_census(grid, brush, grid_min, voxel_size):
    """(filled, covered) of one BRUSH_DTYPE record on a (dimZ, dimY, dimX) uint8 grid, or None when it is invalid."""
    q = er.quantize(brush["centre"], brush["extent"], int(brush["shape"]), er.CARVE, grid_min, voxel_size)
    if q is None:
        return None
    m = er.cover((grid.shape[2], grid.shape[1], grid.shape[0]), int(brush["shape"]), *q)
    return int((m & (grid == 1)).sum()), int(m.sum())


def dense_nearest2(grid, pq, mq):
    """Least squared distance in 1/64 units from pq to the closed box of a FILLED voxel, -1 if none within mq (None: no limit)."""
    z, y, x = np.nonzero(grid == 1)
    if not len(x):
        return -1
    lo = 64 * np.stack([x, y, z], 1).astype(np.int64)
    d2 = int(((pq - np.clip(pq, lo, lo + 64)) ** 2).sum(1).min())
    return d2 if mq is None or d2 <= mq * mq else -1


def dense_leaf_ok(grid, root_size, hit, v):
    """Is `hit` the octree leaf of voxel v, judged from the grid alone?  Its box holds v, is aligned to its size, is uniform (voxels
    outside the grid count as EMPTY) with the recorded value, and its parent's box is not (or it is the root)."""
    def cell(lo, size):
        dz, dy, dx = grid.shape
        sub = grid[max(lo[2], 0):min(lo[2] + size, dz), max(lo[1], 0):min(lo[1] + size, dy), max(lo[0], 0):min(lo[0] + size, dx)]
        ones = int((sub == 1).sum())
        return 0 if ones == 0 else (1 if ones == size ** 3 else 2)   # EMPTY, FILLED, mixed

    lo, size = np.array([hit["x"], hit["y"], hit["z"]], np.int64), int(hit["size"])
    if not ((v >= lo) & (v < lo + size)).all() or (lo % size).any():
        return False
    state = cell(lo, size)
    if state != (1 if hit["solid"] else 0):
        return False
    return size == root_size or cell(lo - lo % (2 * size), 2 * size) == 2
