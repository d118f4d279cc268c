"""The field isosurface rule in numpy float32: every float operation below is one IEEE float32 operation, in
the order the rule writes it.  The case table is the project's own (ray_tracing_octrees_amd/host/mc_cases.inc), which
tests/golden/make_golden_iso.py proves equal to the reference's edgeTable / triTable.

    extract(volume, gmin, vs, level, ...) -> (tris (n, 12) float32, tri_cell (n,) int32, summary dict)
    marching_cubes_volume(field, origin, spacing, iso) -> (n, 12): the reference's marchingCubesVolume, placeholder normals (0, 1, 0)
    unmatched_edges(tris) -> directed edges whose reverse does not occur exactly as often (0: a closed, consistently oriented list)
"""
from __future__ import annotations

import os
import re

import numpy as np

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORNER = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)], np.int64)      # x, y, z
EDGE_A = np.array([0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3], np.int64)
EDGE_B = np.array([1, 2, 3, 0, 5, 6, 7, 4, 4, 5, 6, 7], np.int64)
EPS = F(1e-6)


def load_tables():
    """(tri_edges (256, 15) int, -1 padded; tri_count (256,)) from host/mc_cases.inc."""
    text = open(os.path.join(ROOT, "ray_tracing_octrees_amd", "host", "mc_cases.inc")).read()
    rows = re.findall(r'"([0-9a-f]*)f"', text)
    assert len(rows) == 256, len(rows)
    edges = np.full((256, 15), -1, np.int64)
    for i, r in enumerate(rows):
        assert len(r) % 3 == 0 and len(r) <= 15
        edges[i, :len(r)] = [int(ch, 16) for ch in r]
    return edges, (edges >= 0).sum(axis=1) // 3


TRI_EDGES, TRI_COUNT = load_tables()


def cells_of_samples(S, level):
    """S (sz, sy, sx) float32 samples -> (case (sz-1, sy-1, sx-1) of every cell)."""
    below = S < F(level)
    case = np.zeros(tuple(n - 1 for n in S.shape), np.int64)
    for i, (dx, dy, dz) in enumerate(CORNER):
        case |= below[dz:dz + case.shape[0], dy:dy + case.shape[1], dx:dx + case.shape[2]].astype(np.int64) << i
    return case


def triangles_of_samples(S, first, origin, spacing, level):
    """Marching cubes of the sample block S (sz, sy, sx), whose sample [0, 0, 0] has the index first = (x, y, z); cells in z, y, x
    order.  Returns (verts (n, 9) float32, cell (n, 3) int64: the owning cell's x, y, z index)."""
    S = np.ascontiguousarray(S, F)
    if min(S.shape) < 2:
        return np.zeros((0, 9), F), np.zeros((0, 3), np.int64)
    level, spacing = F(level), F(spacing)
    origin = np.asarray(origin, F)
    case = cells_of_samples(S, level)
    cz, cy, cx = np.nonzero(TRI_COUNT[case] > 0)                      # C order: z slowest, x fastest
    cs = case[cz, cy, cx]
    n = TRI_COUNT[cs]
    rank = np.repeat(np.arange(len(cs)), n)                           # the cell of every triangle, in order
    t = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)      # 0 .. k - 1 within each cell
    cell = np.stack([cx + first[0], cy + first[1], cz + first[2]], axis=1)[rank]
    local = np.stack([cx, cy, cz], axis=1)[rank]
    verts = np.zeros((len(rank), 9), F)
    with np.errstate(all="ignore"):
        for q in range(3):
            e = TRI_EDGES[cs[rank], 3 * t + q]
            a, b = EDGE_A[e], EDGE_B[e]
            la, lb = local + CORNER[a], local + CORNER[b]
            v1, v2 = S[la[:, 2], la[:, 1], la[:, 0]], S[lb[:, 2], lb[:, 1], lb[:, 0]]
            p1 = origin[None, :] + (cell + CORNER[a]).astype(F) * spacing
            p2 = origin[None, :] + (cell + CORNER[b]).astype(F) * spacing
            mu = (level - v1) / (v2 - v1)
            mid = p1 + mu[:, None] * (p2 - p1)
            snap1 = np.abs(level - v1) < EPS
            snap2 = np.abs(level - v2) < EPS
            flat = np.abs(v1 - v2) < EPS
            v = np.where(snap1[:, None], p1, np.where(snap2[:, None], p2, np.where(flat[:, None], p1, mid)))
            verts[:, 3 * q:3 * q + 3] = v.astype(F)
    return verts, cell


def face_normals(verts):
    """localMC's face normal of (n, 9) vertices, (+0, +0, +0) where the squared length is not positive and finite."""
    v0, v1, v2 = verts[:, 0:3], verts[:, 3:6], verts[:, 6:9]
    a, b = v1 - v0, v2 - v0
    with np.errstate(all="ignore"):
        cx = a[:, 1] * b[:, 2] - b[:, 1] * a[:, 2]
        cy = a[:, 2] * b[:, 0] - b[:, 2] * a[:, 0]
        cz = a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]
        l2 = (cx * cx + cy * cy) + cz * cz
        ok = (l2 > 0) & np.isfinite(l2)
        inv = F(1.0) / np.sqrt(l2)
        n = np.stack([cx * inv, cy * inv, cz * inv], axis=1).astype(F)
    n[~ok] = F(0.0)
    return n, ~ok


def samples(volume, level=None, outside=1.0e9, valid=(0, 0x7ffffffe), pad=True, clip=None):
    """The substituted float samples of the cell box and the index (x, y, z) of the first one."""
    vol = np.asarray(volume, np.int32)
    dz, dy, dx = vol.shape
    lo = np.array(clip[0] if clip is not None else (0, 0, 0), np.int64)
    hi = np.array(clip[1] if clip is not None else (dx, dy, dz), np.int64)
    p = 1 if pad else 0
    box = vol[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
    val = np.where((box >= valid[0]) & (box <= valid[1]), box.astype(F), F(outside)).astype(F)
    S = np.full(tuple(n + 2 * p for n in val.shape), F(outside), F)
    S[p:p + val.shape[0], p:p + val.shape[1], p:p + val.shape[2]] = val
    return S, lo - p


def extract(volume, gmin, vs, level, outside=1.0e9, valid=(0, 0x7ffffffe), pad=True, clip=None):
    vol = np.asarray(volume, np.int32)
    dz, dy, dx = vol.shape
    vs = F(vs)
    origin = np.asarray(gmin, F) + F(0.5) * vs
    S, first = samples(vol, level, outside, valid, pad, clip)
    verts, cell = triangles_of_samples(S, first, origin, vs, level)
    normals, degenerate = face_normals(verts)
    tris = np.concatenate([verts, normals], axis=1).astype(F)
    tri_cell = (((cell[:, 2] + 1) * (dy + 1) + (cell[:, 1] + 1)) * (dx + 1) + (cell[:, 0] + 1)).astype(np.int32)
    summary = {"triangles": len(tris), "active_cells": len(np.unique(tri_cell)), "degenerate": int(degenerate.sum())}
    return tris, tri_cell, summary


def marching_cubes_volume(field, origin, spacing, iso):
    """The reference's marchingCubesVolume on a (dimZ, dimY, dimX) float field: (n, 12) with its placeholder normal (0, 1, 0)."""
    verts, _ = triangles_of_samples(np.asarray(field, F), np.zeros(3, np.int64), origin, spacing, iso)
    normal = np.tile(np.array([0.0, 1.0, 0.0], F), (len(verts), 1))
    return np.concatenate([verts, normal], axis=1).astype(F)


def unmatched_edges(tris):
    """Directed edges (by bitwise vertices) minus their reverses: the number left over, 0 for a closed oriented surface."""
    v = np.ascontiguousarray(np.asarray(tris, F)[:, :9]).view(np.uint32).reshape(-1, 3, 3)
    from collections import Counter
    count = Counter()
    for tri in v:
        k = [tuple(int(w) for w in tri[i]) for i in range(3)]
        for i in range(3):
            count[(k[i], k[(i + 1) % 3])] += 1
    return sum(abs(n - count.get((e[1], e[0]), 0)) for e, n in count.items())
