"""Float32 numpy statement of the mesh-extraction rule (include/rto_hip.h, rto_extract_mesh): the triangle
list the reference's renderOctree makes -- a depth-first walk of the octree, children in slots 0..7, that drops every subtree whose
box fails Frustum::testAABB(min, max, margin) and runs MarchingCubesRenderer or VoxelCubeRenderer on every surviving leaf.

Every operation below is one IEEE float32 operation (numpy float32 arrays and scalars never widen).  The octree is a flat GPUNodes
array (the oracle's build_flat_octree), the MC triangles are the leaf-triangle buffer (12 floats per triangle, tri_offset per node)."""
from __future__ import annotations

import numpy as np

F = np.float32
MESH_MC, MESH_CUBES = 0, 1

# corners of a face in addFace*'s order, bit a = the max corner's coordinate on axis a; faces +X, -X, +Y, -Y, +Z, -Z
FACE_CORNERS = ((1, 3, 7, 5), (0, 4, 6, 2), (2, 6, 7, 3), (0, 1, 5, 4), (4, 6, 7, 5), (0, 1, 3, 2))
FACE_NORMALS = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))


def boxes(nodes, grid_min, voxel):
    """min and max corner of every node: min = gridMin + (float)xyz * voxelSize, max = min + (float)size * voxelSize."""
    gm = np.asarray(grid_min, F)
    vs = F(voxel)
    xyz = np.stack([nodes["x"], nodes["y"], nodes["z"]], 1).astype(F)
    mn = gm[None, :] + xyz * vs
    ext = nodes["size"].astype(F) * vs
    return mn, mn + ext[:, None]


def passes(planes, margin, mn, mx):
    """testAABB(min, max, margin) != -1 for every box: only the positive-vertex test can return -1."""
    pl = np.asarray(planes, F).reshape(6, 4)
    m = F(margin)
    emn, emx = mn - m, mx + m
    ok = np.ones(len(mn), bool)
    for i in range(6):
        p = [emx[:, a] if pl[i, a] > 0 else emn[:, a] for a in range(3)]
        t = (pl[i, 0] * p[0] + pl[i, 1] * p[1]) + pl[i, 2] * p[2]
        ok &= ~((t + pl[i, 3]) < 0)
    return ok


def visible_leaves(nodes, grid_min, voxel, planes=None, margin=50.0):
    """Indices of the leaves renderOctree reaches, in the order it reaches them."""
    if len(nodes) == 0:
        return []
    if planes is None:
        ok = np.ones(len(nodes), bool)
    else:
        ok = passes(planes, margin, *boxes(nodes, grid_min, voxel))
    leaf = nodes["isLeaf"] == 1
    uniform = nodes["isUniform"] == 1
    child = nodes["child"]
    out, stack = [], [0]
    while stack:
        i = stack.pop()
        if not ok[i]:
            continue
        if leaf[i]:
            out.append(i)
            continue
        if uniform[i]:                                     # terminal for every traversal of the array; no leaf, so nothing to emit
            continue
        stack.extend(int(c) for c in child[i][::-1] if c >= 0)
    return out


def cube_faces(node, grid_min, voxel, data):
    """addBlockFaces on one solid leaf: (k, 12) float32, two triangles per exposed face."""
    dz, dy, dx = data.shape
    x0, y0, z0, s = int(node["x"]), int(node["y"]), int(node["z"]), int(node["size"])
    h = s // 2
    gm = np.asarray(grid_min, F)
    vs = F(voxel)
    lo = gm + np.array([x0, y0, z0], F) * vs
    hi = lo + np.array([s, s, s], F) * vs
    tests = ((x0 + s, y0 + h, z0 + h), (x0 - 1, y0 + h, z0 + h), (x0 + h, y0 + s, z0 + h), (x0 + h, y0 - 1, z0 + h),
             (x0 + h, y0 + h, z0 + s), (x0 + h, y0 + h, z0 - 1))
    out = []
    for f, (tx, ty, tz) in enumerate(tests):
        outside = tx < 0 or ty < 0 or tz < 0 or tx >= dx or ty >= dy or tz >= dz
        if not (outside or data[tz, ty, tx] == 0):
            continue
        v = [np.array([hi[a] if (c >> a) & 1 else lo[a] for a in range(3)], F) for c in FACE_CORNERS[f]]
        n = np.array(FACE_NORMALS[f], F) + F(0)            # -0 never appears: 0 + 0 = +0
        out.append(np.concatenate([v[0], v[1], v[3], n]))
        out.append(np.concatenate([v[3], v[1], v[2], n]))
    return np.array(out, F).reshape(-1, 12)


def extract(kind, nodes, grid_min, voxel, data=None, tris=None, tri_offset=None, planes=None, margin=50.0):
    """(tris (n, 12) float32, tri_node (n,) int32) of rto_extract_mesh(kind) on this octree."""
    parts, owner = [], []
    for i in visible_leaves(nodes, grid_min, voxel, planes, margin):
        if kind == MESH_MC:
            t = tris[tri_offset[i]:tri_offset[i + 1]]
        elif nodes["isSolid"][i] == 1:
            t = cube_faces(nodes[i], grid_min, voxel, data)
        else:
            continue
        if len(t):
            parts.append(np.asarray(t, F).reshape(-1, 12))
            owner.append(np.full(len(t), i, np.int32))
    if not parts:
        return np.zeros((0, 12), F), np.zeros(0, np.int32)
    return np.ascontiguousarray(np.concatenate(parts)), np.concatenate(owner)


def morton(x, y, z, bits=21):
    """Morton code with x in the lowest bit of every triple."""
    code = np.zeros(len(x), np.uint64)
    for b in range(bits):
        for a, v in enumerate((x, y, z)):
            code |= ((np.asarray(v, np.uint64) >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + a)
    return code
