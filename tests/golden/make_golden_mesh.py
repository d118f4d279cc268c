"""Generates tests/golden/ref_mesh_extract.npz.  Run ONLY where /root/reference exists:

    python tests/golden/make_golden_mesh.py

Expected lists: outputs of the REFERENCE'S OWN createOctreeFromVoxelGrid, Frustum::testAABB, MarchingCubesRenderer::render and
VoxelCubeRenderer::render (453-skeleton/OctreeVoxel.cpp, Frustum.cpp, Renderer.cpp), compiled here from where they lie with the
oracle's flags (g++ -O2 -ffp-contract=off -fno-fast-math, the vendored glm 0.9.9.7).  The small main() below is made in a temporary
directory that is deleted afterwards; it restates the walk of renderOctree (453-skeleton/main.cpp:153-189: test the node's box,
return when it is outside, render a leaf, else visit the children in order) over caller-supplied planes, checks that the three
normals of every MCTriangle are bitwise equal and writes v0, v1, v2, normal[0].  Nothing compiled and no reference text is kept.

Cases: the 16^3 and 32^3 test shell spheres; a non-cubic 20 x 12 x 7 grid at sceneCache.bin's origin and voxel size (faces at the
dims' edge, test voxels outside the grid, large empty leaves); a 16^3 grid with a solid 8^3 leaf whose +X face centre is covered
by one voxel, and the same with that voxel off-centre; an 8^3 checkerboard (every leaf of size 1); all-FILLED and all-EMPTY 8^3; a
200 x 3 x 3 grid (root 256).  Plane sets: none; the test camera's planes at margins 50, 0 and one voxel; a closer camera at margin
0; four seeded sets of random unit planes through the grid's interior at margin 0; one set that culls the root.  Stored per case:
dims, min, voxel size, packed grid, the plane sets and margins, and per set and kind the count and SHA-256 of the expected (n, 12)
float32 list, plus the list itself where it is small.
"""
from __future__ import annotations

import hashlib
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.dirname(TESTS))
import mesh_ref as mr  # noqa: E402
from oracle import orc  # noqa: E402

REF = "/root/reference"
SRC = os.path.join(REF, "453-skeleton")
GLM = os.path.join(REF, "thirdparty", "glm-0.9.9.7")
OUT = os.path.join(HERE, "ref_mesh_extract.npz")
FULL_LIMIT = 16384          # bytes: longer lists are stored as count + SHA-256 only
ASPECT = 4.0 / 3.0
SPHERE_CAM = (0.5, 0.7, 1.8)
CLOSE_CAM = (0.5, 0.7, 0.9)

MAIN = r"""
#include <array>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include <glm/glm.hpp>
#define private public
#include "Frustum.h"
#undef private
#include "OctreeVoxel.h"
#include "Renderer.h"

static void visit(const OctreeNode* node, const VoxelGrid& g, Renderer& r, const Frustum* fr, float margin, std::vector<MCTriangle>& out) {
    if (!node) return;
    if (fr) {
        float vs = g.voxelSize;
        glm::vec3 lo(g.minX + node->x * vs, g.minY + node->y * vs, g.minZ + node->z * vs);
        glm::vec3 hi = lo + glm::vec3(node->size * vs);
        if (fr->testAABB(lo, hi, margin) == -1) return;
    }
    if (node->isLeaf) {
        std::vector<MCTriangle> t = r.render(node, g, node->x, node->y, node->z, node->size);
        out.insert(out.end(), t.begin(), t.end());
        return;
    }
    for (const OctreeNode* c : node->children) visit(c, g, r, fr, margin, out);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    VoxelGrid g;
    int32_t d[3]; float m[4]; int32_t sets = 0;
    if (std::fread(d, 4, 3, f) != 3 || std::fread(m, 4, 4, f) != 4) return 3;
    g.dimX = d[0]; g.dimY = d[1]; g.dimZ = d[2]; g.minX = m[0]; g.minY = m[1]; g.minZ = m[2]; g.voxelSize = m[3];
    std::vector<uint8_t> bytes((size_t)d[0] * d[1] * d[2]);
    if (std::fread(bytes.data(), 1, bytes.size(), f) != bytes.size()) return 3;
    g.data.resize(bytes.size());
    for (size_t i = 0; i < bytes.size(); i++) g.data[i] = bytes[i] ? VoxelState::FILLED : VoxelState::EMPTY;
    if (std::fread(&sets, 4, 1, f) != 1) return 3;
    OctreeNode* root = createOctreeFromVoxelGrid(g);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 3;
    for (int s = 0; s < sets; s++) {
        int32_t has; float pl[24], margin;
        if (std::fread(&has, 4, 1, f) != 1 || std::fread(pl, 4, 24, f) != 24 || std::fread(&margin, 4, 1, f) != 1) return 3;
        Frustum fr(glm::mat4(1.0f));
        for (int i = 0; i < 6; i++) fr.m_planes[i] = glm::vec4(pl[4 * i], pl[4 * i + 1], pl[4 * i + 2], pl[4 * i + 3]);
        for (int kind = 0; kind < 2; kind++) {
            MarchingCubesRenderer mc; VoxelCubeRenderer vc;
            Renderer& r = kind == 0 ? static_cast<Renderer&>(mc) : static_cast<Renderer&>(vc);
            std::vector<MCTriangle> out;
            visit(root, g, r, has ? &fr : nullptr, margin, out);
            int64_t n = (int64_t)out.size();
            std::fwrite(&n, 8, 1, o);
            for (const MCTriangle& t : out) {
                if (std::memcmp(&t.normal[0], &t.normal[1], 12) || std::memcmp(&t.normal[0], &t.normal[2], 12)) return 4;
                float rec[12];
                for (int v = 0; v < 3; v++) for (int a = 0; a < 3; a++) rec[3 * v + a] = t.v[v][a];
                for (int a = 0; a < 3; a++) rec[9 + a] = t.normal[0][a];
                std::fwrite(rec, 4, 12, o);
            }
        }
    }
    std::fclose(o);
    std::fclose(f);
    if (root) freeOctree(root);
    return 0;
}
"""


def build(tmp):
    with open(os.path.join(tmp, "main.cpp"), "w") as f:
        f.write(MAIN)
    exe = os.path.join(tmp, "mesh")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-w", f"-I{SRC}", f"-I{GLM}",
                    os.path.join(tmp, "main.cpp"), os.path.join(SRC, "OctreeVoxel.cpp"), os.path.join(SRC, "Renderer.cpp"),
                    os.path.join(SRC, "Frustum.cpp"), "-o", exe], check=True)
    return exe


def run_ref(exe, tmp, dims, gmin, vs, data, sets):
    """sets: [(planes (24,) or None, margin)] -> [[mc (n, 12), cubes (n, 12)] per set]."""
    ip, op = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(ip, "wb") as f:
        f.write(struct.pack("<3i", *dims))
        f.write(np.asarray(gmin, np.float32).tobytes() + np.float32(vs).tobytes())
        f.write(np.ascontiguousarray(data, np.uint8).tobytes())
        f.write(struct.pack("<i", len(sets)))
        for planes, margin in sets:
            f.write(struct.pack("<i", 0 if planes is None else 1))
            f.write((np.zeros(24, np.float32) if planes is None else np.asarray(planes, np.float32)).tobytes())
            f.write(np.float32(margin).tobytes())
    subprocess.run([exe, ip, op], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    b = open(op, "rb").read()
    out, pos = [], 0
    for _ in sets:
        pair = []
        for _kind in range(2):
            n = struct.unpack_from("<q", b, pos)[0]
            pos += 8
            pair.append(np.frombuffer(b, np.float32, n * 12, pos).copy().reshape(n, 12))
            pos += n * 48
        out.append(pair)
    assert pos == len(b)
    return out


# ---------------------------------------------------------------- grids: (name, data (dz, dy, dx) uint8, min, voxel, unit scale)
def grids():
    out = []
    for dim in (16, 32):
        g = orc.test_sphere_grid(dim)
        out.append((f"sphere{dim}", np.ascontiguousarray(g.data, np.uint8).reshape(dim, dim, dim), g.min, g.voxel_size, True))
    rng = np.random.default_rng(11)
    d = np.zeros((7, 12, 20), np.uint8)
    d[0:4, 0:4, 0:4] = 1                   # an aligned solid 4^3 leaf in the corner
    d[2:7, 4:12, 12:20] = 1                # a block against three of the dims' edges (cut by dimZ = 7)
    d[4:6, 1:3, 8:10] = 1
    d |= (rng.random(d.shape) < 0.06).astype(np.uint8)
    out.append(("noncubic", d, np.array([-2125.0, -1215.0, -150.0], np.float32), np.float32(10.0), False))
    for name, extra in (("centre_covered", (4, 4, 8)), ("centre_open", (4, 5, 8))):
        d = np.zeros((16, 16, 16), np.uint8)
        d[0:8, 0:8, 0:8] = 1
        d[extra] = 1                        # (z, y, x): the +X face's test voxel is (8, 4, 4)
        out.append((name, d, np.array([-0.5, -0.5, -0.5], np.float32), np.float32(1.0 / 16), True))
    z, y, x = np.indices((8, 8, 8))
    out.append(("checker8", ((x + y + z) & 1).astype(np.uint8), np.array([-0.5, -0.5, -0.5], np.float32), np.float32(0.125), True))
    out.append(("full8", np.ones((8, 8, 8), np.uint8), np.array([-0.5, -0.5, -0.5], np.float32), np.float32(0.125), True))
    out.append(("empty8", np.zeros((8, 8, 8), np.uint8), np.array([-0.5, -0.5, -0.5], np.float32), np.float32(0.125), True))
    d = np.zeros((3, 3, 200), np.uint8)
    for x0 in (0, 1, 63, 64, 127, 128, 150, 199):
        d[x0 % 3, (x0 // 3) % 3, x0] = 1
    d[0:2, 0:2, 96:98] = 1
    out.append(("long200", d, np.array([-0.4, -0.01, -0.01], np.float32), np.float32(1.0 / 256), True))
    return out


def camera_planes(theta, phi, radius, target=None):
    cam = orc.Camera(theta, phi, radius)
    if target is not None:
        cam.set_target(*target)
    vp = orc.mat4_mul(orc.perspective(orc.radians(45.0), ASPECT, 0.01, 5000.0), cam.get_view())
    return orc.frustum_planes(vp)


def random_planes(seed, lo, hi):
    """Six unit planes through points of the grid's interior, each turned so that the grid's centre is in front of it."""
    rng = np.random.default_rng(seed)
    centre = 0.5 * (lo + hi)
    pl = np.zeros((6, 4), np.float64)
    for i in range(6):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        p = lo + rng.random(3) * (hi - lo)
        if np.dot(n, centre - p) < 0:
            n = -n
        pl[i, :3] = n
        pl[i, 3] = -np.dot(n, p)
    pl = pl.astype(np.float32)
    return pl.reshape(24)


def root_cull_planes(hi):
    pl = np.zeros((6, 4), np.float32)
    pl[:, 2] = 1.0
    pl[:, 3] = 1e9                                         # in front of everything
    pl[0] = (1.0, 0.0, 0.0, -(float(hi[0]) + 1000.0))      # the whole grid behind the first plane
    return pl.reshape(24)


def plane_sets(name, data, gmin, vs, unit, seeds):
    dz, dy, dx = data.shape
    lo = np.asarray(gmin, np.float64)
    hi = lo + np.array([dx, dy, dz], np.float64) * float(vs)
    if unit:
        cam, close = camera_planes(*SPHERE_CAM), camera_planes(*CLOSE_CAM)
    else:                                                  # the orbit camera aimed at the grid's centre
        c = 0.5 * (lo + hi)
        cam, close = camera_planes(0.6, 0.5, 600.0, c), camera_planes(0.6, 0.5, 150.0, c)
    sets = [("none", None, 50.0), ("cam_m50", cam, 50.0), ("cam_m0", cam, 0.0), ("cam_mvox", cam, float(vs)), ("close_m0", close, 0.0)]
    sets += [(f"rand{s}", random_planes(s, lo, hi), 0.0) for s in seeds]
    sets.append(("rootcull", root_cull_planes(hi), 0.0))
    return sets


def pick_seeds(exe, tmp):
    """Four seeds of which at least two cull more than 10 % and less than 90 % of the 16^3 sphere's triangles (both kinds)."""
    name, data, gmin, vs, unit = grids()[0]
    dims = (data.shape[2], data.shape[1], data.shape[0])
    lo = np.asarray(gmin, np.float64)
    hi = lo + np.array(dims, np.float64) * float(vs)
    full = run_ref(exe, tmp, dims, gmin, vs, data, [(None, 0.0)])[0]
    cand = list(range(1, 33))
    res = run_ref(exe, tmp, dims, gmin, vs, data, [(random_planes(s, lo, hi), 0.0) for s in cand])
    partial = [s for s, r in zip(cand, res) if all(0.1 * len(f) < len(f) - len(g) < 0.9 * len(f) for f, g in zip(full, r))]
    assert len(partial) >= 2, partial
    rest = [s for s in cand if s not in partial[:3]]
    return partial[:3] + rest[:1]


def main():
    if not os.path.isfile(os.path.join(SRC, "Renderer.cpp")):
        sys.exit("the reference is not here: nothing to generate")
    z = {}
    names = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        seeds = pick_seeds(exe, tmp)
        z["seeds"] = np.array(seeds, np.int32)
        for name, data, gmin, vs, unit in grids():
            dims = (data.shape[2], data.shape[1], data.shape[0])
            sets = plane_sets(name, data, gmin, vs, unit, seeds)
            res = run_ref(exe, tmp, dims, gmin, vs, data, [(p, m) for _, p, m in sets])
            names.append(name)
            z[f"{name}_dims"] = np.array(dims, np.int32)
            z[f"{name}_min"] = np.asarray(gmin, np.float32)
            z[f"{name}_vs"] = np.float32(vs)
            z[f"{name}_packed"] = np.packbits(data.reshape(-1))
            z[f"{name}_sets"] = np.array([s[0] for s in sets])
            z[f"{name}_has_planes"] = np.array([s[1] is not None for s in sets])
            z[f"{name}_planes"] = np.stack([np.zeros(24, np.float32) if s[1] is None else np.asarray(s[1], np.float32) for s in sets])
            z[f"{name}_margins"] = np.array([s[2] for s in sets], np.float32)
            counts = np.zeros((len(sets), 2), np.int64)
            sha = np.zeros((len(sets), 2, 32), np.uint8)
            # the numpy statement of the rule must agree before anything is written
            g = orc.Grid(dims, np.asarray(gmin, np.float32), np.float32(vs), data)
            nodes = orc.build_flat_octree(g)
            tris, off = orc.build_leaf_triangles(g, nodes)
            for si, ((sname, planes, margin), pair) in enumerate(zip(sets, res)):
                for kind, want in enumerate(pair):
                    got, _ = mr.extract(kind, nodes, gmin, vs, data=data, tris=tris, tri_offset=off, planes=planes, margin=margin)
                    assert got.tobytes() == want.tobytes(), (name, sname, kind, got.shape, want.shape)
                    counts[si, kind] = len(want)
                    sha[si, kind] = np.frombuffer(hashlib.sha256(want.tobytes()).digest(), np.uint8)
                    if name != "sphere32" and want.nbytes <= FULL_LIMIT:
                        z[f"{name}_{sname}_{'mc' if kind == 0 else 'cubes'}"] = want
            z[f"{name}_counts"] = counts
            z[f"{name}_sha256"] = sha
            print(name, dims, "nodes", len(nodes), "counts", counts.tolist())
            if name == "sphere16":                         # the condition on the random sets, on the reference's own lists
                full = counts[0]
                part = [si for si, s in enumerate(sets) if s[0].startswith("rand")
                        and all(0.1 * full[k] < full[k] - counts[si, k] < 0.9 * full[k] for k in range(2))]
                assert len(part) >= 2, counts
            if unit and name not in ("empty8",):           # margin 50 on a unit-scale scene culls nothing
                assert (counts[1] == counts[0]).all(), (name, counts)
            if name == "full8":
                assert counts[0, 1] == 12
            if name == "centre_covered":
                assert not any((t[9] == 1.0 and t[0] == t[3] == t[6] == np.float32(0.0)) for t in res[0][1]), "the covered +X face is there"
    z["names"] = np.array(names)
    np.savez_compressed(OUT, **z)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
