"""Generates tests/golden/ref_dc.npz.  Run ONLY where /root/reference exists:

    python tests/golden/make_golden_dc.py

Expected vertices and lists: outputs of the REFERENCE'S OWN AdaptiveDualContouringRenderer functions
(453-skeleton/AdaptiveDualContouringRenderer.cpp: gatherHermiteData with size 1, calculateIntersection, generateDualVertex with
QEFSolver, and buildTrianglesCPU), compiled here from where they lie with the oracle's flags (g++ -O2 -ffp-contract=off
-fno-fast-math, the vendored glm 0.9.9.7, glad and glfw headers; no GL call runs).  The small main() below is made in a temporary
directory that is deleted afterwards; it fills a VoxelGrid, asks for the vertex of every voxel -- the centre handed to
generateDualVertex is gridToWorld(x, y, z) + vec3(0.5f * voxelSize) -- and hands the vertices to buildTrianglesCPU.  Nothing compiled
and no reference text is kept.

Before anything is written the maker asserts that tests/dc_ref.py (the rule in numpy float32) agrees with the reference byte for byte
on every vertex volume and on every list of the reference's area rule.  The reference has no RTO_DC_AREA_NONE: that case stores
dc_ref's list over the vertices just shown equal.  It counts how often each way through the vertex rule is taken over the fixture
and asserts at least one of each.  One way is taken by no input and cannot be: "a dominant axis but no aligned point".  A
Hermite normal is an axis, or a unit diagonal of two axes, so its dot with the snapped axis is 0, +-0.70710677 or +-1; the summed
normal points along +axis only if some normal has a positive component there, and that normal's dot is at least 0.70710677 > 0.7.
The census stores its count, asserted 0, and DESIGN.md section 32 names it as uncovered.

Stored: every grid once, as bits, with its dims, grid min and voxel size; per grid the SHA-256 of its vertex volume (16 bytes per
voxel: three float32 and the int32 number of Hermite points, x fastest) and the volume itself where it is at most 32 KiB; per case
its grid's name, the area rule, the triangle count, the triangles the area rule dropped, the SHA-256 of the (n, 12) float32 record
list, and the list itself where it is at most 16 KiB.
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
import dc_ref as dc  # noqa: E402

REF = "/root/reference"
SRC = os.path.join(REF, "453-skeleton")
GLM = os.path.join(REF, "thirdparty", "glm-0.9.9.7")
GLAD = os.path.join(REF, "thirdparty", "glad-opengl-4.6-core")
GLFW = os.path.join(REF, "thirdparty", "glfw-3.4", "include")
OUT = os.path.join(HERE, "ref_dc.npz")
FULL_LIST = 16384           # bytes: longer lists are stored as count + SHA-256 only
FULL_VERTS = 32768
SIZE_LIMIT = 100_000
VERTEX_DTYPE = np.dtype([("p", np.float32, 3), ("points", np.int32)])

MAIN = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "AdaptiveDualContouringRenderer.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    FILE* o = std::fopen(argv[2], "wb");
    if (!f || !o) return 3;
    int32_t d[3]; float m[4];
    if (std::fread(d, 4, 3, f) != 3 || std::fread(m, 4, 4, f) != 4) return 3;
    VoxelGrid grid;
    grid.dimX = d[0]; grid.dimY = d[1]; grid.dimZ = d[2];
    grid.minX = m[0]; grid.minY = m[1]; grid.minZ = m[2]; grid.voxelSize = m[3];
    std::vector<uint8_t> bytes((size_t)d[0] * d[1] * d[2]);
    if (std::fread(bytes.data(), 1, bytes.size(), f) != bytes.size()) return 3;
    grid.data.resize(bytes.size());
    for (size_t i = 0; i < bytes.size(); i++) grid.data[i] = bytes[i] ? VoxelState::FILLED : VoxelState::EMPTY;
    AdaptiveDualContouringRenderer r;
    std::vector<glm::vec4> verts(bytes.size());
    for (int z = 0; z < d[2]; z++)
        for (int y = 0; y < d[1]; y++)
            for (int x = 0; x < d[0]; x++) {
                std::vector<HermitePoint> points = r.gatherHermiteData(grid, x, y, z, 1);
                glm::vec3 centre = r.gridToWorld(grid, x, y, z) + glm::vec3(0.5f * grid.voxelSize);
                glm::vec3 v = r.generateDualVertex(points, centre, grid.voxelSize);
                verts[grid.index(x, y, z)] = glm::vec4(v, 0.0f);
                int32_t n = (int32_t)points.size();
                std::fwrite(&v[0], 4, 3, o);
                std::fwrite(&n, 4, 1, o);
            }
    std::vector<MCTriangle> tris = r.buildTrianglesCPU(grid, verts);
    int64_t n = (int64_t)tris.size();
    std::fwrite(&n, 8, 1, o);
    for (const MCTriangle& t : tris) {
        if (t.normal[0] != t.normal[1] || t.normal[0] != t.normal[2]) return 4;
        float rec[12];
        for (int v = 0; v < 3; v++) for (int a = 0; a < 3; a++) rec[3 * v + a] = t.v[v][a];
        for (int a = 0; a < 3; a++) rec[9 + a] = t.normal[0][a];
        std::fwrite(rec, 4, 12, o);
    }
    std::fclose(o);
    std::fclose(f);
    return 0;
}
"""


def build(tmp):
    with open(os.path.join(tmp, "main.cpp"), "w") as f:
        f.write(MAIN)
    exe = os.path.join(tmp, "dc")
    inc = [f"-I{SRC}", f"-I{GLM}", f"-I{GLAD}/include", f"-I{GLFW}"]
    flags = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-w"]
    objs = []
    for src in ("AdaptiveDualContouringRenderer.cpp", "OctreeVoxel.cpp", "Renderer.cpp"):
        obj = os.path.join(tmp, src.replace(".cpp", ".o"))
        subprocess.run(["g++", *flags, *inc, "-c", os.path.join(SRC, src), "-o", obj], check=True)
        objs.append(obj)
    glad = os.path.join(tmp, "glad.o")
    subprocess.run(["gcc", "-O1", "-w", f"-I{GLAD}/include", "-c", os.path.join(GLAD, "src", "glad.c"), "-o", glad], check=True)
    subprocess.run(["g++", *flags, *inc, os.path.join(tmp, "main.cpp"), *objs, glad, "-o", exe, "-ldl", "-lpthread"], check=True)
    return exe


def run_ref(exe, tmp, vox, gmin, vs):
    ip, op = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    dz, dy, dx = vox.shape
    with open(ip, "wb") as f:
        f.write(struct.pack("<3i", dx, dy, dz))
        f.write(np.asarray(gmin, np.float32).tobytes() + np.float32(vs).tobytes())
        f.write(np.ascontiguousarray(vox, np.uint8).tobytes())
    subprocess.run([exe, ip, op], check=True, stdout=subprocess.DEVNULL)
    b = open(op, "rb").read()
    nv = dx * dy * dz
    verts = np.frombuffer(b, VERTEX_DTYPE, nv, 0).copy().reshape(dz, dy, dx)
    n = struct.unpack_from("<q", b, 16 * nv)[0]
    assert len(b) == 16 * nv + 8 + 48 * n
    return verts, np.frombuffer(b, np.float32, n * 12, 16 * nv + 8).copy().reshape(n, 12)


# ---------------------------------------------------------------- grids: name -> (uint8 (dz, dy, dx), min, voxel size)
def noise(seed, shape, density=0.5):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def sphere16():
    z, y, x = np.indices((16, 16, 16)).astype(np.float64)
    return (((x - 7.5) ** 2 + (y - 7.5) ** 2 + (z - 7.5) ** 2) < 36).astype(np.uint8)


def rand12():
    """The first seed whose 12^3 grid at density 0.5 takes the rare way 'QEF accepted'."""
    unit = np.array([-0.5, -0.5, -0.5], np.float32)
    for seed in range(256):
        v = noise(seed, (12, 12, 12))
        _, _, branch = dc.vertices(v, unit, np.float32(1.0 / 12))
        if (branch == dc.B_QEF).any():
            return v
    raise AssertionError("no seed takes 'QEF accepted'")


def grids():
    unit = np.array([-0.5, -0.5, -0.5], np.float32)
    out = {}
    out["sphere16"] = (sphere16(), unit, np.float32(1.0 / 16))
    out["sphere16_fine"] = (sphere16(), unit, np.float32(1.0 / 512))
    out["rand12"] = (rand12(), unit, np.float32(1.0 / 12))
    out["sparse12"] = (noise(21, (12, 12, 12), 0.06), unit, np.float32(1.0 / 12))
    rng = np.random.default_rng(11)                    # make_golden_mesh.py's non-cubic grid
    d = np.zeros((7, 12, 20), np.uint8)
    d[0:4, 0:4, 0:4] = 1
    d[2:7, 4:12, 12:20] = 1
    d[4:6, 1:3, 8:10] = 1
    d |= (rng.random(d.shape) < 0.06).astype(np.uint8)
    out["noncubic"] = (d, np.array([-2125.0, -1215.0, -150.0], np.float32), np.float32(10.0))
    d = np.zeros((3, 3, 200), np.uint8)                # make_golden_mesh.py's long grid
    for x0 in (0, 1, 63, 64, 127, 128, 150, 199):
        d[x0 % 3, (x0 // 3) % 3, x0] = 1
    d[0:2, 0:2, 96:98] = 1
    out["long200"] = (d, np.array([-0.4, -0.01, -0.01], np.float32), np.float32(1.0 / 256))
    for k, seed in ((33, 5), (34, 6), (35, 7), (36, 8)):          # the halo reaches three voxels past a tile of 32 x 8 x 8
        out[f"edge{k}"] = (noise(seed, (k - 24, k - 24, k), 0.35), unit, np.float32(1.0 / k))
    out["thin1"] = (noise(9, (5, 5, 1)), unit, np.float32(0.2))
    out["tiny2"] = (noise(10, (2, 2, 2)), unit, np.float32(0.5))
    return out


def cases():
    """(name, grid, area rule)"""
    out = [(g, g, dc.AREA_REFERENCE) for g in ("sphere16", "sphere16_fine", "rand12", "sparse12", "noncubic", "long200", "edge33", "edge34",
                                               "edge35", "edge36", "thin1", "tiny2")]
    out.insert(2, ("sphere16_fine_all", "sphere16_fine", dc.AREA_NONE))
    return out


def main():
    if not os.path.isfile(os.path.join(SRC, "AdaptiveDualContouringRenderer.cpp")):
        sys.exit("the reference is not here: nothing to generate")
    z = {}
    gs = grids()
    census = np.zeros(6, np.int64)                     # the five ways, and 'dominant axis but no aligned point'
    ref_verts, ref_lists, mine = {}, {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        for name, (v, gmin, vs) in gs.items():
            ref_verts[name], ref_lists[name] = run_ref(exe, tmp, v, gmin, vs)
    for name, (v, gmin, vs) in gs.items():
        dz, dy, dx = v.shape
        z[f"bits_{name}"] = np.packbits(v.reshape(-1))
        z[f"dims_{name}"] = np.array([dx, dy, dz], np.int32)
        z[f"min_{name}"] = np.asarray(gmin, np.float32)
        z[f"vs_{name}"] = np.float32(vs)
        verts, points, branch, lone = dc.vertices(v, gmin, vs, with_dominant=True)
        got = np.zeros(v.shape, VERTEX_DTYPE)
        got["p"], got["points"] = verts, points
        want = ref_verts[name]
        assert got.tobytes() == want.tobytes(), (name, "vertices", int((got != want).sum()))
        mine[name] = (verts, points)
        for b in range(5):
            census[b] += int((branch == b).sum())
        census[5] += int(lone.sum())
        z[f"vsha_{name}"] = np.frombuffer(hashlib.sha256(want.tobytes()).digest(), np.uint8)
        if want.nbytes <= FULL_VERTS:
            z[f"verts_{name}"] = want
    names = list(dc.BRANCH_NAMES) + ["dominant axis but no aligned point"]
    for b, nm in enumerate(names):
        print(f"{nm}: {census[b]}")
        assert (census[b] > 0) == (b < 5), f"'{nm}': {census[b]}"
    z["census"] = census
    cs = cases()
    counts = np.zeros(len(cs), np.int64)
    dropped = np.zeros(len(cs), np.int64)
    sha = np.zeros((len(cs), 32), np.uint8)
    for ci, (name, g, rule) in enumerate(cs):
        v, gmin, vs = gs[g]
        tris, cell, summary = dc.extract(v, gmin, vs, rule, None, *mine[g])
        if rule == dc.AREA_REFERENCE:
            want = ref_lists[g]
            assert tris.tobytes() == want.tobytes(), (name, tris.shape, want.shape)
        else:
            want = tris
            assert len(want) == 2 * summary["faces"] and len(want) > len(ref_lists[g])
        counts[ci], dropped[ci] = len(want), summary["dropped"]
        sha[ci] = np.frombuffer(hashlib.sha256(want.tobytes()).digest(), np.uint8)
        if want.nbytes <= FULL_LIST:
            z[f"tris_{name}"] = want
        print(name, "triangles", len(want), "dropped", summary["dropped"], "degenerate", summary["degenerate"],
              "stored" if want.nbytes <= FULL_LIST else "")
    z["names"] = np.array([c[0] for c in cs])
    z["case_grid"] = np.array([c[1] for c in cs])
    z["area_rule"] = np.array([c[2] for c in cs], np.int32)
    z["counts"] = counts
    z["dropped"] = dropped
    z["sha256"] = sha
    np.savez_compressed(OUT, **z)
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    assert size < SIZE_LIMIT, size


if __name__ == "__main__":
    main()
