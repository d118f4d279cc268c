"""Generates tests/golden/ref_voxelize.npz.  Run ONLY where /root/reference exists:

    python tests/golden/make_golden_voxelize.py

ref_* vectors: outputs of the REFERENCE'S OWN loadCSVDataIntoVoxelGrid (453-skeleton/BuildingLoader.cpp:153-290), compiled
here from where it lies with the oracle's flags (g++ -O2 -ffp-contract=off -fno-fast-math, the vendored glm 0.9.9.7, no OpenMP:
the grid is an OR over faces, so the order does not matter).  Two things stand between that file and a compiler, and both are
made in a temporary directory that is deleted afterwards: its `#include "buildingloader.h"` (the file is BuildingLoader.h) is
answered by a one-line header that includes the real one, and a small main() #includes BuildingLoader.cpp, reads the two CSV
files it is given and writes the grid (dims, float min, voxelSize, bytes).  Nothing compiled and no reference text is kept.

Meshes (deterministic): two extruded blocks at UTM magnitudes at voxel 10, 3.7 and 1.3; a unit-scale UV sphere at voxel 1/64
(the 1e-7f degenerate cut rejects its polar faces); a triangle soup with degenerate and collinear faces, repeated vertices,
duplicate keys, faces naming missing vertices, several mesh numbers and unused far-away rows; one ground triangle spanning the
grid; extents giving a dim in 1001..1999 (scale 1) and above 2000 (voxelSize doubled); CSV text with blank lines, padded
tokens, short rows and unparsable numbers.  Stored per case: the CSV text, the voxel size asked for, the rows and faces as the
host layer resolves them, and the reference's dims, min, voxelSize and packed grid.
"""
from __future__ import annotations

import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import voxelize_ref as vr  # noqa: E402

REF = "/root/reference"
SRC = os.path.join(REF, "453-skeleton")
GLM = os.path.join(REF, "thirdparty", "glm-0.9.9.7")
OUT = os.path.join(HERE, "ref_voxelize.npz")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <limits>
#include "BuildingLoader.cpp"
int main(int argc, char** argv) {
    if (argc != 5) return 2;
    VoxelGrid g = loadCSVDataIntoVoxelGrid(argv[1], argv[2], (float)std::strtod(argv[3], nullptr));
    FILE* f = std::fopen(argv[4], "wb");
    if (!f) return 3;
    int32_t d[3] = { g.dimX, g.dimY, g.dimZ };
    float m[4] = { g.minX, g.minY, g.minZ, g.voxelSize };
    std::fwrite(d, 4, 3, f);
    std::fwrite(m, 4, 4, f);
    std::fwrite(g.data.data(), 1, g.data.size(), f);
    std::fclose(f);
    return 0;
}
"""


def build(tmp):
    with open(os.path.join(tmp, "buildingloader.h"), "w") as f:
        f.write('#include "BuildingLoader.h"\n')
    with open(os.path.join(tmp, "main.cpp"), "w") as f:
        f.write(MAIN)
    exe = os.path.join(tmp, "vox")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-w", "-include", "limits", "-include", "cmath",
                    f"-I{tmp}", f"-I{SRC}", f"-I{GLM}", os.path.join(tmp, "main.cpp"), os.path.join(SRC, "OctreeVoxel.cpp"),
                    os.path.join(SRC, "Renderer.cpp"), "-o", exe], check=True)
    return exe


def run_ref(exe, tmp, verts_csv, faces_csv, voxel):
    vp, fp, op = (os.path.join(tmp, n) for n in ("v.csv", "f.csv", "out.bin"))
    with open(vp, "w") as f:
        f.write(verts_csv)
    with open(fp, "w") as f:
        f.write(faces_csv)
    subprocess.run([exe, vp, fp, repr(float(voxel)), op], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    b = open(op, "rb").read()
    dims = np.frombuffer(b[:12], np.int32).copy()
    mv = np.frombuffer(b[12:28], np.float32).copy()
    data = np.frombuffer(b[28:], np.uint8).copy()
    assert len(data) == int(np.prod(dims.astype(np.int64))), (dims, len(data))
    return dims, mv[:3], mv[3], data


# ---------------------------------------------------------------- meshes: (rows [(mesh, vnum, x, y, z)], faces [(mesh, a, b, c)])
def to_csv(rows, faces):
    v = "MeshNumber,VertexNumber,Easting,Northing,Elevation,Latitude,Longitude,ElevMin\n"
    v += "".join(f"{m},{n},{x!r},{y!r},{z!r},51.04,-114.06,0.0\n" for m, n, x, y, z in rows)
    f = "MeshNumber,V1,V2,V3\n" + "".join(f"{m},{a},{b},{c}\n" for m, a, b, c in faces)
    return v, f


def box_mesh(mesh, base_vnum, corners_xy, z0, z1):
    """An extruded quad footprint (4 corners, counter-clockwise): 8 rows, 12 faces."""
    rows = [(mesh, base_vnum + i, float(x), float(y), float(z0)) for i, (x, y) in enumerate(corners_xy)]
    rows += [(mesh, base_vnum + 4 + i, float(x), float(y), float(z1)) for i, (x, y) in enumerate(corners_xy)]
    q = base_vnum
    faces = [(mesh, q, q + 2, q + 1), (mesh, q, q + 3, q + 2), (mesh, q + 4, q + 5, q + 6), (mesh, q + 4, q + 6, q + 7)]
    for i in range(4):
        j = (i + 1) % 4
        faces += [(mesh, q + i, q + j, q + 4 + j), (mesh, q + i, q + 4 + j, q + 4 + i)]
    return rows, faces


def utm_blocks():
    ex, ny = 700123.37, 5661234.81
    c, s = np.cos(0.37), np.sin(0.37)
    fp1 = [(ex + c * u - s * v, ny + s * u + c * v) for u, v in ((0, 0), (31.3, 0), (31.3, 22.7), (0, 22.7))]
    fp2 = [(ex + 45.1 + x, ny + 12.9 + y) for x, y in ((0, 0), (18.4, 0), (18.4, 27.2), (0, 27.2))]
    r1, f1 = box_mesh(1, 1, fp1, 1045.2, 1083.9)
    r2, f2 = box_mesh(2, 1, fp2, 1046.05, 1101.35)
    return r1 + r2, f1 + f2


def uv_sphere(nlat=32, nlon=64, r=0.45):
    rows, faces = [(1, 0, 0.0, 0.0, r)], []
    for i in range(1, nlat):
        th = np.pi * i / nlat
        for j in range(nlon):
            ph = 2 * np.pi * j / nlon
            rows.append((1, 1 + (i - 1) * nlon + j, float(r * np.sin(th) * np.cos(ph)), float(r * np.sin(th) * np.sin(ph)), float(r * np.cos(th))))
    south = 1 + (nlat - 1) * nlon
    rows.append((1, south, 0.0, 0.0, -r))
    vid = lambda i, j: 1 + (i - 1) * nlon + (j % nlon)           # noqa: E731
    for j in range(nlon):
        faces.append((1, 0, vid(1, j), vid(1, j + 1)))
        faces.append((1, south, vid(nlat - 1, j + 1), vid(nlat - 1, j)))
    for i in range(1, nlat - 1):
        for j in range(nlon):
            faces.append((1, vid(i, j), vid(i + 1, j), vid(i + 1, j + 1)))
            faces.append((1, vid(i, j), vid(i + 1, j + 1), vid(i, j + 1)))
    return rows, faces


def soup(seed=7):
    rng = np.random.default_rng(seed)
    rows, faces = [], []
    for mesh in (3, 5, 9):
        pts = rng.uniform([0, 0, 0], [20, 15, 10], size=(30, 3)).round(3)
        for k, p in enumerate(pts):
            rows.append((mesh, k, *map(float, p)))
        for _ in range(40):
            a, b, c = rng.integers(0, 30, 3)
            faces.append((mesh, int(a), int(b), int(c)))
        faces += [(mesh, 1, 1, 2), (mesh, 4, 4, 4)]               # degenerate: repeated vertices
        rows += [(mesh, 100, 1.0, 1.0, 1.0), (mesh, 101, 3.0, 2.0, 1.5), (mesh, 102, 7.0, 5.0, 3.0)]   # collinear
        faces.append((mesh, 100, 101, 102))
        faces += [(mesh, 5, 6, 999), (mesh, 998, 2, 3)]             # missing vertex numbers
        faces.append((77, 1, 2, 3))                                 # missing mesh
    rows.append((3, 7, 18.5, 2.25, 9.75))                          # duplicate key: the last row wins
    rows.append((5, 0, 0.5, 14.5, 0.25))
    rows += [(11, 0, -31.0, 40.0, -12.0), (11, 1, 52.0, -25.0, 30.0)]   # unused far-away rows: they set the bounds
    return rows, faces


def ground():
    rows = [(1, 1, 0.0, 0.0, 0.0), (1, 2, 120.0, 3.0, 4.5), (1, 3, 10.0, 90.0, 2.0)]
    return rows, [(1, 1, 2, 3)]


def strip(length):
    rows = [(1, 1, 0.0, 0.0, 0.0), (1, 2, float(length), 0.0, 0.0), (1, 3, float(length), 1.0, 0.5), (1, 4, 0.0, 1.0, 0.5)]
    return rows, [(1, 1, 2, 3), (1, 1, 3, 4)]


def messy_csv():
    rows, faces = box_mesh(4, 10, [(0, 0), (6.5, 0), (6.5, 4.25), (0, 4.25)], 0.0, 5.5)
    v, f = to_csv(rows, faces)
    vl, fl = v.split("\n"), f.split("\n")
    vl.insert(3, "")                                               # blank line
    vl.insert(5, "4,99,1.0,2.0")                                   # short row
    vl.insert(6, "4,abc,1.0,2.0,3.0,0,0,0")                        # unparsable vertex number
    vl.insert(7, "4,50,x1.0,2.0,3.0,0,0,0")                        # unparsable coordinate
    vl.insert(8, "   4 ,  51 ,  3.25 ,\t1.5 , 2.0 ,0,0,0  ")       # padded tokens: an unused row inside the bounds
    vl.insert(9, "4,52,1e1,2.5e0,-3.0,0,0,0,extra,tokens")         # more tokens than needed: used for the bounds
    fl.insert(2, "")
    fl.insert(3, "4,10,11")                                        # short face row
    fl.insert(4, "4, 10 ,x,12")                                    # unparsable face
    fl.insert(5, "  4 , 10 , 52 , 12 ")                            # padded face using the extra row
    return "\n".join(vl), "\n".join(fl)


def cases():
    out = []
    b = to_csv(*utm_blocks())
    for vox, tag in ((10.0, "10"), (3.7, "3p7"), (1.3, "1p3")):
        out.append((f"utm_blocks_{tag}", *b, vox))
    out.append(("uv_sphere", *to_csv(*uv_sphere()), 1.0 / 64))
    out.append(("soup", *to_csv(*soup()), 1.0))
    out.append(("ground", *to_csv(*ground()), 1.0))
    out.append(("dim1500", *to_csv(*strip(1495.0)), 1.0))
    out.append(("dim2500", *to_csv(*strip(2500.0)), 1.0))
    out.append(("messy_csv", *messy_csv(), 0.5))
    return out


def main():
    if not os.path.isfile(os.path.join(SRC, "BuildingLoader.cpp")):
        sys.exit("the reference is not here: nothing to generate")
    z = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        for name, vcsv, fcsv, vox in cases():
            dims, gmin, vs, data = run_ref(exe, tmp, vcsv, fcsv, vox)
            xyz, tris, _ = vr.parse_csv_mesh(vcsv, fcsv)
            want = vr.voxelize(xyz, tris, vox)
            assert want is not None and tuple(want[1]) == tuple(dims) and want[2].tobytes() == gmin.tobytes(), name
            assert np.float32(want[3]).tobytes() == np.float32(vs).tobytes() and np.array_equal(want[0].reshape(-1), data), name
            z[f"{name}_verts_csv"] = np.frombuffer(vcsv.encode(), np.uint8)
            z[f"{name}_faces_csv"] = np.frombuffer(fcsv.encode(), np.uint8)
            z[f"{name}_voxel"] = np.float32(vox)
            z[f"{name}_xyz"] = xyz
            z[f"{name}_tris"] = tris
            z[f"{name}_dims"] = dims
            z[f"{name}_min"] = gmin
            z[f"{name}_vs"] = np.float32(vs)
            z[f"{name}_packed"] = np.packbits(data)
            print(f"{name}: dims {tuple(dims)} vs {vs!r} filled {int(data.sum())} of {len(data)}")
    z["names"] = np.array([c[0] for c in cases()])
    np.savez_compressed(OUT, **z)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
