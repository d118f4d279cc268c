"""Generates tests/golden/ref_iso.npz.  Run ONLY where /root/reference exists:

    python tests/golden/make_golden_iso.py

Expected lists: outputs of the REFERENCE'S OWN marchingCubesVolume and marchingCubesCell (453-skeleton/MarchingCubes.cpp:544-689),
compiled here from where they lie with the oracle's flags (g++ -O2 -ffp-contract=off -fno-fast-math, the vendored glm 0.9.9.7).  The
small main() below is made in a temporary directory that is deleted afterwards; it #includes MarchingCubes.cpp, calls
marchingCubesVolume on a float field and, for padded and clipped cases, marchingCubesCell over the restated cell loop (z, y, x; the
corner positions origin + vec3(x, y, z) * spacing with the block's first index added).  It also dumps edgeTable and triTable.
Nothing compiled and no reference text is kept.

The float field handed over is the rule's substituted sample block (tests/iso_ref.py: samples): the reference knows no validity
window, pad ring or clip box.  Before anything is written the maker asserts that tests/iso_ref.py agrees byte for byte on every
vertex list, that marchingCubesVolume and the restated loop agree where both apply, and that the project's case table
(host/mc_cases.inc) equals the reference's two tables.

Stored: every volume once (int32, with its grid min and voxel size); per case its volume's name and a row of parameters (level,
outside, valid_lo, valid_hi, pad, clip flag, clip_lo, clip_hi), the count and the SHA-256 of the expected (n, 9) float32 vertex
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
sys.path.insert(0, os.path.dirname(TESTS))
import distance_ref as dr  # noqa: E402
import iso_ref as ir  # noqa: E402
from oracle import orc  # noqa: E402

REF = "/root/reference"
SRC = os.path.join(REF, "453-skeleton")
GLM = os.path.join(REF, "thirdparty", "glm-0.9.9.7")
OUT = os.path.join(HERE, "ref_iso.npz")
FULL_LIMIT = 16384          # bytes: longer lists are stored as count + SHA-256 only
SIZE_LIMIT = 100_000

MAIN = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "MarchingCubes.cpp"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 3;
    if (argv[1][0] == '-') {                       // the tables
        for (int i = 0; i < 256; i++) { int32_t e = edgeTable[i]; std::fwrite(&e, 4, 1, o); }
        for (int i = 0; i < 256; i++) for (int k = 0; k < 16; k++) { int32_t t = triTable[i][k]; std::fwrite(&t, 4, 1, o); }
        std::fclose(o);
        return 0;
    }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t mode, d[3], first[3]; float m[5];
    if (std::fread(&mode, 4, 1, f) != 1 || std::fread(d, 4, 3, f) != 3 || std::fread(first, 4, 3, f) != 3 || std::fread(m, 4, 5, f) != 5) return 3;
    std::vector<float> field((size_t)d[0] * d[1] * d[2]);
    if (std::fread(field.data(), 4, field.size(), f) != field.size()) return 3;
    const glm::vec3 origin(m[0], m[1], m[2]);
    const float spacing = m[3], iso = m[4];
    std::vector<MCTriangle> out;
    if (mode == 0) out = marchingCubesVolume(field.data(), d[0], d[1], d[2], origin, spacing, iso);
    else {
        auto val = [&](int x, int y, int z) { return field[(size_t)x + (size_t)y * d[0] + (size_t)z * d[0] * d[1]]; };
        const int off[8][3] = { {0,0,0}, {1,0,0}, {1,1,0}, {0,1,0}, {0,0,1}, {1,0,1}, {1,1,1}, {0,1,1} };
        for (int z = 0; z < d[2] - 1; z++)
            for (int y = 0; y < d[1] - 1; y++)
                for (int x = 0; x < d[0] - 1; x++) {
                    std::array<Corner, 8> corner = {};
                    for (int i = 0; i < 8; i++) {
                        corner[i].pos = origin + glm::vec3(x + off[i][0] + first[0], y + off[i][1] + first[1], z + off[i][2] + first[2]) * spacing;
                        corner[i].val = val(x + off[i][0], y + off[i][1], z + off[i][2]);
                    }
                    auto cell = marchingCubesCell(corner, iso);
                    out.insert(out.end(), cell.begin(), cell.end());
                }
    }
    int64_t n = (int64_t)out.size();
    std::fwrite(&n, 8, 1, o);
    for (const MCTriangle& t : out) {
        for (int v = 0; v < 3; v++) if (t.normal[v] != glm::vec3(0, 1, 0)) return 4;      // the placeholder
        float rec[9];
        for (int v = 0; v < 3; v++) for (int a = 0; a < 3; a++) rec[3 * v + a] = t.v[v][a];
        std::fwrite(rec, 4, 9, o);
    }
    std::fclose(o);
    std::fclose(f);
    return 0;
}
"""


def build(tmp):
    with open(os.path.join(tmp, "main.cpp"), "w") as f:
        f.write(MAIN)
    exe = os.path.join(tmp, "iso")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-w", f"-I{SRC}", f"-I{GLM}",
                    os.path.join(tmp, "main.cpp"), "-o", exe], check=True)
    return exe


def ref_tables(exe, tmp):
    op = os.path.join(tmp, "tables.bin")
    subprocess.run([exe, "-", op], check=True)
    t = np.fromfile(op, np.int32)
    return t[:256].copy(), t[256:].reshape(256, 16).copy()


def run_ref(exe, tmp, mode, S, first, origin, spacing, level):
    ip, op = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(ip, "wb") as f:
        f.write(struct.pack("<i", mode))
        f.write(struct.pack("<3i", S.shape[2], S.shape[1], S.shape[0]))
        f.write(struct.pack("<3i", *[int(v) for v in first]))
        f.write(np.asarray(origin, np.float32).tobytes() + np.float32(spacing).tobytes() + np.float32(level).tobytes())
        f.write(np.ascontiguousarray(S, np.float32).tobytes())
    subprocess.run([exe, ip, op], check=True)
    b = open(op, "rb").read()
    n = struct.unpack_from("<q", b, 0)[0]
    assert len(b) == 8 + 36 * n
    return np.frombuffer(b, np.float32, n * 9, 8).copy().reshape(n, 9)


# ---------------------------------------------------------------- volumes: name -> (int32 (dz, dy, dx), min, voxel size)
def noise(seed, shape, lo=0, hi=8):
    return np.random.default_rng(seed).integers(lo, hi, size=shape).astype(np.int32)


def noise12():
    """The first seed whose 12^3 volume of values 0..7, with a uniform 3^3 block of 0 and one of 7, shows all 256 cases at 3.5."""
    for seed in range(64):
        v = noise(seed, (12, 12, 12))
        v[1:4, 1:4, 1:4] = 0
        v[7:10, 6:9, 5:8] = 7
        case = ir.cells_of_samples(v.astype(np.float32), 3.5)
        if len(np.unique(case)) == 256:
            return v
    raise AssertionError("no seed shows all 256 cases")


def volumes():
    unit = np.array([-0.5, -0.5, -0.5], np.float32)
    out = {}
    g = orc.test_sphere_grid(16)
    out["sphere16"] = (dr.field(np.asarray(g.data, np.uint8).reshape(16, 16, 16), dr.SET_EMPTY), g.min, g.voxel_size)
    out["noise12"] = (noise12(), unit, np.float32(1.0 / 12))
    rng = np.random.default_rng(11)                    # make_golden_mesh.py's non-cubic grid
    d = np.zeros((7, 12, 20), np.uint8)
    d[0:4, 0:4, 0:4] = 1
    d[2:7, 4:12, 12:20] = 1
    d[4:6, 1:3, 8:10] = 1
    d |= (rng.random(d.shape) < 0.06).astype(np.uint8)
    out["noncubic"] = (dr.field(d, dr.SET_EMPTY), np.array([-2125.0, -1215.0, -150.0], np.float32), np.float32(10.0))
    d = np.zeros((3, 3, 200), np.uint8)                # make_golden_mesh.py's long grid; the distance to its solids
    for x0 in (0, 1, 63, 64, 127, 128, 150, 199):
        d[x0 % 3, (x0 // 3) % 3, x0] = 1
    d[0:2, 0:2, 96:98] = 1
    out["long200"] = (dr.field(d, dr.SET_SOLID), np.array([-0.4, -0.01, -0.01], np.float32), np.float32(1.0 / 256))
    out["edge33"] = (noise(5, (9, 9, 33)), unit, np.float32(1.0 / 33))
    out["edge34"] = (noise(6, (10, 10, 34)), unit, np.float32(1.0 / 34))
    out["thin1"] = (noise(7, (5, 5, 1)), unit, np.float32(0.2))
    out["tiny2"] = (noise(8, (2, 2, 2)), unit, np.float32(0.5))
    out["big24"] = ((1 << 24) + noise(9, (6, 7, 8), -3, 4), unit, np.float32(0.125))
    out["signed"] = (noise(10, (6, 7, 8), -5, 8), unit, np.float32(0.125))
    return out


def cases():
    """(name, volume, level, outside, valid, pad, clip)"""
    dflt = (0, 0x7ffffffe)
    out = []

    def both(name, vol, level, outside, valid=dflt, clip=None):
        for pad in (1, 0):
            out.append((f"{name}_{'pad' if pad else 'nopad'}", vol, level, outside, valid, pad, clip))

    for lv, tag in ((0.5, "l05"), (2.5, "l25"), (4.0, "l40")):
        both(f"sphere16_{tag}", "sphere16", lv, 0.0)
    both("sphere16_l25_clip", "sphere16", 2.5, 0.0, clip=((3, 2, 4), (13, 12, 11)))
    both("noise12_l35", "noise12", 3.5, 0.0)
    both("noise12_l30", "noise12", 3.0, 0.0)
    both("noncubic_l05", "noncubic", 0.5, 0.0)
    both("noncubic_l15", "noncubic", 1.5, 0.0)
    both("long200_l25", "long200", 2.5, 1.0e6)
    both("edge33_l35", "edge33", 3.5, 0.0)
    both("edge34_l35", "edge34", 3.5, 0.0)
    both("edge34_l35_clip", "edge34", 3.5, 9.0, clip=((1, 1, 1), (33, 9, 9)))
    both("thin1_l35", "thin1", 3.5, 0.0)
    both("tiny2_l35", "tiny2", 3.5, 0.0)
    both("big24_l", "big24", 16777218.0, 0.0)
    both("signed_l35", "signed", 3.5, 9.0, valid=(0, 7))
    both("signed_l15_window", "signed", 1.5, -2.0, valid=(-3, 5))
    return out


def main():
    if not os.path.isfile(os.path.join(SRC, "MarchingCubes.cpp")):
        sys.exit("the reference is not here: nothing to generate")
    z = {}
    vols = volumes()
    for name, (v, gmin, vs) in vols.items():
        z[f"vol_{name}"] = np.ascontiguousarray(v, np.int32)
        z[f"min_{name}"] = np.asarray(gmin, np.float32)
        z[f"vs_{name}"] = np.float32(vs)
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        edge_table, tri_table = ref_tables(exe, tmp)
        # the project's table against the reference's two
        assert (tri_table[:, 15] == -1).all()
        assert (tri_table[:, :15] == ir.TRI_EDGES).all(), "host/mc_cases.inc differs from the reference's triTable"
        used = np.array([sum(1 << e for e in set(row[row >= 0].tolist())) for row in ir.TRI_EDGES])
        assert (used == edge_table).all(), "the edges host/mc_cases.inc uses differ from the reference's edgeTable"
        cs = cases()
        params = np.zeros((len(cs), 12), np.float64)
        counts = np.zeros(len(cs), np.int64)
        sha = np.zeros((len(cs), 32), np.uint8)
        for ci, (name, vol, level, outside, valid, pad, clip) in enumerate(cs):
            v, gmin, vs = vols[vol]
            S, first = ir.samples(v, level, outside, valid, pad, clip)
            origin = np.asarray(gmin, np.float32) + np.float32(0.5) * np.float32(vs)
            want = run_ref(exe, tmp, 1, S, first, origin, vs, level)
            if not pad and clip is None:
                whole = run_ref(exe, tmp, 0, S, first, origin, vs, level)
                assert whole.tobytes() == want.tobytes(), (name, "marchingCubesVolume against the restated loop")
            got, cell, summary = ir.extract(v, gmin, vs, level, outside, valid, pad, clip)
            assert got[:, :9].tobytes() == want.tobytes(), (name, got.shape, want.shape)
            params[ci] = [np.float32(level), np.float32(outside), valid[0], valid[1], pad, 0 if clip is None else 1,
                          *(clip[0] if clip else (0, 0, 0)), *(clip[1] if clip else (0, 0, 0))]
            counts[ci] = len(want)
            sha[ci] = np.frombuffer(hashlib.sha256(want.tobytes()).digest(), np.uint8)
            if want.nbytes <= FULL_LIMIT:
                z[f"verts_{name}"] = want
            print(name, "triangles", len(want), "degenerate", summary["degenerate"], "stored" if want.nbytes <= FULL_LIMIT else "")
        z["names"] = np.array([c[0] for c in cs])
        z["case_volume"] = np.array([c[1] for c in cs])
        z["params"] = params
        z["counts"] = counts
        z["sha256"] = sha
    np.savez_compressed(OUT, **z)
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    assert size < SIZE_LIMIT, size


if __name__ == "__main__":
    main()
