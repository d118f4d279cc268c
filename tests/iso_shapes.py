"""The launch geometry of the isosurface kernels (csrc/rto_iso.inc), as code: which tiles a call launches and
where the first one starts, which of them k_iso_count skips, how many blocks and rounds the scans take, and how the emit pass is
launched.  Plain functions: no GPU, no import of the library; tests/iso_ref.py supplies the triangles.  Each line restates one line
of iso_extract or of a kernel and names it; a mirror can drift, so the table is re-read when a launch line of rto_iso.inc changes.

dims is (dimX, dimY, dimZ); a volume has shape dims[::-1]; a clip box is ((x0, y0, z0), (x1, y1, z1)), None for the whole grid.

The second half holds the inputs of tests/test_iso_shapes.py (seeded numpy, no fixture file) and the list of calls made on them."""
from __future__ import annotations

import itertools
from collections import namedtuple

import numpy as np

import iso_ref as ir

F = np.float32
TILE = (32, 8, 8)             # kIsoTileX, kIsoTileY, kIsoTileZ
BLOCK = 256                   # kBlock
WAVE = 64                     # kWave
RUNS_PER_BLOCK = 8 * BLOCK    # kIsoRunsPerBlock
SCAN = 1024                   # k_iso_scan_sums: block sums a round
VALID = (0, 0x7ffffffe)       # the default window
AXES = "xyz"
SCAN_TEST = "test_gpu_more_than_2_to_the_23_active_runs"      # tests/test_isosurface.py: the call of 4,107 block sums

_PER_AXIS = {
    "iso:t0-%s==0": ("iso_extract: A.t0[a] = uLo[a] / tile[a] == 0", "a box that starts in the first tile: no clip box"),
    "iso:t0-%s>=1": ("iso_extract: A.t0[a] >= 1; k_iso_count: u0 = (t0 + b) * tile; k_iso_place: ux = (t0[0] + rx) * 32 + lane", "clip_lo = 32 (x), 8 (y, z) under pad"),
    "iso:first-tile-%s:whole": ("k_iso_count: uLo[a] % tile == 0, inXY / rowY / rowZ hold from the tile's first cell", "clip_lo = 32 (x), 8 (y, z) under pad"),
    "iso:first-tile-%s:partial": ("k_iso_count: uLo[a] % tile != 0, the cells before uLo get case 0 and no run", "no clip box under pad: uLo = 0 is whole, so clip_lo = 1"),
    "iso:last-tile-%s:whole": ("k_iso_count: uHi[a] % tile == 0", "clip_hi = 31 (x), 7 (y, z) under pad"),
    "iso:last-tile-%s:partial": ("k_iso_count: uHi[a] % tile != 0, the cells from uHi on get case 0 and no run", "clip_hi = 2"),
    "iso:tiles-%s==1": ("iso_extract: tiles[a] = ceil(uHi / tile) - t0 == 1", "1 x 1 x 1 under pad"),
    "iso:tiles-%s>=2": ("iso_extract: tiles[a] >= 2; along x: A.runsX >= 2, iso_run's bx and k_iso_place's run % runsX", "33 cells along x, 9 along y or z"),
}

# class -> (the condition in the source, the smallest input that takes it)
TABLE = {
    "iso:box-without-a-cell": ("iso_extract: cells[a] <= 0 on an axis, no kernel runs and the three times are -1", "a clip box one sample thick, without pad"),
    **{k % n: v for k, v in _PER_AXIS.items() for n in AXES},
    "iso_bricks:runs-x==1": ("iso_extract: runsB = (nbx + 7) / 8 == 1", "1 x 1 x 1"),
    "iso_bricks:runs-x>=2": ("k_iso_bricks: rx = w % runsX, row = w / runsX with runsX >= 2, dimX above 64", "65 x 1 x 1"),
    **{f"iso_bricks:brick-partial-{n}": (f"k_iso_bricks: dim{n.upper()} % 8 != 0: " + ("x < A.dimX fails in the last brick's lanes, bx < A.nbx in the run's last groups" if n == "x" else
                                                                                             f"{n}1 = min(b{n} * 8 + 8, dim) cuts the last brick"), "1 x 1 x 1") for n in AXES},
    "iso_bricks:last-block-short": ("k_iso_bricks: w >= waves in the last workgroup, waves % 4 != 0", "1 x 1 x 1"),
    "iso_bricks:last-block-whole": ("k_iso_bricks: waves % 4 == 0", "1 x 32 x 1"),
    "iso_count:tile-staged": ("k_iso_count: the level lies in the tile's range, or the table is off", "1 x 1 x 1 of 7 at 3.5, outside 0, pad"),
    "iso_count:tile-staged:t0>=1": ("the same in a call with some t0[a] >= 1", "a clip box from 32 (x) or 8 (y, z) under pad"),
    "iso_count:tile-skipped": ("k_iso_count: mn >= A.level || mx < A.level, zero counts and the early return", "1 x 1 x 1 of 7 at 3.5, outside 9"),
    "iso_count:tile-skipped:t0>=1": ("the same in a call with some t0[a] >= 1", "a clip box from 32 (x) or 8 (y, z) under pad"),
    "iso_count:skipped:rows-outside-the-cell-box": ("k_iso_count: uy >= A.uLo[1] && uy < A.uHi[1] && uz >= ... fails for rows of a skipped tile", "a skipped tile with uLo or uHi off the tile along y or z"),
    "iso_count:crossed-by-outside-alone": ("k_iso_count: if (beyond) mn = fminf(mn, A.outside) ...: the bricks lie on one side of the level, the tile has triangles", "1 x 1 x 1 of 7 at 3.5, outside 0, pad"),
    "iso_count:staged-without-a-triangle": ("k_iso_count: a staged tile whose runs all count 0: the range crosses through voxels the box or a cell's ownership excludes", "2 x 1 x 1 of (0, 7), clip box on the 7"),
    "iso_sums:blocks==1": ("iso_extract: nb = ceil(runs / kIsoRunsPerBlock) == 1", "1 x 1 x 1"),
    "iso_sums:blocks>=2": ("iso_extract: nb >= 2, blockTris[blockIdx.x] carries into k_iso_offsets", "2,049 runs"),
    "iso_sums:tail-partial": ("k_iso_sums, k_iso_offsets: first + k < runs fails in the last block, runs % 2048 != 0", "1 x 1 x 1"),
    "iso_sums:all-whole": ("first + k < runs holds for every thread, runs % 2048 == 0", "4 x 63 x 31 under pad: 1 x 64 x 32 runs"),
    "iso_scan:rounds==1": ("k_iso_scan_sums: n <= 1024 block sums", "1 x 1 x 1"),
    "iso_scan:rounds>=2": ("k_iso_scan_sums: i0 += 1024 with the carries, more than 1024 blocks of 2,048 runs", f"2,097,153 runs: {SCAN_TEST} (2 x 2901 x 2901, 8,410,000 runs)"),
    "iso_place:blocks==1": ("iso_extract: ceil(activeRuns / 8) == 1 workgroup of k_iso_place", "1 active run"),
    "iso_place:blocks>=2": ("activeRuns > 8: hw = blockIdx.x * 8 + (t >> 5)", "9 active runs"),
    "iso_place:half-wave-idle": ("k_iso_place: live = hw < active fails for half-waves of the last workgroup, active % 8 != 0; they still reach block_sum", "1 active run"),
    "iso_place:live-and-dead-in-one-wave": ("k_iso_place: live is uniform over the half-wave, not over the wave: active odd, __shfl_up of width 32 beside a dead half", "1 active run"),
    "iso_place:five-in-a-cell": ("k_iso_place: for (k = 0; k < n; k++) with n == 5, which = cs | k << 8 up to k = 4", "one cell of a 5-triangle case"),
    "iso_emit:blocks==1": ("iso_extract: ceil(total / kBlock) == 1 workgroup of k_iso_emit", "1 triangle"),
    "iso_emit:blocks>=2": ("total > kBlock: d = blockIdx.x * kBlock + threadIdx.x", "257 triangles"),
    "iso_emit:no-triangle": ("iso_extract: total == 0 behind the count and rank kernels, k_iso_place and k_iso_emit are not launched", "1 x 1 x 1 of 7 at 3.5, outside 9"),
    "iso_out:buffer-grows": ("iso_extract: total > c->isoCap || !c->d_iso, both buffers are replaced", "the first call of a context"),
    "iso_out:buffer-kept": ("iso_extract: total <= c->isoCap, the list is written into the buffer of a longer one", "a shorter list after a longer one"),
}

# class -> (the condition, the refusal or the size that keeps it out of a test)
BY_INSPECTION = {
    "iso:tri_cell>=2^31": ("k_iso_place: cell = (uz * (dimY + 1) + uy) * (dimX + 1) + ux in an int", "iso_check refuses: '(dimX + 1)(dimY + 1)(dimZ + 1) is 2^31 or more'"),
    "iso:triangles>=2^31": ("k_iso_offsets: activeOff saturates at kIsoTooMany; k_iso_emit: d and total are unsigned", "iso_extract refuses: 'more than 2^31 - 1 triangles', before anything is emitted; such a list is 96 GiB"),
    "iso:runs-near-2^31": ("iso_extract: (unsigned)nb workgroups, activeRun holds (unsigned)(first + k)", "runs <= cells / 32 + the rows' ends < 2^31 by the tri_cell refusal; 2^30 runs need 44 GiB of scratch"),
}


# ---------------------------------------------------------------- the geometry
def geometry(dims, pad, clip):
    """iso_extract's loop over the axes: lo, hi, uLo, uHi, cells, t0, tiles as 3-tuples and runs; None for a box without a cell."""
    p = 1 if pad else 0
    lo = tuple(clip[0]) if clip is not None else (0, 0, 0)                # A.lo[a] = p->clip ? p->clip_lo[a] : 0
    hi = tuple(clip[1]) if clip is not None else tuple(dims)              # A.hi[a] = p->clip ? p->clip_hi[a] : c->voxDim[a]
    uLo = tuple(l - p + 1 for l in lo)                                    # A.uLo[a] = A.lo[a] - p->pad + 1
    uHi = tuple(h - 1 + p + 1 for h in hi)                                # A.uHi[a] = A.hi[a] - 1 + p->pad + 1
    cells = tuple(b - a for a, b in zip(uLo, uHi))                        # cells[a] = A.uHi[a] - A.uLo[a]
    if min(cells) <= 0:                                                   # if (cells[a] <= 0) empty = true
        return None
    t0 = tuple(a // t for a, t in zip(uLo, TILE))                         # A.t0[a] = A.uLo[a] / tile[a]
    tiles = tuple((b + t - 1) // t - s for b, t, s in zip(uHi, TILE, t0))  # tiles[a] = (A.uHi[a] + tile[a] - 1) / tile[a] - A.t0[a]
    runs = tiles[0] * cells[1] * cells[2]                                 # runs = A.runsX * A.ny * A.nz
    return dict(lo=lo, hi=hi, uLo=uLo, uHi=uHi, cells=cells, t0=t0, tiles=tiles, runs=runs)


def brick_table(volume, outside=1.0e9, valid=VALID):
    """k_iso_bricks: (mn, mx), each (nbz, nby, nbx) float32: every 8^3 brick's smallest and largest substituted value.  The box does
    not enter."""
    vol = np.asarray(volume, np.int32)
    f = np.where((vol >= valid[0]) & (vol <= valid[1]), vol.astype(F), F(outside)).astype(F)       # v >= validLo && v <= validHi ? (float)v : outside
    nb = tuple((n + 7) // 8 for n in vol.shape)                                                    # A.nbz, A.nby, A.nbx
    out = []
    for fill, fold in ((np.inf, np.min), (-np.inf, np.max)):                                       # mn = inf, mx = -inf; by * 8 + k < y1, x < A.dimX
        g = np.full(tuple(8 * n for n in nb), fill, F)
        g[:vol.shape[0], :vol.shape[1], :vol.shape[2]] = f
        out.append(fold(g.reshape(nb[0], 8, nb[1], 8, nb[2], 8), axis=(1, 3, 5)))
    return out[0], out[1]


def run_index(g, ux, uy, uz):
    """iso_run with bx = ux / 32 - t0[0]."""
    return ((uz - g["uLo"][2]) * g["cells"][1] + (uy - g["uLo"][1])) * g["tiles"][0] + (ux // TILE[0] - g["t0"][0])


def cells_of(tri_cell, dims):
    """tri_cell -> (ux, uy, uz), as k_iso_emit takes it apart."""
    c = np.asarray(tri_cell, np.int64)
    ux, r = c % (dims[0] + 1), c // (dims[0] + 1)                         # ux = cell % (A.dimX + 1), r = cell / (A.dimX + 1)
    return ux, r % (dims[1] + 1), r // (dims[1] + 1)


Tile = namedtuple("Tile", "b beyond bricks skipped triangles rows_outside")


def tiles_of(volume, level, outside=1.0e9, valid=VALID, pad=True, clip=None, ref=None, bricks=None):
    """The workgroups of k_iso_count, in blockIdx order: Tile(b = (bx, by, bz); beyond: the tile's samples reach beyond the box; bricks:
    (min, max) of the bricks its 33 x 9 x 9 samples touch, before `outside` joins them; skipped: with the table on; triangles: by
    iso_ref; rows_outside: some of its 8 x 8 rows lie outside the cell box).  A skipped tile has no triangle: asserted here, on
    the rule alone.  ref: iso_ref.extract of the same call, bricks: brick_table of the same volume, when the caller has them."""
    vol = np.asarray(volume, np.int32)
    dims = vol.shape[::-1]
    g = geometry(dims, pad, clip)
    if g is None:
        return []
    if ref is None:
        ref = ir.extract(vol, np.zeros(3, F), F(1), level, outside, valid, pad, clip)
    mnT, mxT = bricks if bricks is not None else brick_table(vol, outside, valid)
    level, outside = F(level), F(outside)
    ux, uy, uz = cells_of(ref[1], dims)
    per_tile = np.zeros(g["tiles"][::-1], np.int64)
    np.add.at(per_tile, (uz // TILE[2] - g["t0"][2], uy // TILE[1] - g["t0"][1], ux // TILE[0] - g["t0"][0]), 1)
    nb = mnT.shape[::-1]
    # the (min, max) of the bricks every tile touches, an axis at a time: a box of bricks is a product of three ranges
    mnB, mxB = mnT, mxT
    for a in range(3):
        ax = 2 - a
        parts = ([], [])
        for b in range(g["tiles"][a]):
            s0 = (g["t0"][a] + b) * TILE[a] - 1                                                   # s0 = u0 - 1: the tile's first sample
            k0, k1 = max(s0 >> 3, 0), min((s0 + TILE[a]) >> 3, nb[a] - 1)                         # for (kx = s0x >> 3; kx <= (s0x + kIsoTileX) >> 3; kx++)
            sel = [slice(None)] * 3                                                               # if (kx < 0 || ... || kx >= A.nbx ...) continue
            sel[ax] = slice(k0, k1 + 1)
            for part, whole, fold, none in ((parts[0], mnB, np.min, np.inf), (parts[1], mxB, np.max, -np.inf)):
                part.append(fold(whole[tuple(sel)], axis=ax, initial=none))
        mnB, mxB = np.stack(parts[0], axis=ax), np.stack(parts[1], axis=ax)
    out = []
    for bz, by, bx in itertools.product(*(range(n) for n in g["tiles"][::-1])):                    # bx = blockIdx.x % tilesX, by = rest % tilesY, bz = rest / tilesY
        b = (bx, by, bz)
        u0 = [(g["t0"][a] + b[a]) * TILE[a] for a in range(3)]                                    # u0 = (A.t0 + b) * kIsoTile
        s0 = [u - 1 for u in u0]
        beyond = any(s0[a] < g["lo"][a] or s0[a] + TILE[a] >= g["hi"][a] for a in range(3))       # bool beyond = s0x < A.lo[0] || s0x + kIsoTileX >= A.hi[0] || ...
        mn, mx = F(mnB[bz, by, bx]), F(mxB[bz, by, bx])
        smn, smx = (min(mn, outside), max(mx, outside)) if beyond else (mn, mx)                   # if (beyond) { mn = fminf(mn, A.outside); mx = fmaxf(mx, A.outside); }
        skipped = bool(smn >= level or smx < level)                                               # if (mn >= A.level || mx < A.level)
        rows_outside = any(u0[a] < g["uLo"][a] or u0[a] + TILE[a] > g["uHi"][a] for a in (1, 2))  # uy >= A.uLo[1] && uy < A.uHi[1] && uz >= A.uLo[2] && uz < A.uHi[2]
        n = int(per_tile[bz, by, bx])
        assert not (skipped and n), f"a skipped tile {b} holds {n} triangles: the skip rule is wrong"
        out.append(Tile(b, beyond, (mn, mx), skipped, n, rows_outside))
    return out


def rows_written(g, t0=None, guard=True):
    """How often k_iso_count's workgroups write each run's count, on either path (the staged tile's `rowY && rowZ` and the skipped
    tile's test are the same condition): an array of `runs` counts, and the number of writes that fall outside it.  t0 and guard
    restate the kernel with another first tile, or without the uLo / uHi test, to show what those would do."""
    t0 = g["t0"] if t0 is None else t0
    hits = np.zeros(g["runs"], np.int64)
    stray = 0
    for bz, by, bx in itertools.product(*(range(n) for n in g["tiles"][::-1])):
        for dz, dy in itertools.product(range(TILE[2]), range(TILE[1])):
            uy, uz = (t0[1] + by) * TILE[1] + dy, (t0[2] + bz) * TILE[2] + dz
            if guard and not (g["uLo"][1] <= uy < g["uHi"][1] and g["uLo"][2] <= uz < g["uHi"][2]):
                continue
            run = ((uz - g["uLo"][2]) * g["cells"][1] + (uy - g["uLo"][1])) * g["tiles"][0] + bx  # iso_run(A, bx, uy, uz)
            if 0 <= run < g["runs"]:
                hits[run] += 1
            else:
                stray += 1
    return hits, stray


def launch_classes(dims, pad, clip, table=True):
    """The rows that the dims, the pad and the box alone decide."""
    g = geometry(dims, pad, clip)
    if g is None:
        return {"iso:box-without-a-cell"}
    out = set()
    for a, n in enumerate(AXES):
        out.add(f"iso:t0-{n}" + ("==0" if g["t0"][a] == 0 else ">=1"))
        out.add(f"iso:first-tile-{n}:" + ("whole" if g["uLo"][a] % TILE[a] == 0 else "partial"))
        out.add(f"iso:last-tile-{n}:" + ("whole" if g["uHi"][a] % TILE[a] == 0 else "partial"))
        out.add(f"iso:tiles-{n}" + ("==1" if g["tiles"][a] == 1 else ">=2"))
    if table:                                                                                     # if (A.useTable)
        nb = [(d + 7) // 8 for d in dims]
        runs_b = (nb[0] + 7) // 8                                                                 # runsB = (A.nbx + 7) / 8
        out.add("iso_bricks:runs-x" + ("==1" if runs_b == 1 else ">=2"))
        out |= {f"iso_bricks:brick-partial-{n}" for a, n in enumerate(AXES) if dims[a] % 8}
        waves = runs_b * nb[1] * nb[2]                                                            # waves = runsB * A.nby * A.nbz
        out.add("iso_bricks:last-block-" + ("short" if waves % (BLOCK // WAVE) else "whole"))      # w >= waves
    blocks = (g["runs"] + RUNS_PER_BLOCK - 1) // RUNS_PER_BLOCK                                   # nb = (runs + kIsoRunsPerBlock - 1) / kIsoRunsPerBlock
    out.add("iso_sums:blocks" + ("==1" if blocks == 1 else ">=2"))
    out.add("iso_sums:" + ("tail-partial" if g["runs"] % RUNS_PER_BLOCK else "all-whole"))         # first + k < runs
    out.add("iso_scan:rounds" + ("==1" if blocks <= SCAN else ">=2"))                             # for (i0 = 0; i0 < n; i0 += 1024)
    return out


def active_runs(g, dims, tri_cell):
    """The runs that hold a triangle (k_iso_sums: active += c ? 1 : 0)."""
    ux, uy, uz = cells_of(tri_cell, dims)
    return len(np.unique(run_index(g, ux, uy, uz)))


def buffer_class(cap, total):
    """iso_extract's output buffer: (the row, the capacity after the call).  cap: the capacity before it, 0 for a context that has
    none yet."""
    if total > cap or cap == 0:                                                                   # if (total > c->isoCap || !c->d_iso)
        return "iso_out:buffer-grows", max(total, 1)                                              # cap = total ? total : 1
    return "iso_out:buffer-kept", cap


def classes(volume, level, outside=1.0e9, valid=VALID, pad=True, clip=None, table=True, cap=None, ref=None, bricks=None, tiles=None):
    """The rows of TABLE one call takes.  table: whether the brick table is on; cap: the output buffer's capacity before the call,
    None to leave the iso_out rows out; tiles: tiles_of the same call, when the caller has it."""
    vol = np.asarray(volume, np.int32)
    dims = vol.shape[::-1]
    out = launch_classes(dims, pad, clip, table)
    g = geometry(dims, pad, clip)
    if g is None:
        return out
    if ref is None:
        ref = ir.extract(vol, np.zeros(3, F), F(1), level, outside, valid, pad, clip)
    later = ":t0>=1" if max(g["t0"]) >= 1 else ""
    for t in tiles if tiles is not None else tiles_of(vol, level, outside, valid, pad, clip, ref, bricks):
        if table and t.skipped:
            out |= {"iso_count:tile-skipped", "iso_count:tile-skipped" + later}
            if t.rows_outside:
                out.add("iso_count:skipped:rows-outside-the-cell-box")
            continue
        out |= {"iso_count:tile-staged", "iso_count:tile-staged" + later}
        if t.triangles == 0:
            out.add("iso_count:staged-without-a-triangle")
        elif t.beyond and (t.bricks[0] >= F(level) or t.bricks[1] < F(level)):
            out.add("iso_count:crossed-by-outside-alone")
    total = len(ref[1])
    if total == 0:                                                                                # if (total > 0)
        out.add("iso_emit:no-triangle")
    else:
        active = active_runs(g, dims, ref[1])
        out.add("iso_place:blocks" + ("==1" if active <= BLOCK // 32 else ">=2"))                  # (activeRuns + kBlock / 32 - 1) / (kBlock / 32)
        if active % (BLOCK // 32):
            out.add("iso_place:half-wave-idle")                                                   # live = hw < active
        if active % 2:
            out.add("iso_place:live-and-dead-in-one-wave")
        if np.bincount(np.unique(ref[1], return_inverse=True)[1]).max() == 5:
            out.add("iso_place:five-in-a-cell")                                                   # n = triCount[cs] == 5
        out.add("iso_emit:blocks" + ("==1" if total <= BLOCK else ">=2"))                          # (total + kBlock - 1) / kBlock
    if cap is not None:
        out.add(buffer_class(cap, total)[0])
    return out


# ---------------------------------------------------------------- the inputs
GMIN = np.array([-1.5, 0.25, 2.0], F)       # not a round origin: positions round
VS = F(0.375)
LEVEL = 3.5
WINDOW = dict(valid=(1, 6), outside=9.0)    # the window removes the uniform 0 and 7; `outside` sits above the level

SHELF_X = [(0, 100), (31, 100), (32, 100), (33, 64), (33, 65), (31, 63), (64, 100), (65, 96), (70, 72), (0, 31), (0, 32), (95, 100)]
SHELF_Y = [(0, 28), (7, 28), (8, 16), (9, 17), (8, 9), (15, 24), (16, 28)]
SHELF_Z = [(0, 27), (7, 27), (8, 16), (9, 15), (16, 17), (17, 27)]
WINDOW_X = [(0, 100), (33, 65), (31, 63), (65, 96), (95, 100)]
WINDOW_Y = [(0, 28), (9, 17), (15, 24)]
WINDOW_Z = [(0, 27), (9, 15)]
ROW_X = [(1984, 2100), (2047, 2049), (64, 2080)]

_GRIDS = {}


def grid(name):
    """The volumes, made once and never written to.
    shelf  100 x 28 x 27: 7 everywhere, noise 0..7 at x >= 40, a block of 0 at x 66..99, y 9..27, z 9..26
    row    2100 x 3 x 3 of noise 0..7: 66 runs a row, 33 brick runs
    even63, even127   4 x 63 x 31 and 4 x 127 x 31 of noise: 2,048 and 4,096 runs under pad"""
    if name not in _GRIDS:
        if name == "shelf":
            rng = np.random.default_rng(3001)
            v = np.full((27, 28, 100), 7, np.int32)
            v[:, :, 40:] = rng.integers(0, 8, (27, 28, 60))
            v[9:27, 9:28, 66:100] = 0
        else:
            dims = {"row": (2100, 3, 3), "even63": (4, 63, 31), "even127": (4, 127, 31)}[name]
            v = np.random.default_rng(3002 + dims[1]).integers(0, 8, dims[::-1]).astype(np.int32)
        v.setflags(write=False)
        _GRIDS[name] = v
    return _GRIDS[name]


Call = namedtuple("Call", "grid level outside valid pad clip")


def _boxes(xs, ys, zs):
    return [((x[0], y[0], z[0]), (x[1], y[1], z[1])) for x, y, z in itertools.product(xs, ys, zs)]


def shelf_calls(pad):
    """The full product of the shelf's clip ends and the call without a box: 505 calls."""
    return [Call("shelf", LEVEL, 0.0, VALID, pad, clip) for clip in [None, *_boxes(SHELF_X, SHELF_Y, SHELF_Z)]]


def window_calls():
    return [Call("shelf", LEVEL, WINDOW["outside"], WINDOW["valid"], pad, clip) for pad in (True, False) for clip in _boxes(WINDOW_X, WINDOW_Y, WINDOW_Z)]


def row_calls():
    return [Call("row", LEVEL, 0.0, VALID, pad, clip) for pad in (True, False) for clip in [None, *_boxes(ROW_X, [(0, 3)], [(0, 3)])]]


def even_calls():
    return [Call(name, LEVEL, outside, valid, True, None) for name in ("even63", "even127") for outside, valid in ((0.0, VALID), (WINDOW["outside"], WINDOW["valid"]))]


def all_calls():
    return [*shelf_calls(True), *shelf_calls(False), *window_calls(), *row_calls(), *even_calls()]


_REF = {}
_BRICKS = {}
_TILES = {}


def ref(call):
    """iso_ref's list of a call, computed once."""
    if call not in _REF:
        _REF[call] = ir.extract(grid(call.grid), GMIN, VS, call.level, call.outside, call.valid, call.pad, call.clip)
    return _REF[call]


def cell_list(call):
    """tri_cell of a call without its triangles: the owning cell of every triangle, from the case bytes alone."""
    vol = grid(call.grid)
    dz, dy, dx = vol.shape
    S, first = ir.samples(vol, call.level, call.outside, call.valid, call.pad, call.clip)
    if min(S.shape) < 2:
        return np.zeros(0, np.int32)
    n = ir.TRI_COUNT[ir.cells_of_samples(S, call.level)]
    cz, cy, cx = np.nonzero(n)
    cell = ((cz + first[2] + 1) * (dy + 1) + (cy + first[1] + 1)) * (dx + 1) + (cx + first[0] + 1)
    return np.repeat(cell, n[cz, cy, cx]).astype(np.int32)


def call_classes(call, table=True, cap=None):
    key = (call.grid, call.outside, call.valid)
    if key not in _BRICKS:
        _BRICKS[key] = brick_table(grid(call.grid), call.outside, call.valid)
    if call not in _TILES:
        _TILES[call] = tiles_of(grid(call.grid), call.level, call.outside, call.valid, call.pad, call.clip, ref(call), _BRICKS[key])
    return classes(grid(call.grid), call.level, call.outside, call.valid, call.pad, call.clip, table, cap, ref(call), _BRICKS[key], _TILES[call])


def call_geometry(call):
    return geometry(grid(call.grid).shape[::-1], call.pad, call.clip)


def ordered(calls):
    """The calls in the order the GPU makes them: a long list, then a box without a cell while there are any, then a short list
    (a list of no triangle counts as short), and so on: the output buffer is kept after it grew, and nothing follows nothing.
    The long lists begin with four of rising length and then the longest, so a context that starts here grows its buffer five
    times; the rest fall."""
    with_cells = sorted((c for c in calls if call_geometry(c) is not None), key=lambda c: -len(ref(c)[1]))     # stable: ties keep their order
    without = [c for c in calls if call_geometry(c) is None]
    half = (len(with_cells) + 1) // 2
    long, short = with_cells[:half], with_cells[half:][::-1]
    if half >= 5:
        ramp = [half * k // 5 for k in (4, 3, 2, 1)]
        long = [long[i] for i in ramp] + [c for i, c in enumerate(long) if i not in ramp]
    assert len(without) <= len(long) and (not without or len(ref(long[len(without) - 1])[1]) > 0), "a box without a cell follows a list"
    out = []
    for i, c in enumerate(long):
        out.append(c)
        if i < len(without):
            out.append(without[i])
        if i < len(short):
            out.append(short[i])
    return out
