"""Seeded voxel grids for rto_build_leaf_triangles at its thread, wave and chunk edges.  Every case is
(name, dims (x, y, z), data uint8 (dimZ, dimY, dimX), grid_min, voxel_size).

The builder walks a leaf's candidate cells -- those on the leaf's three max faces, cut by `c < dim - 1` -- with one thread up to
64 candidates (serial), one wave in steps of 64 up to 2048 (wave), and one wave per chunk of 2048 above that (chunks).  The
enumeration has one form per clip mask fullX | fullY << 1 | fullZ << 2, an axis being full when dim - 1 does not cut the leaf on it.

Construction: uniform blocks (aligned cubes, so each becomes one leaf) in salt-and-pepper noise of p = 0.5, which makes the
blocks' max-face cells emit triangles and keeps the blocks from merging with their siblings.  A block that reaches past the grid
has to be EMPTY (voxels outside the grid read EMPTY, so only then is the cube uniform); a block inside the grid may be FILLED.

  name              dims            block(s)                         the block's leaf
  serial64_mask4    (9, 9, 18)      16^3 EMPTY, cut to 9 x 9 x 16    total 64 = 8 * 8: one thread, exactly at the limit
  wave65_mask4      (14, 6, 18)     16^3 EMPTY, cut to 14 x 6 x 16   total 65 = 13 * 5: the smallest leaf a wave walks
  chunk2048_mask4   (33, 65, 130)   128^3 EMPTY, cut to 33 x 65      total 2048 = 32 * 64: one chunk, full
  chunk2080_mask4   (33, 66, 130)   128^3 EMPTY, cut to 33 x 66      total 2080 = 32 * 65: two chunks, the last of half a wave
  chunks_mask7      (70, 45, 33)    32^3 EMPTY                       total 2977 = 3 s^2 - 3 s + 1: two chunks among 89 k nodes
  chunks_mask6      (21, 66, 67)    64^3 EMPTY, x cut to 20          total 2540 = 20 * 127
  chunks_mask5      (67, 34, 66)    64^3 EMPTY, y cut to 33          total 4191 = 33 * 127: three chunks
  chunks_mask3      (66, 67, 18)    64^3 EMPTY, z cut to 17          total 2159 = 17 * 127
  chunks_mask1      (66, 51, 46)    64^3 EMPTY, y to 50, z to 45     total 2250 = 50 * 45
  chunks_mask2      (48, 66, 62)    64^3 EMPTY, x to 47, z to 61     total 2867 = 47 * 61
  chunks_offorigin  (66, 67, 65)    32^3 FILLED at (32, 32, 32)      total 2977, mask 7, x0, y0, z0 != 0 on the chunk path
  corner16          (44, 43, 42)    16^3 at {0, 32}^3                totals 65 .. 2048 with masks 0 .. 7 (origin block FILLED)
  corner4           (11, 10, 10)    4^3 at {0, 8}^3                  totals 1 .. 64 with masks 0 .. 7 (origin block FILLED)
  checkerboard      (64, 64, 64)    8^3 blocks, alternating, no noise  512 leaves, 490 of them above 64 candidates: the big
                                                                     list spans two workgroups; FILLED leaves cut by one voxel
  dimx1             (1, 9, 7)       noise                            dimX - 1 == 0: no leaf has a candidate
  all_empty         (12, 9, 7)      --                               one EMPTY root leaf
  all_filled        (12, 9, 7)      --                               every cell has eight FILLED corners

BLOCKS gives each case's planted leaves as (x0, y0, z0, size, total, mask); tests/test_leaf_triangle_edges.py checks them against
the oracle's octree."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

EMPTY, FILLED = 0, 1
GRID_MIN = np.array([0.5, -2.0, 3.0], np.float32)
VOXEL = np.float32(0.3)


class Case(NamedTuple):
    name: str
    dims: tuple
    data: np.ndarray
    grid_min: np.ndarray
    voxel_size: np.float32


def _noise(dims, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((dims[2], dims[1], dims[0])) < 0.5).astype(np.uint8)


def _plant(data, origin, size, value):
    x0, y0, z0 = origin
    data[z0:z0 + size, y0:y0 + size, x0:x0 + size] = value              # the slice stops at the grid's sides


def _blocks_in_noise(name, dims, seed, blocks):
    data = _noise(dims, seed)
    for origin, size, value in blocks:
        _plant(data, origin, size, value)
    return Case(name, tuple(dims), data, GRID_MIN.copy(), VOXEL)


def _corners(name, dims, seed, size, far):
    """Blocks of edge `size` at {0, far}^3: the one at the origin FILLED and inside the grid, the others EMPTY and cut by the
    grid's sides on the axes where they sit at `far`."""
    blocks = [((far * (c & 1), far * (c >> 1 & 1), far * (c >> 2 & 1)), size, FILLED if c == 0 else EMPTY) for c in range(8)]
    return _blocks_in_noise(name, dims, seed, blocks)


def _checkerboard():
    b = np.indices((8, 8, 8)).sum(0) & 1
    data = np.kron(b, np.ones((8, 8, 8), np.int64)).astype(np.uint8)
    return Case("checkerboard", (64, 64, 64), data, GRID_MIN.copy(), VOXEL)


def _degenerate(name):
    dims = (1, 9, 7) if name == "dimx1" else (12, 9, 7)
    if name == "dimx1":
        data = _noise(dims, 31)
    else:
        data = np.full((dims[2], dims[1], dims[0]), FILLED if name == "all_filled" else EMPTY, np.uint8)
    return Case(name, dims, data, GRID_MIN.copy(), VOXEL)


_O = (0, 0, 0)
_MAKERS = {
    "serial64_mask4": lambda n: _blocks_in_noise(n, (9, 9, 18), 1, [(_O, 16, EMPTY)]),
    "wave65_mask4": lambda n: _blocks_in_noise(n, (14, 6, 18), 2, [(_O, 16, EMPTY)]),
    "chunk2048_mask4": lambda n: _blocks_in_noise(n, (33, 65, 130), 3, [(_O, 128, EMPTY)]),
    "chunk2080_mask4": lambda n: _blocks_in_noise(n, (33, 66, 130), 4, [(_O, 128, EMPTY)]),
    "chunks_mask7": lambda n: _blocks_in_noise(n, (70, 45, 33), 5, [(_O, 32, EMPTY)]),
    "chunks_mask6": lambda n: _blocks_in_noise(n, (21, 66, 67), 6, [(_O, 64, EMPTY)]),
    "chunks_mask5": lambda n: _blocks_in_noise(n, (67, 34, 66), 7, [(_O, 64, EMPTY)]),
    "chunks_mask3": lambda n: _blocks_in_noise(n, (66, 67, 18), 8, [(_O, 64, EMPTY)]),
    "chunks_mask1": lambda n: _blocks_in_noise(n, (66, 51, 46), 9, [(_O, 64, EMPTY)]),
    "chunks_mask2": lambda n: _blocks_in_noise(n, (48, 66, 62), 10, [(_O, 64, EMPTY)]),
    "chunks_offorigin": lambda n: _blocks_in_noise(n, (66, 67, 65), 11, [((32, 32, 32), 32, FILLED)]),
    "corner16": lambda n: _corners(n, (44, 43, 42), 12, 16, 32),
    "corner4": lambda n: _corners(n, (11, 10, 10), 13, 4, 8),
    "checkerboard": lambda n: _checkerboard(),
    "dimx1": _degenerate,
    "all_empty": _degenerate,
    "all_filled": _degenerate,
}
NAMES = tuple(_MAKERS)
DEGENERATE = ("dimx1", "all_empty", "all_filled")


def make(name) -> Case:
    return _MAKERS[name](name)


def _corner_rows(size, far, e):
    """(x0, y0, z0, size, total, mask) of _corners' eight blocks; e = the cut extents (ex, ey, ez) of the blocks at `far`."""
    rows = []
    for c in range(8):
        ext = [e[a] if (c >> a) & 1 else size for a in range(3)]
        inner = [min(v, size - 1) for v in ext]
        mask = sum(1 << a for a in range(3) if ext[a] == size)
        # the block at (far, far, far) is all of its octant that lies inside the grid: the leaf is the octant, of twice the edge
        rows.append((far * (c & 1), far * (c >> 1 & 1), far * (c >> 2 & 1), 2 * size if c == 7 else size,
                     ext[0] * ext[1] * ext[2] - inner[0] * inner[1] * inner[2], mask))
    return rows


# the planted leaves every case promises: (x0, y0, z0, size, total, mask)
BLOCKS = {
    "serial64_mask4": [(0, 0, 0, 16, 64, 4)],
    "wave65_mask4": [(0, 0, 0, 16, 65, 4)],
    "chunk2048_mask4": [(0, 0, 0, 128, 2048, 4)],
    "chunk2080_mask4": [(0, 0, 0, 128, 2080, 4)],
    "chunks_mask7": [(0, 0, 0, 32, 2977, 7)],
    "chunks_mask6": [(0, 0, 0, 64, 2540, 6)],
    "chunks_mask5": [(0, 0, 0, 64, 4191, 5)],
    "chunks_mask3": [(0, 0, 0, 64, 2159, 3)],
    "chunks_mask1": [(0, 0, 0, 64, 2250, 1)],
    "chunks_mask2": [(0, 0, 0, 64, 2867, 2)],
    "chunks_offorigin": [(32, 32, 32, 32, 2977, 7)],
    "corner16": _corner_rows(16, 32, (11, 10, 9)),
    "corner4": _corner_rows(4, 8, (2, 1, 1)),
    "checkerboard": [(0, 0, 0, 8, 169, 7), (56, 0, 0, 8, 105, 6), (0, 56, 0, 8, 105, 5), (0, 0, 56, 8, 105, 3),
                     (56, 56, 0, 8, 49, 4), (56, 0, 56, 8, 49, 2), (0, 56, 56, 8, 49, 1), (56, 56, 56, 8, 0, 0)],
    "dimx1": [],
    "all_empty": [(0, 0, 0, 16, 0, 0)],
    "all_filled": [],
}

# a voxel strictly inside the uniform block of the two cases the edit test splits and restores
EDIT_VOXEL = {"chunk2080_mask4": (13, 40, 77), "chunks_mask7": (21, 9, 14)}
