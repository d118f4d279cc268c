"""The launch shapes of the grid kernels ("Launch shapes of the grid kernels"), as code: which template, which side of a
launch cap, which trip count of a device loop the *shape* of an input selects -- its dims, its voxel count, its component, seed,
anchor or brush-box count.  Plain functions: no GPU, no import of the library.  Each line restates one selection of the host code
or of a kernel and names the condition it mirrors; a mirror can drift, so the table is re-read when a launch line changes.

Paths that the grid's *content* selects (how many merge passes, which tiles wake, which waves hold one label) are not here: the
feature suites pin them with grids made for them (serpentine48, the maze, tests/test_tile_wake.py).

dims is (dimX, dimY, dimZ); a grid array has shape dims[::-1]."""
from __future__ import annotations

BLOCK = 256                   # kBlock
TILE = (32, 8, 8)             # kCcTileX, kCcTileY, kCcTileZ
VEC = 16                      # kCcVec, kEditRun: bytes, or voxels, per wide access
CHUNK = BLOCK * 16            # kCcChunk, kDtChunk: voxels per block of the streaming kernels
DT_ROW_VOX = 2048             # kDtRowVox
TOTAL_CAP = 1024              # k_measure_total's launch cap, workgroups
SUMMARY_CAP = 4096            # k_skel_summary's launch cap, workgroups
ALL_BUT_LARGEST = 1           # RTO_SELECT_ALL_BUT_LARGEST

# class -> (the condition in the source, the smallest input that takes it)
TABLE = {
    # rto_edit.inc
    "edit_voxels:nothing-inside": ("rto_edit_voxels: n == 0 || box[0] > box[3], no launch", "any grid, one brush outside it"),
    "edit_brushes:wide": ("rto_edit_voxels: dims[0] % kEditRun == 0", "16 x 1 x 1"),
    "edit_brushes:narrow": ("rto_edit_voxels: dims[0] % kEditRun != 0", "1 x 1 x 1"),
    "edit_brushes:blocks-x==1": ("eb.blocksX == 1: the box spans at most 16 runs of 16", "1 x 1 x 1"),
    "edit_brushes:blocks-x>=2": ("eb.blocksX >= 2: run >= box.runsX in the last block", "a box 257 voxels wide"),
    "edit_brushes:blocks-y==1": ("eb.blocksY == 1: y >= box.y1 for the threads behind the box", "a box at most 16 rows high"),
    "edit_brushes:blocks-y>=2": ("eb.blocksY >= 2", "a box 17 rows high"),
    # rto_components.inc
    "cc_local:wide": ("cc_label: D.x % kCcVec == 0", "16 x 1 x 1"),
    "cc_local:narrow": ("cc_label: D.x % kCcVec != 0", "1 x 1 x 1"),
    "cc_local:wide:chunk-beyond-row": ("k_cc_local<WIDE>: c0 >= D.x, dimX = 16 mod 32", "16 x 1 x 1"),
    "cc_local:rows-beyond-grid": ("k_cc_local: !rowIn, dimY % 8 or dimZ % 8", "1 x 1 x 1"),
    "cc_local:rows-all-inside": ("k_cc_local: rowIn for every thread", "1 x 8 x 8"),
    "cc_scan:rounds==1": ("k_scan_counts<kBlock> behind k_cc_flatten: n <= kBlock chunks", "1 x 1 x 1"),
    "cc_scan:rounds>=2": ("k_scan_counts<kBlock>: i0 += THREADS, n > kBlock chunks, above 256 x 4096 voxels", "1,048,577 voxels"),
    "cc_stats:all-whole": ("k_cc_stats: whole for every thread, n % 32 == 0", "32 x 1 x 1"),
    "cc_stats:tail-partial": ("k_cc_stats: !whole in the last thread, n % 32 != 0", "1 x 1 x 1"),
    "cc_label:count==0": ("cc_label: total == 0, k_cc_stats and k_cc_touches are not launched", "a grid without the set"),
    "cc_touches:blocks==1": ("cc_label: 1 <= total <= kBlock", "1 component"),
    "cc_touches:blocks>=2": ("cc_label: total > kBlock", "257 components"),
    "edit_components:count==0": ("rto_edit_components: r.count == 0, nothing is launched", "a grid without the set"),
    "cc_largest:rounds==1": ("k_cc_largest: count <= kBlock", "1 component"),
    "cc_largest:rounds>=2": ("k_cc_largest: i += kBlock, count > kBlock", "257 components"),
    "cc_select:blocks==1": ("rto_edit_components: count <= kBlock", "1 component"),
    "cc_select:blocks>=2": ("rto_edit_components: count > kBlock", "257 components"),
    "cc_flip:wide": ("rto_edit_components: n % kCcVec == 0", "16 x 1 x 1"),
    "cc_flip:narrow": ("rto_edit_components: n % kCcVec != 0", "1 x 1 x 1"),
    "cc_flip:wide:rows-unaligned": ("k_cc_flip<true> behind k_cc_local<false>: n % 16 == 0, dimX % 16 != 0", "4 x 4 x 1"),
    # rto_distance.inc
    "dt_x:wide": ("dt_transform: D.x % kCcVec == 0", "16 x 1 x 1"),
    "dt_x:narrow": ("dt_transform: D.x % kCcVec != 0", "1 x 1 x 1"),
    "dt_x:wide:piece-beyond-row": ("k_dt_x<WIDE>: x0 + 16 h >= D.x, dimX = 16 mod 32", "16 x 1 x 1"),
    "dt_x:rows-per-block>=2": ("dt_transform: kDtRowVox / D.x >= 2", "1 x 1 x 1"),
    "dt_x:rows-per-block==1": ("dt_transform: max(1, kDtRowVox / D.x) == 1", "1025 x 1 x 1"),
    "dt_x:blocks-all-full": ("k_dt_x: rows == rowsPerBlock in every block", "1 x 2048 x 1"),
    "dt_x:last-block-short": ("k_dt_x: rows = numRows - row0 < rowsPerBlock", "1 x 1 x 1"),
    "dt_x:mask-rounds==1": ("k_dt_x: words <= kBlock", "1 x 1 x 1"),
    "dt_x:mask-rounds>=2": ("k_dt_x: i += kBlock over words > kBlock", "1 x 257 x 1"),
    "dt_x:sweep-rounds==1": ("k_dt_x: rows <= kBlock", "1 x 1 x 1"),
    "dt_x:sweep-rounds>=2": ("k_dt_x: r += kBlock over rows > kBlock", "1 x 257 x 1"),
    "morph_flip:wide": ("rto_edit_morphology, rto_edit_geodesic: n % kCcVec == 0", "16 x 1 x 1"),
    "morph_flip:narrow": ("rto_edit_morphology, rto_edit_geodesic: n % kCcVec != 0", "1 x 1 x 1"),
    "morph_flip:wide:rows-unaligned": ("k_morph_flip<true> behind k_dt_x<false> or k_geo_relax<false, .>: n % 16 == 0, dimX % 16 != 0", "4 x 4 x 1"),
    # rto_geodesic.inc
    "geo_fill:all-whole": ("k_geo_fill: v0 + kCcVec <= n for every thread, n % 16 == 0", "16 x 1 x 1"),
    "geo_fill:tail-partial": ("k_geo_fill: the scalar tail, n % 16 != 0", "1 x 1 x 1"),
    "geo_seeds:blocks==1": ("geo_relax: n <= kBlock seeds", "1 seed"),
    "geo_seeds:blocks>=2": ("geo_relax: n > kBlock seeds", "257 seeds"),
    "geo_relax:wide": ("geo_relax: D.x % kCcVec == 0", "16 x 1 x 1"),
    "geo_relax:narrow": ("geo_relax: D.x % kCcVec != 0", "1 x 1 x 1"),
    "geo_relax:wide:chunk-beyond-row": ("k_geo_relax<WIDE>: c0 >= D.x, dimX = 16 mod 32", "16 x 1 x 1"),
    "geo_relax:rows-beyond-grid": ("k_geo_relax: !rowIn, dimY % 8 or dimZ % 8", "1 x 1 x 1"),
    "geo_relax:rows-all-inside": ("k_geo_relax: rowIn for every thread", "1 x 8 x 8"),
    # rto_thickness.inc
    "thick_gather:column-beyond-grid": ("k_thick_gather: !inXY or z0 + j >= D.z, a dim off its tile", "1 x 1 x 1"),
    "thick_gather:tiles-all-inside": ("k_thick_gather: every column of every tile inside", "32 x 8 x 8"),
    # rto_measure.inc
    "measure:count==0": ("rto_measure_components: count == 0, no kernel is launched", "a grid without the set"),
    "measure:wide": ("rto_measure_components: D.x % kCcVec == 0", "16 x 1 x 1"),
    "measure:narrow": ("rto_measure_components: D.x % kCcVec != 0", "1 x 1 x 1"),
    "measure:wide:segment-beyond-row": ("ms_load8<WIDE>: gx0 >= D.x, dimX = 16 mod 32", "16 x 1 x 1"),
    "measure:rows-beyond-grid": ("ms_load8: gy >= D.y || gz >= D.z for a tile row, dimY % 8 or dimZ % 8", "1 x 1 x 1"),
    "measure:rows-all-inside": ("ms_load8: every tile row inside", "1 x 8 x 8"),
    "measure_fold:blocks==1": ("rto_measure_components: tiles <= kBlock", "1 x 1 x 1"),
    "measure_fold:blocks>=2": ("rto_measure_components: tiles > kBlock", "257 tiles: 8193 x 1 x 1"),
    "measure_total:round==1": ("k_measure_total: count <= 1024 x 256", "1 component"),
    "measure_total:round>=2": ("k_measure_total: i += gridDim.x kBlock, count > 1024 x 256", "262,145 components"),
    # rto_skeleton.inc
    "skel_init:wide": ("skel_thin: D.x % 32 == 0", "32 x 1 x 1"),
    "skel_init:narrow": ("skel_thin: D.x % 32 != 0, cnt < 32 in a row's last word", "1 x 1 x 1"),
    "skel_window:words-per-row==1": ("sk_window: wx == 0 and wx + 1 == D.wordsX", "1 x 1 x 1"),
    "skel_window:words-per-row>=2": ("sk_window: wx > 0, wx + 1 < D.wordsX", "33 x 1 x 1"),
    "skel_step:voxel-beyond-grid": ("k_skel_step: !inGrid, a dim off its tile", "1 x 1 x 1"),
    "skel_step:tiles-all-inside": ("k_skel_step: inGrid for every thread", "32 x 8 x 8"),
    "skel_anchors:none": ("skel_thin: n == 0, VoxelList::upload makes no list and in_parts launches nothing", "no anchors"),
    "skel_anchors:blocks==1": ("skel_thin: 1 <= n <= kBlock anchors", "1 anchor"),
    "skel_anchors:blocks>=2": ("skel_thin: n > kBlock anchors", "257 anchors"),
    "skel_summary:round==1": ("k_skel_summary: nvox <= 4096 x 256", "1 x 1 x 1"),
    "skel_summary:round>=2": ("k_skel_summary: v += gridDim.x kBlock, nvox > 4096 x 256", "1,048,577 voxels"),
}

# class -> (the condition, the refusal or the limit that keeps a test from running it): the rows that say "by inspection"
BY_INSPECTION = {
    "grid:voxels>2^31-2": ("every 32-bit index of these files", "resident_grid_check refuses: 'the grid has more than 2^31 - 2 voxels'"),
    "dt:diagonal>=2^31-1": ("k_dt_x, k_dt_axis: a squared distance beyond int32", "dt_check_grid refuses: 'the grid's diagonal squared does not fit'"),
    "geo:longest-path>=2^31-1": ("k_geo_relax: a path length beyond int32", "geo_check_args refuses: 'the longest possible path does not fit'"),
    "measure:dim>32768": ("k_measure: tile-local sums beyond 32 bits", "rto_measure_components refuses: 'a dimension of the grid is above 32768'"),
    "edit_brushes:blocks>2^31-1": ("rto_edit_voxels: blocks > 0x7fffffff", "rto_edit_voxels refuses: 'the brushes' box is too large for one launch'"),
    "geo_seeds:launches>=2": ("geo_relax: VoxelList::in_parts, at += 2^30, above 2^30 seeds", "cannot hold: the list alone is 8 GiB on the host and again on the device"),
    "skel_anchors:launches>=2": ("skel_thin: VoxelList::in_parts, at += 2^30, above 2^30 anchors", "cannot hold: the list alone is 8 GiB on the host and again on the device"),
}

# the kernels' classes by the operation whose source file holds them
OWN = {
    "edit_voxels": ("edit_voxels:", "edit_brushes:"),
    "components": ("cc_", "edit_components:"),
    "distance": ("dt_x:", "morph_flip:"),
    "geodesic": ("geo_",),
    "thickness": ("thick_",),
    "measure": ("measure",),
    "skeleton": ("skel_",),
}


def own(operation):
    """The rows of TABLE that belong to `operation`'s source file."""
    return {c for c in TABLE if c.startswith(OWN[operation])}


def _voxels(dims):
    return dims[0] * dims[1] * dims[2]


def _tiles(dims):
    return tuple((d + t - 1) // t for d, t in zip(dims, TILE))         # CcTiles (cc_label, geo_relax, skel_thin, ...): the tiles along x, y, z


def _off_tile(dims):
    return any(d % t for d, t in zip(dims, TILE))


def _row_kernel(prefix, dims, beyond):
    """k_cc_local, k_geo_relax and k_measure: one thread per 8-voxel segment of a 32 x 8 x 8 tile, WIDE on dimX % 16."""
    x, y, z = dims
    out = {prefix + (":wide" if x % VEC == 0 else ":narrow")}           # D.x % kCcVec == 0
    if x % VEC == 0 and x % TILE[0] == VEC:                             # a 16-byte chunk of the last tile starts at or behind D.x
        out.add(prefix + ":wide:" + beyond)
    out.add(prefix + (":rows-beyond-grid" if y % TILE[1] or z % TILE[2] else ":rows-all-inside"))      # gy < D.y && gz < D.z
    return out


def _flip(prefix, dims):
    """k_cc_flip and k_morph_flip: a thread owns 16 consecutive voxels of the volume, WIDE on n % 16."""
    n = _voxels(dims)
    out = {prefix + (":wide" if n % VEC == 0 else ":narrow")}           # n % kCcVec == 0
    if n % VEC == 0 and dims[0] % VEC:                                  # the wide flip behind the narrow row kernels
        out.add(prefix + ":wide:rows-unaligned")
    return out


def _count_blocks(prefix, count, what="blocks"):
    if count is None or count < 1:
        return set()
    return {f"{prefix}:{what}" + ("==1" if count <= BLOCK else ">=2")}  # (count + kBlock - 1) / kBlock workgroups, or i += kBlock


def edit_voxels(dims, box="whole"):
    """rto_edit_voxels.  box: "whole" (a brush over the whole grid), "outside", or ((x0, y0, z0), (x1, y1, z1)) inclusive."""
    if box == "outside":
        return {"edit_voxels:nothing-inside"}                           # n == 0 || box[0] > box[3]
    lo, hi = ((0, 0, 0), tuple(d - 1 for d in dims)) if box == "whole" else box
    runs = (hi[0] + 1 - (lo[0] & ~(VEC - 1)) + VEC - 1) // VEC          # eb.runsX from eb.x0 = box[0] & ~15
    return {"edit_brushes:" + ("wide" if dims[0] % VEC == 0 else "narrow"),                  # dims[0] % kEditRun == 0
            "edit_brushes:blocks-x" + ("==1" if runs <= 16 else ">=2"),                      # eb.blocksX = ceil(runsX / kEditRunsX)
            "edit_brushes:blocks-y" + ("==1" if hi[1] - lo[1] + 1 <= 16 else ">=2")}         # eb.blocksY = ceil(rows / kEditRowsY)


def label(dims, count=None):
    """rto_label_components.  count: the components of the labelled set, None when the caller does not know it."""
    n = _voxels(dims)
    out = _row_kernel("cc_local", dims, "chunk-beyond-row")
    out.add("cc_scan:rounds" + ("==1" if (n + CHUNK - 1) // CHUNK <= BLOCK else ">=2"))      # i0 += THREADS over the chunks
    out.add("cc_stats:" + ("all-whole" if n % 32 == 0 else "tail-partial"))                  # v0 + kCcStatPerThread <= D.n
    if count == 0:
        out.add("cc_label:count==0")                                    # if (total)
    return out | _count_blocks("cc_touches", count)


def edit_components(dims, count=None, select=None):
    """rto_edit_components: the labelling, then the selection and the flip."""
    out = label(dims, count)
    if count == 0:
        return out | {"edit_components:count==0"}                       # if (r.count == 0) return RTO_OK
    if select == ALL_BUT_LARGEST:
        out |= _count_blocks("cc_largest", count, "rounds")             # i += kBlock
    return out | _count_blocks("cc_select", count) | _flip("cc_flip", dims)


def distance(dims):
    """rto_distance_field: dt_transform."""
    x, y, z = dims
    out = {"dt_x:" + ("wide" if x % VEC == 0 else "narrow")}            # D.x % kCcVec == 0
    if x % VEC == 0 and x % 32 == VEC:
        out.add("dt_x:wide:piece-beyond-row")                           # x0 + 16 * h < D.x fails in the row's last word
    per_block = max(1, DT_ROW_VOX // x)                                 # rowsPerBlock = max(1, kDtRowVox / D.x)
    rows = min(per_block, y * z)                                        # rows of the first workgroup
    words = rows * ((x + 31) // 32)                                     # words = rows * rowWords
    out.add("dt_x:rows-per-block" + ("==1" if per_block == 1 else ">=2"))
    out.add("dt_x:" + ("last-block-short" if (y * z) % per_block else "blocks-all-full"))    # min(rowsPerBlock, numRows - row0)
    out.add("dt_x:mask-rounds" + ("==1" if words <= BLOCK else ">=2"))  # i += kBlock
    out.add("dt_x:sweep-rounds" + ("==1" if rows <= BLOCK else ">=2"))  # r += kBlock
    return out


def morphology(dims):
    """rto_edit_morphology with a radius in reach: dt_transform, then k_morph_flip."""
    return distance(dims) | _flip("morph_flip", dims)


def geodesic(dims, seeds=1):
    """rto_geodesic_field with `seeds` seeds."""
    out = _row_kernel("geo_relax", dims, "chunk-beyond-row")
    out.add("geo_fill:" + ("all-whole" if _voxels(dims) % VEC == 0 else "tail-partial"))     # v0 + kCcVec <= n
    return out | _count_blocks("geo_seeds", seeds)


def edit_geodesic(dims, seeds=1):
    """rto_edit_geodesic: the field, then k_morph_flip."""
    return geodesic(dims, seeds) | _flip("morph_flip", dims)


def thickness(dims):
    """rto_thickness_field: dt_transform, then the gather."""
    return distance(dims) | {"thick_gather:" + ("column-beyond-grid" if _off_tile(dims) else "tiles-all-inside")}    # inXY && z0 + j < D.z


def measure(dims, count=None):
    """rto_measure_components on a labelling of `count` components."""
    if count == 0:
        return {"measure:count==0"}                                     # if (count)
    out = _row_kernel("measure", dims, "segment-beyond-row")
    tx, ty, tz = _tiles(dims)
    out.add("measure_fold:blocks" + ("==1" if tx * ty * tz <= BLOCK else ">=2"))             # (tiles + kBlock - 1) / kBlock
    if count is not None:
        out.add("measure_total:round" + ("==1" if count <= TOTAL_CAP * BLOCK else ">=2"))    # min(ceil(count / kBlock), 1024u) workgroups
    return out


def skeleton(dims, anchors=0, summary=True):
    """rto_skeleton_field (summary: k_skel_summary runs) or rto_edit_skeleton (it does not)."""
    x = dims[0]
    out = {"skel_init:" + ("wide" if x % 32 == 0 else "narrow"),                             # D.x % 32 == 0
           "skel_window:words-per-row" + ("==1" if x <= 32 else ">=2"),                      # wx > 0, wx + 1 < D.wordsX
           "skel_step:" + ("voxel-beyond-grid" if _off_tile(dims) else "tiles-all-inside")}  # gx < D.x && gy < D.y && gz < D.z
    out |= _count_blocks("skel_anchors", anchors) if anchors else {"skel_anchors:none"}      # if (n > 0)
    if summary:
        out.add("skel_summary:round" + ("==1" if _voxels(dims) <= SUMMARY_CAP * BLOCK else ">=2"))   # min(ceil(nvox / kBlock), 4096u)
    return out


def edit_skeleton(dims, anchors=0):
    return skeleton(dims, anchors, summary=False)
