"""rto_build_leaf_triangles at its thread, wave and chunk edges, on the small grids of tests/leaftri_families.py.

The builder (csrc/rto_device.hip.h, k_leaftri_*) walks a leaf's candidate cells with one thread (total <= 64), one wave
(64 < total <= 2048) or one wave per chunk of 2048 candidates (above), and enumerates them with one form per clip mask.

CPU: a numpy statement of which cells of a leaf can emit (localMC's loop bounds `c < c0 + size && c < dim - 1`, and a uniform leaf's
cells reading corners c .. c + 1) gives every leaf's candidate list, total and mask; the oracle's localMC emits in a subset of that
list and in its order; the families reach every (class, mask) cell and the threshold totals; the product's C++ builder equals the
oracle's.  GPU: the builder's bytes against the oracle's for both sources of the octree, rebuilt twice, read back through the mesh
extraction, after edits that split and restore a several-chunk leaf, and rendered."""
from __future__ import annotations

import numpy as np
import pytest

import leaftri_families as fam
import mesh_ref as mr

gpu = pytest.mark.gpu
SERIAL_MAX, CHUNK = 64, 2048              # the builder's two thresholds, as the design states them
CLASSES = ("serial", "wave", "chunks")
SOURCES = ("upload", "build")


# ================================================================ the rule: which cells of a leaf can emit, in which order
def leaf_extents(x0, y0, z0, s, dims):
    """Cells localMC visits in a leaf per axis: c < c0 + size && c < dim - 1."""
    return tuple(np.maximum(0, np.minimum(c0 + s, d - 1) - c0) for c0, d in zip((x0, y0, z0), dims))


def leaf_totals(nodes, dims):
    """(total, mask) per node, -1 for nodes that are no leaves.  A cell whose local index is below size - 1 on every axis reads
    eight voxels of the (uniform) leaf and cannot emit: total = visited cells - those."""
    s = nodes["size"].astype(np.int64)
    ex, ey, ez = leaf_extents(nodes["x"].astype(np.int64), nodes["y"].astype(np.int64), nodes["z"].astype(np.int64), s, dims)
    inner = np.minimum(ex, s - 1) * np.minimum(ey, s - 1) * np.minimum(ez, s - 1)
    total = ex * ey * ez - inner
    mask = (ex == s).astype(np.int64) | (ey == s).astype(np.int64) << 1 | (ez == s).astype(np.int64) << 2
    mask[total == 0] = 0                                   # nothing to enumerate: no form is chosen
    leaf = nodes["isLeaf"] == 1
    return np.where(leaf, total, -1), np.where(leaf, mask, -1)


def leaf_candidates(x0, y0, z0, s, dims):
    """Candidate cells of one leaf as local (i, j, k) rows in localMC's loop order (z slowest, x fastest)."""
    ex, ey, ez = (int(e) for e in leaf_extents(x0, y0, z0, s, dims))
    if ex == 0 or ey == 0 or ez == 0:
        return np.zeros((0, 3), np.int64)
    k, j, i = np.mgrid[0:ez, 0:ey, 0:ex]
    on = (i == s - 1) | (j == s - 1) | (k == s - 1)
    return np.stack([i[on], j[on], k[on]], 1)


def leaf_class(total):
    return "none" if total <= 0 else "serial" if total <= SERIAL_MAX else "wave" if total <= CHUNK else "chunks"


def triangle_cells(tris, grid_min, voxel):
    """The cell of every triangle: its vertices are midpoints of one cell's edges, so the centroid lies strictly inside it."""
    v = np.asarray(tris, np.float32)[:, :9].astype(np.float64).reshape(-1, 3, 3)
    c = ((v - np.asarray(grid_min, np.float64)) / float(voxel)).mean(1)
    assert (np.abs(c - np.round(c)) > 0.1).all(), "a triangle lies in a cell's face: its cell cannot be told from its centroid"
    return np.floor(c).astype(np.int64)


class Family:
    def __init__(self, orc, name):
        self.case = fam.make(name)
        self.name, self.dims, self.data = name, self.case.dims, self.case.data
        self.min, self.vs = self.case.grid_min, self.case.voxel_size
        self.grid = orc.Grid(self.dims, self.min, self.vs, self.data)
        self.nodes = orc.build_flat_octree(self.grid)
        self.tris, self.off = orc.build_leaf_triangles(self.grid, self.nodes)
        self.total, self.mask = leaf_totals(self.nodes, self.dims)
        self._mesh = None

    def mesh(self):
        if self._mesh is None:
            self._mesh = mr.extract(mr.MESH_MC, self.nodes, self.min, self.vs, tris=self.tris, tri_offset=self.off)
        return self._mesh

    def describe(self, i):
        nd = self.nodes[i]
        t = int(self.total[i])
        return (f"node {i} at ({nd['x']}, {nd['y']}, {nd['z']}) size {nd['size']} isLeaf {nd['isLeaf']}: mask {int(self.mask[i])}, "
                f"total {t}, class {leaf_class(t)}")


@pytest.fixture(scope="module")
def families(orc):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Family(orc, name)
        return cache[name]
    return get


def _node_at(f, x0, y0, z0, s):
    n = f.nodes
    hit = np.nonzero((n["x"] == x0) & (n["y"] == y0) & (n["z"] == z0) & (n["size"] == s))[0]
    assert len(hit) == 1, f"{f.name}: no node at ({x0}, {y0}, {z0}) of size {s}"
    return int(hit[0])


# ================================================================ CPU
def test_families_are_small_and_seeded():
    for name in fam.NAMES:
        a, b = fam.make(name), fam.make(name)
        assert a.data.tobytes() == b.data.tobytes() and a.data.shape == a.dims[::-1] and a.data.dtype == np.uint8
        assert a.data.size <= 300_000, (name, a.data.size)
        assert a.grid_min.dtype == np.float32 and a.grid_min.tobytes() == fam.GRID_MIN.tobytes() and a.voxel_size == fam.VOXEL


@pytest.mark.parametrize("name", fam.NAMES)
def test_oracle_emits_inside_the_candidate_list_in_its_order(orc, families, name):
    """For every leaf: the cells where localMC emits triangles are candidates and come in the candidates' order; over the grid they
    are exactly the cells whose eight corners are not all alike."""
    f = families(name)
    leaves = np.nonzero(f.nodes["isLeaf"] == 1)[0]
    assert (np.diff(f.off)[f.nodes["isLeaf"] != 1] == 0).all()
    cells = triangle_cells(f.tris, f.min, f.vs)
    owner = np.repeat(np.arange(len(f.nodes)), np.diff(f.off))
    # leaves of one voxel: the candidate list is the voxel's own cell when dim - 1 leaves it, else empty
    one = f.nodes["size"][owner] == 1
    o1 = owner[one]
    assert (f.total[o1] == 1).all()
    assert (cells[one] == np.stack([f.nodes["x"][o1], f.nodes["y"][o1], f.nodes["z"][o1]], 1)).all()
    # larger leaves: the list itself, against localMC on that leaf
    dx, dy = f.dims[0], f.dims[1]
    seen = 0
    for i in leaves[f.nodes["size"][leaves] > 1]:
        nd = f.nodes[i]
        x0, y0, z0, s = int(nd["x"]), int(nd["y"]), int(nd["z"]), int(nd["size"])
        cand = leaf_candidates(x0, y0, z0, s, f.dims)
        assert len(cand) == f.total[i], f.describe(i)
        ckey = ((cand[:, 2] + z0) * dy + cand[:, 1] + y0) * dx + cand[:, 0] + x0
        assert (np.diff(ckey) > 0).all()                                  # loop order = increasing z, y, x
        lm = orc.local_mc(f.grid, x0, y0, z0, s)
        assert lm[:, :9].tobytes() == f.tris[f.off[i]:f.off[i + 1], :9].tobytes(), f.describe(i)
        if len(lm) == 0:
            continue
        ec = triangle_cells(lm, f.min, f.vs)
        ekey = (ec[:, 2] * dy + ec[:, 1]) * dx + ec[:, 0]
        assert (np.diff(ekey) >= 0).all(), f.describe(i)                  # a cell's triangles are consecutive, cells in loop order
        assert np.isin(ekey, ckey).all(), f.describe(i)
        seen += 1
    # the whole grid: emitting cells == cells with mixed corners
    d = f.data
    if min(d.shape) > 1:
        c8 = [d[a:d.shape[0] - 1 + a, b:d.shape[1] - 1 + b, c:d.shape[2] - 1 + c] for a in (0, 1) for b in (0, 1) for c in (0, 1)]
        mixed = np.minimum.reduce(c8) != np.maximum.reduce(c8)
        want = np.argwhere(mixed)[:, ::-1]
    else:
        want = np.zeros((0, 3), np.int64)
    got = np.unique(cells, axis=0) if len(cells) else np.zeros((0, 3), np.int64)
    assert got.shape == want.shape and (got[np.lexsort(got.T)] == want[np.lexsort(want.T)]).all()
    if name not in fam.DEGENERATE:
        assert seen > 0 and len(f.tris) > 0
    else:
        assert len(f.tris) == 0 and not f.off.any()
        assert (f.total <= 0).all() == (name != "all_filled")             # all_filled has candidates; none of them emits


def test_families_reach_every_class_mask_and_threshold(families):
    """A condition on the inputs, from the oracle's octree alone: each family holds the leaf its table row promises; together
    they put every mask 1 .. 7 into each of the three classes and hit the totals 64, 65, 2048 and one in (2048, 2048 + 64).
    No (class, mask) cell is impossible: a leaf of edge 4, 16 or 64 cut on the right axes reaches each (corner4, corner16, the
    chunks_mask* grids).  Mask 0 (every axis cut) always has total 0 and belongs to no class."""
    reached = {}
    totals = set()
    for name in fam.NAMES:
        f = families(name)
        for x0, y0, z0, s, total, mask in fam.BLOCKS[name]:
            i = _node_at(f, x0, y0, z0, s)
            assert f.nodes["isLeaf"][i] == 1, f.describe(i)
            assert (int(f.total[i]), int(f.mask[i])) == (total, mask), f.describe(i)
            assert len(leaf_candidates(x0, y0, z0, s, f.dims)) == total
        leaf = f.total >= 0
        assert (f.total[leaf & (f.mask == 0)] == 0).all()
        for t, m in set(zip(f.total[leaf].tolist(), f.mask[leaf].tolist())):
            if t > 0:
                reached.setdefault((leaf_class(t), m), set()).add(name)
                totals.add(t)
    for cls in CLASSES:
        for m in range(1, 8):
            print(f"{cls:7s} mask {m}: {sorted(reached.get((cls, m), ()))}")
    missing = [(cls, m) for cls in CLASSES for m in range(1, 8) if (cls, m) not in reached]
    assert not missing, missing
    for m in range(1, 8):                                                 # each several-chunk cell by a grid made for it
        own = {4: "chunk2080_mask4"}.get(m, f"chunks_mask{m}")
        assert own in reached[("chunks", m)], m
    assert {SERIAL_MAX, SERIAL_MAX + 1, CHUNK} <= totals
    assert any(CHUNK < t < CHUNK + 64 for t in totals)                    # a last chunk shorter than one wave
    print("threshold totals:", sorted(t for t in totals if t in (64, 65, 2048) or CHUNK < t < CHUNK + 64))
    # clipped several-chunk leaves are cut by more than one voxel; one several-chunk leaf sits away from the origin
    for m in (1, 2, 3, 5, 6):
        x0, y0, z0, s, _, _ = fam.BLOCKS[f"chunks_mask{m}"][0]
        ext = leaf_extents(x0, y0, z0, s, families(f"chunks_mask{m}").dims)
        assert all(e == s or e < s - 1 for e in ext) and any(e < s - 1 for e in ext)
    assert min(fam.BLOCKS["chunks_offorigin"][0][:3]) > 0
    # the big list (leaves above the serial limit) spans two workgroups of 256 on the checkerboard
    cb = families("checkerboard")
    assert int((cb.total > SERIAL_MAX).sum()) == 490 and len(cb.nodes) == 585
    # both polarities on every class
    for c, cls in enumerate(CLASSES):
        solid = set()
        for name in fam.NAMES:
            f = families(name)
            sel = (np.searchsorted([1, SERIAL_MAX + 1, CHUNK + 1], f.total, side="right") == c + 1) & (np.diff(f.off) > 0)
            solid |= set(f.nodes["isSolid"][sel].tolist())
        assert solid == {0, 1}, (cls, solid)


@pytest.mark.parametrize("name", fam.NAMES)
def test_host_builder_equals_the_oracle(orc, families, name):
    import ray_tracing_octrees_amd as rto
    f = families(name)
    g = rto.VoxelGrid.from_array(f.data, f.min, f.vs)
    tris, off = rto.buildLeafTriangles(g, f.nodes)
    assert off.tobytes() == f.off.tobytes(), name
    assert np.asarray(tris, np.float32).reshape(-1, 12).tobytes() == f.tris.tobytes(), name
    if name in fam.DEGENERATE:
        assert len(tris) == 0 and not np.asarray(off).any()


# ================================================================ GPU
def _resident(ctx, f, source, data=None):
    """The family's octree resident from `source`, its leaf triangles built on the GPU."""
    from ray_tracing_octrees_amd import hip
    data = f.data if data is None else data
    ctx.set_kernel(hip.KERNEL_AUTO)
    if source == "upload":
        ctx.upload_octree(f.nodes, f.min, f.vs)
        ctx.build_leaf_triangles(data)
    else:
        ctx.build_octree(data, f.min, f.vs)
        ctx.build_leaf_triangles(None)


def _assert_buffer(f, got, want_tris, want_off, what):
    """got = download_leaf_triangles(); on a mismatch name the first differing node with its size, mask, total and class."""
    gt, go = got
    want_off = np.asarray(want_off, np.int32)
    want_tris = np.ascontiguousarray(want_tris, np.float32).reshape(-1, 12)
    assert go.shape == want_off.shape, f"{what}: triOffset has {go.shape} entries, the oracle's {want_off.shape}"
    if go.tobytes() != want_off.tobytes():
        p = int(np.nonzero(go != want_off)[0][0])                         # offset p is wrong: node p - 1 has the wrong count
        i = max(p - 1, 0)
        raise AssertionError(f"{what}: triOffset[{p}] = {go[p]}, the oracle's {want_off[p]}; first wrong count at {f.describe(i)}")
    assert gt.shape == want_tris.shape, f"{what}: {gt.shape} vs {want_tris.shape}"
    if gt.tobytes() != want_tris.tobytes():
        t = int(np.nonzero((gt.view(np.uint32) != want_tris.view(np.uint32)).any(1))[0][0])
        i = int(np.searchsorted(want_off, t, side="right")) - 1
        raise AssertionError(f"{what}: triangle {t} (number {t - want_off[i]} of {want_off[i + 1] - want_off[i]} in its leaf) differs; "
                             f"{f.describe(i)}")


@gpu
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("name", fam.NAMES)
def test_gpu_builder_equals_the_oracle(ctx, families, name, source):
    f = families(name)
    _resident(ctx, f, source)
    if source == "build":
        assert ctx.download_nodes().tobytes() == f.nodes.tobytes()
    _assert_buffer(f, ctx.download_leaf_triangles(), f.tris, f.off, f"{name} {source}")
    if name in fam.DEGENERATE:
        gt, go = ctx.download_leaf_triangles()
        assert gt.shape == (0, 12) and not go.any()


@gpu
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("name", fam.NAMES)
def test_gpu_rebuilds_give_the_same_bytes(ctx, families, name, source):
    """Three builds in one context: the order the atomics gave the big list and the scratch pool's reuse do not show."""
    f = families(name)
    _resident(ctx, f, source)
    first = ctx.download_leaf_triangles()
    for rep in (1, 2):
        ctx.build_leaf_triangles(f.data if source == "upload" else None)
        again = ctx.download_leaf_triangles()
        _assert_buffer(f, again, f.tris, f.off, f"{name} {source} build {rep + 1}")
        assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()


@gpu
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("name", fam.NAMES)
def test_gpu_mesh_extraction_reads_the_long_ranges(ctx, families, name, source):
    """RTO_MESH_MC without planes = the oracle's buffer in depth-first order (tests/mesh_ref.py): k_mesh_emit_mc's binary search
    over triOffset across the ranges of several-chunk leaves."""
    from ray_tracing_octrees_amd import hip
    f = families(name)
    _resident(ctx, f, source)
    want, wnode = f.mesh()
    got, gnode = ctx.extract_mesh(hip.MESH_MC, None, 0.0)
    assert len(got) == len(want) == len(f.tris), name
    if gnode.tobytes() != wnode.tobytes():
        t = int(np.nonzero(gnode != wnode)[0][0])
        raise AssertionError(f"{name} {source}: mesh triangle {t} belongs to node {gnode[t]}, the rule's {wnode[t]}; {f.describe(int(wnode[t]))}")
    if got.tobytes() != want.tobytes():
        t = int(np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))[0][0])
        raise AssertionError(f"{name} {source}: mesh triangle {t} differs; {f.describe(int(wnode[t]))}")


@gpu
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("name", sorted(fam.EDIT_VOXEL))
def test_gpu_edit_splits_and_restores_a_several_chunk_leaf(ctx, orc, families, name, source):
    """FILL one voxel inside the uniform EMPTY block: the block splits into leaves of every smaller edge, serial and wave ones
    among them (chunks_mask7: nothing stays on the chunk path; chunk2080_mask4: its 64^3 child cut to 32 x 64 does, at 4064);
    CARVE it again.  After each edit the resident triangles are the oracle's for the edited grid; the final state is the first
    build's bytes."""
    import edit_ref as er
    from ray_tracing_octrees_amd import hip
    f = families(name)
    x0, y0, z0, s, total, _ = fam.BLOCKS[name][0]
    vx = fam.EDIT_VOXEL[name]
    assert total > CHUNK and all(o <= v < min(o + s, d) for v, o, d in zip(vx, (x0, y0, z0), f.dims)) and f.data[vx[2], vx[1], vx[0]] == 0
    ctx.set_kernel(hip.KERNEL_AUTO)
    ctx.build_octree(f.data, f.min, f.vs)                                 # edits need the resident grid
    if source == "build":
        ctx.build_leaf_triangles(None)
    else:
        ctx.upload_leaf_triangles(f.tris, f.off)
    centre = (np.asarray(f.min, np.float64) + (np.asarray(vx, np.float64) + 0.5) * float(f.vs)).astype(np.float32)
    cur = f.data
    for op in (er.FILL, er.CARVE):
        b = hip.make_brushes([centre], np.float32(0.5 * float(f.vs)), er.SPHERE, op)
        want, changed = er.apply(cur, b, f.min, f.vs)
        assert changed == 1 and want[vx[2], vx[1], vx[0]] == (1 if op == er.FILL else 0)
        assert ctx.edit_voxels(b) == 1
        e = Family.__new__(Family)                                        # the edited grid's own oracle state, for the report
        e.name, e.dims, e.min, e.vs = f"{name} after {'FILL' if op == er.FILL else 'CARVE'}", f.dims, f.min, f.vs
        e.grid = orc.Grid(f.dims, f.min, f.vs, want)
        e.nodes = orc.build_flat_octree(e.grid)
        e.tris, e.off = orc.build_leaf_triangles(e.grid, e.nodes)
        e.total, e.mask = leaf_totals(e.nodes, e.dims)
        if op == er.FILL:
            inside = (e.nodes["x"] < x0 + s) & (e.nodes["y"] < y0 + s) & (e.nodes["z"] < z0 + s) & (e.nodes["isLeaf"] == 1)
            assert len(e.nodes) > len(f.nodes) and e.nodes["size"][inside].max() < s      # the block did split
            assert {leaf_class(int(t)) for t in e.total[inside]} >= {"serial", "wave"}
        assert ctx.download_nodes().tobytes() == e.nodes.tobytes(), e.name
        _assert_buffer(e, ctx.download_leaf_triangles(), e.tris, e.off, f"{e.name} {source}")
        cur = want
    assert cur.tobytes() == f.data.tobytes()
    _assert_buffer(f, ctx.download_leaf_triangles(), f.tris, f.off, f"{name} {source}: restored")


@gpu
def test_gpu_built_triangles_render_the_oracles_frame(ctx, orc, families):
    """One 160 x 120 shadowed frame of chunks_mask7 from the GPU-built buffer, bit for bit the oracle's on its own buffer."""
    from conftest import assert_bit_exact
    from ray_tracing_octrees_amd import hip
    f = families("chunks_mask7")
    _resident(ctx, f, "build")
    W, H = 160, 120
    cam = orc.Camera(0.5, 0.7, 32.0)
    cam.set_target(*[float(v) for v in f.min + np.float32(0.5) * np.array(f.dims, np.float32) * f.vs])
    view, pos = cam.get_view(), cam.get_pos()
    want, st = orc.render_triangles(f.nodes, f.tris, f.off, f.min, f.vs, view, pos, W / H, 45.0, W, H, shadow=True,
                                    nthreads=min(16, orc.max_threads()))
    assert st["hits"] > W * H // 10
    frame = hip.make_frame(view, pos, W / H, 45.0, W, H)
    got, gs = ctx.render_triangles_host(frame, shadow=True, stats=True)
    assert_bit_exact(got, want, "chunks_mask7: shadowed triangle frame from the GPU-built buffer")
    assert (gs["pops"], gs["hits"]) == (st["pops"], st["hits"])
