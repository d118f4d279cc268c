"""The frustum states and scenes of tests/test_frustum_states.py as data ("Entry points under a frustum
update"), and the search for a grid origin whose root box ends an ulp below a child's.  Imports no library: the functions take
numpy and a seeded generator from their caller."""

FOV = 45.0
FRAMES = ((96, 64), (100, 60))          # 100 x 60: the last 8 x 8 tile column and row are partial
BIG_FRAME = (64, 64)                    # scene C's one frame per state

# A plane (nx, ny, nz, d) keeps a box whose positive vertex p has n . p + d >= 0.
KEEP = (0.0, 0.0, 0.0, 1.0)             # 0 . p + 1 >= 0: keeps every box
STATES = ("OFF", "HALF", "NONE", "ROOTLESS")
NONE_PLANES = ((1.0, 0.0, 0.0, -1.0e6),) + (KEEP,) * 5        # x >= 1e6: culls the root and everything under it

# scene -> (kind, argument).  A: exact grid (sphere64's origin and voxel are powers of two); B: the seeded 16^3 grids of
# test_culled_root_with_surviving_descendants_follows_the_reference, not exact; C: a 128^3 checkerboard, 2,396,745 nodes of
# which 299,593 are internal (1,171 workgroups of k_cull_desc, 9,363 blocks of flags); D: the oracle's compaction of sphere64
# under D_SOURCE_PLANES, uploaded as a non-canonical array.
SCENES = {
    "A": ("sphere", 64),
    "B-leaf": ("rootless16", "solid leaf"),
    "B-internal": ("rootless16", "internal node"),
    "C": ("checker", 128),
    "D": ("compacted", "A"),
}
FRAME_SCENES = ("A", "B-leaf", "B-internal", "D")
GRID_SCENES = ("A", "B-leaf", "B-internal")                   # built with rto_build_octree: the grid is resident
ROOTLESS_SCENES = ("B-leaf", "B-internal", "C")
SEARCH_SEED = 4                          # the seed of the test the search comes from
C_SEARCH_SEED = 4
D_SOURCE_PLANES = ((-1.0, 0.0, 0.0, 0.0),) + (KEEP,) * 5      # x <= 0: the half of sphere64 that holds HALF's slab

# HALF on sphere64: the planes the query suites use, x >= -0.45 and x <= -0.40 (421 of 23,561 nodes survive, the root among them)
HALF_SPHERE = ((1.0, 0.0, 0.0, 0.45), (-1.0, 0.0, 0.0, -0.40), (0.0, 1.0, 0.0, 0.5), (0.0, -1.0, 0.0, 0.5), (0.0, 0.0, 1.0, 0.5),
               (0.0, 0.0, -1.0, 0.5))
HALF_SLAB = (0.05, 0.10)                 # elsewhere: the slab's faces as fractions of the root box's edge, from its low x face

# the lit renders' settings and the camera of every scene: Camera(theta, phi, radius in root-box edges) aimed at the box's centre
LIGHT = dict(light_dir=(0.3, -0.8, 0.45), shadow=True, ao_samples=4, seed=7)
AO_RADIUS_VOXELS = 4.0
CAMERA = (0.6, 0.8, 1.4)
RAYS, RAY_SEED = 2048, 31
MIN_CHANGED_PIXELS = 0.01                # of the frame, between a state's oracle frame and OFF's
MIN_CULLED_HITS = 0.25                   # of the rays that hit under OFF: their leaf is culled under HALF


def states_of(scene):
    return tuple(s for s in STATES if s != "ROOTLESS" or scene in ROOTLESS_SCENES)


def half_planes(scene, grid_min_x, edge):
    """HALF's six planes for a scene whose root box starts at grid_min_x and is `edge` long."""
    if SCENES[scene][0] in ("sphere", "compacted"):
        return HALF_SPHERE
    lo, hi = grid_min_x + HALF_SLAB[0] * edge, grid_min_x + HALF_SLAB[1] * edge
    return ((1.0, 0.0, 0.0, -lo), (-1.0, 0.0, 0.0, hi)) + (KEEP,) * 4


def rootless_planes(axis, child_max):
    """The construction's plane: n = +axis through the surviving child's max plane (margin 0), five planes that keep everything."""
    first = [0.0, 0.0, 0.0, -float(child_max)]
    first[axis] = 1.0
    return (tuple(first),) + (KEEP,) * 5


def search_origin(np, rng, dim, first_survivor):
    """A grid origin and voxel size for a dim^3 grid at which the frustum test can drop the ROOT and keep descendants.  Nested
    boxes make that impossible in exact arithmetic; in float it needs a corner where the root's nodeMax and a child's differ by an
    ulp: gridMin + 0*vs + dim*vs against (gridMin + (dim/2)*vs) + (dim/2)*vs.  "internal node": the far quarter (x = 3 dim/4, size
    dim/4) must stick out of the root as well, so that the solid leaves under the first survivor survive too.  Draws from rng
    until one is found; returns (gridMin, vs, axis, the root's max, the plane's offset) or None after 4000 draws."""
    f32 = np.float32
    half, quarter = dim // 2, dim // 4
    for _ in range(4000):
        gmin = rng.uniform(-60, 60, 3).astype(f32)
        vs = f32(rng.choice([0.7, 3.3, 0.37, 1.9])) if first_survivor == "solid leaf" else f32(rng.uniform(0.2, 4.0))
        for a in range(3):
            root_mx = f32(f32(gmin[a] + f32(0) * vs) + f32(dim) * vs)
            child_mx = f32(f32(gmin[a] + f32(half) * vs) + f32(half) * vs)
            quarter_mx = f32(f32(gmin[a] + f32(dim - quarter) * vs) + f32(quarter) * vs)
            if child_mx > root_mx and (first_survivor == "solid leaf" or quarter_mx > root_mx):
                return gmin, vs, a, root_mx, child_mx if first_survivor == "solid leaf" else min(child_mx, quarter_mx)
    return None


def rootless16_data(np, rng, axis, first_survivor):
    """The 16^3 voxels of the construction, [z][y][x]: 35 % noise; the root's child on the far side of `axis` that comes first in
    BFS order (octant 1 << axis) lands at index 0 of the compacted array, where the reference's traversal starts: a solid leaf,
    or a mixed cell (near half noise, far half solid) so that the traversal starts at an internal node."""
    data = (rng.random((16, 16, 16)) < 0.35).astype(np.uint8)
    sl = [slice(0, 8)] * 3
    sl[2 - axis] = slice(8, 16)
    if first_survivor == "solid leaf":
        data[tuple(sl)] = 1
    else:
        data[tuple(sl)] = (rng.random((8, 8, 8)) < 0.5).astype(np.uint8)
        sl[2 - axis] = slice(12, 16)
        data[tuple(sl)] = 1
    return data
