"""numpy statement of the mesh voxelization rule (include/rto_hip.h, rto_voxelize_mesh), the reference's
loadCSVDataIntoVoxelGrid (453-skeleton/BuildingLoader.cpp:131-290) and recenterFilledVoxels (main.cpp:376-422).  The grid is
computed in float64 like the reference; every per-face and per-voxel step in float32, one IEEE operation per line.  Used by the
CPU and GPU tests where a committed fixture would be too large."""
from __future__ import annotations

import numpy as np

f32 = np.float32
MAX_DIM = 1000


def auto_grid(xyz, n_tris, voxel_size):
    """(dims (x, y, z), grid_min float32[3], voxel_size float32) of the AUTO rule, or None for the reference's empty grid."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    if len(xyz) == 0 or n_tris == 0:
        return None
    fin = np.isfinite(xyz).all(axis=1)
    if not fin.any():
        return None
    vs = f32(voxel_size)
    pad = float(vs)
    mn = xyz[fin].min(axis=0) - pad
    mx = xyz[fin].max(axis=0) + pad
    dims = [int(np.ceil((mx[a] - mn[a]) / float(vs))) for a in range(3)]
    if max(dims) > MAX_DIM:
        scale = f32(max(d // MAX_DIM for d in dims))           # integer division: 1001..1999 gives 1
        vs = f32(vs * scale)
        dims = [int(np.ceil((mx[a] - mn[a]) / float(vs))) for a in range(3)]
    return tuple(dims), mn.astype(np.float32), vs


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz       # float32 arrays: each product and sum rounds to float32


def face_terms(xyz, tris, gmin, vs, dims):
    """Per face: lo (int64 [nf, 3]), n (int64 [nf, 3], 0 on some axis = no voxels), a, e0, e1 (float32 [nf, 3]), d00, d01, d11,
    inv (float32 [nf]), and `bad` (a finite face whose int casts would overflow: the call is refused)."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    v = xyz[tris].astype(np.float32)                           # [nf, 3 vertices, 3 axes]
    finite = np.isfinite(v).all(axis=(1, 2))
    gmin = np.asarray(gmin, np.float32)
    vs = f32(vs)
    with np.errstate(all="ignore"):
        tmin = v.min(axis=1)
        tmax = v.max(axis=1)
        ts = (tmin - gmin) / vs
        te = (tmax - gmin) / vs
        ok = (ts >= f32(-2147483648.0)) & (ts < f32(2147483648.0)) & (te >= f32(-2147483648.0)) & (te < f32(2147483648.0))
        bad = finite & ~ok.all(axis=1)
        ts = np.where(ok, ts, 0).astype(np.float32)
        te = np.where(ok, te, 0).astype(np.float32)
        s = np.maximum(0, np.trunc(ts).astype(np.int64))
        e = np.minimum(np.asarray(dims, np.int64) - 1, np.trunc(te).astype(np.int64) + 1)
        a = v[:, 0]
        e0 = v[:, 2] - v[:, 0]
        e1 = v[:, 1] - v[:, 0]
        d00 = _dot(e0[:, 0], e0[:, 1], e0[:, 2], e0[:, 0], e0[:, 1], e0[:, 2])
        d01 = _dot(e0[:, 0], e0[:, 1], e0[:, 2], e1[:, 0], e1[:, 1], e1[:, 2])
        d11 = _dot(e1[:, 0], e1[:, 1], e1[:, 2], e1[:, 0], e1[:, 1], e1[:, 2])
        denom = d00 * d11 - d01 * d01
        degenerate = np.abs(denom) < f32(1e-7)
        inv = f32(1.0) / denom
    n = np.maximum(e - s + 1, 0)
    keep = finite & ~bad & ~degenerate
    n[~keep] = 0
    return dict(lo=s, n=n, a=a, e0=e0, e1=e1, d00=d00, d01=d01, d11=d11, inv=inv, bad=bool(bad.any()))


def fill(xyz, tris, gmin, vs, dims, chunk=1 << 22):
    """The grid (uint8 [dimZ, dimY, dimX]) and the number of (face, voxel) pairs tested; raises ValueError where the library
    refuses the mesh."""
    T = face_terms(xyz, tris, gmin, vs, dims)
    if T["bad"]:
        raise ValueError("a face's voxel box overflows int")
    dims = tuple(int(d) for d in dims)
    out = np.zeros(dims[0] * dims[1] * dims[2], np.uint8)
    gmin = np.asarray(gmin, np.float32)
    vs = f32(vs)
    cnt = T["n"].prod(axis=1)
    faces = np.nonzero(cnt)[0]
    pairs = int(cnt.sum())
    i = 0
    while i < len(faces):
        # a chunk of faces with at most `chunk` pairs (at least one face)
        csum = np.cumsum(cnt[faces[i:]])
        j = i + max(1, int(np.searchsorted(csum, chunk, side="right")))
        fs = faces[i:j]
        c = cnt[fs]
        fi = np.repeat(fs, c)
        q = np.arange(int(c.sum()), dtype=np.int64) - np.repeat(np.cumsum(c) - c, c)
        n = T["n"][fi]
        x = q % n[:, 0]
        y = (q // n[:, 0]) % n[:, 1]
        z = q // (n[:, 0] * n[:, 1])
        ijk = np.stack([x, y, z], axis=1) + T["lo"][fi]
        p = gmin + (ijk.astype(np.float32) + f32(0.5)) * vs
        w = p - T["a"][fi]
        e0, e1 = T["e0"][fi], T["e1"][fi]
        with np.errstate(all="ignore"):
            d02 = _dot(e0[:, 0], e0[:, 1], e0[:, 2], w[:, 0], w[:, 1], w[:, 2])
            d12 = _dot(e1[:, 0], e1[:, 1], e1[:, 2], w[:, 0], w[:, 1], w[:, 2])
            u = (T["d11"][fi] * d02 - T["d01"][fi] * d12) * T["inv"][fi]
            v = (T["d00"][fi] * d12 - T["d01"][fi] * d02) * T["inv"][fi]
            inside = (u >= 0) & (v >= 0) & (u + v <= 1)
        k = ijk[inside]
        out[k[:, 0] + k[:, 1] * dims[0] + k[:, 2] * (dims[0] * dims[1])] = 1
        i = j
    return out.reshape(dims[2], dims[1], dims[0]), pairs


def recenter(grid, gmin, vs, passes=1):
    """recenterFilledVoxels applied `passes` times: the float32 grid_min after it."""
    gmin = np.asarray(gmin, np.float32).copy()
    vs = f32(vs)
    lo, hi = [], []
    for a in range(3):                                       # grid is [z, y, x]: axis a is array axis 2 - a
        occ = np.flatnonzero(grid.any(axis=tuple(k for k in range(3) if k != 2 - a)))
        if len(occ) == 0:
            return gmin
        lo.append(int(occ[0]))
        hi.append(int(occ[-1]))
    for _ in range(passes):
        for a in range(3):
            clo = gmin[a] + (f32(lo[a]) + f32(0.5)) * vs
            chi = gmin[a] + (f32(hi[a]) + f32(0.5)) * vs
            gmin[a] = gmin[a] - f32(0.5) * (clo + chi)
    return gmin


def voxelize(xyz, tris, voxel_size, grid=None, recenter_passes=0):
    """The whole rule: (grid uint8 [z, y, x], dims, grid_min float32[3], voxel_size float32, pairs).  grid: None = AUTO, else
    FIXED (dims, grid_min, voxel_size).  None for AUTO's empty grid."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    if grid is None:
        g = auto_grid(xyz, len(tris), voxel_size)
        if g is None:
            return None
        dims, gmin, vs = g
    else:
        dims, gmin, vs = tuple(int(d) for d in grid[0]), np.asarray(grid[1], np.float32), f32(grid[2])
    out, pairs = fill(xyz, tris, gmin, vs, dims)
    return out, dims, recenter(out, gmin, vs, recenter_passes), vs, pairs


# ---------------------------------------------------------------- CSV text (BuildingLoader.cpp:36-129)
def _parse(text, ntok):
    rows = []
    lines = text.split("\n")
    for line in lines[1:]:                                   # header skipped
        if line == "":
            continue
        toks = [t.strip(" \t\n\r") for t in line.split(",")]
        if line.endswith(","):
            toks = toks[:-1]                                 # std::getline on ',' yields no empty last token
        if len(toks) < ntok:
            continue
        rows.append(toks)
    return rows


def parse_csv_mesh(verts_text, faces_text):
    """(xyz float64 [n, 3], tris int32 [m, 3]) as the host layer resolves them: rows whose stoi / stod fail are skipped; the key
    (mesh, vertex) maps to its LAST row; a face naming a missing key is dropped.  A simplified parser: it covers the fixtures'
    cases (integers and decimal numbers), not every corner of stoi / stod."""
    import re
    num_i = re.compile(r"^[ \t\n\r\f\v]*[+-]?\d+")
    num_d = re.compile(r"^[ \t\n\r\f\v]*[+-]?(\d+\.?\d*([eE][+-]?\d+)?|\.\d+([eE][+-]?\d+)?|inf|nan)", re.I)
    rows, keys = [], {}
    for t in _parse(verts_text, 8):
        if not (num_i.match(t[0]) and num_i.match(t[1]) and all(num_d.match(x) for x in t[2:8])):
            continue
        k = (int(num_i.match(t[0]).group(0)), int(num_i.match(t[1]).group(0)))
        keys[k] = len(rows)
        rows.append([float(num_d.match(t[a]).group(0)) for a in (2, 3, 4)])
    tris = []
    nfaces = 0
    for t in _parse(faces_text, 4):
        if not all(num_i.match(x) for x in t[:4]):
            continue
        nfaces += 1
        m, a, b, c = (int(num_i.match(x).group(0)) for x in t[:4])
        if (m, a) in keys and (m, b) in keys and (m, c) in keys:
            tris.append([keys[(m, a)], keys[(m, b)], keys[(m, c)]])
    return np.asarray(rows, np.float64).reshape(-1, 3), np.asarray(tris, np.int32).reshape(-1, 3), nfaces


# ---------------------------------------------------------------- synthetic scenes (tests, tools/voxelize_bench.py)
def downtown(n_buildings=4200, extent=2000.0, seed=11, origin=(701000.25, 5660500.75, 1040.5)):
    """A synthetic city at UTM magnitudes: extruded rotated-rectangle footprints with sloped roofs (12 faces each) plus one ground
    quad under everything.  (xyz float64 [n, 3], tris int32 [m, 3])."""
    rng = np.random.default_rng(seed)
    ox, oy, oz = origin
    cx = rng.uniform(30.0, extent - 30.0, n_buildings)
    cy = rng.uniform(30.0, extent - 30.0, n_buildings)
    hw = rng.uniform(4.0, 14.0, n_buildings)
    hd = rng.uniform(4.0, 14.0, n_buildings)
    ang = rng.uniform(0.0, np.pi, n_buildings)
    h0 = rng.uniform(6.0, 120.0, n_buildings)
    slope = rng.uniform(0.0, 6.0, n_buildings)
    c, s = np.cos(ang), np.sin(ang)
    u = np.array([-1, 1, 1, -1], np.float64)
    v = np.array([-1, -1, 1, 1], np.float64)
    fx = ox + cx[:, None] + c[:, None] * (u * hw[:, None]) - s[:, None] * (v * hd[:, None])
    fy = oy + cy[:, None] + s[:, None] * (u * hw[:, None]) + c[:, None] * (v * hd[:, None])
    zb = np.full((n_buildings, 4), oz)
    zt = oz + h0[:, None] + slope[:, None] * (u + 1.0) * 0.5                   # roof sloping along the footprint's u axis
    bottom = np.stack([fx, fy, zb], -1)
    top = np.stack([fx, fy, zt], -1)
    xyz = np.concatenate([bottom, top], 1).reshape(-1, 3)                   # 8 rows per building
    q = np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7]] + [[i, (i + 1) % 4, 4 + (i + 1) % 4] for i in range(4)]
                 + [[i, 4 + (i + 1) % 4, 4 + i] for i in range(4)], np.int64)
    tris = (np.arange(n_buildings)[:, None, None] * 8 + q[None]).reshape(-1, 3)
    g = len(xyz)
    ground = np.array([[ox, oy, oz - 0.5], [ox + extent, oy, oz - 0.5], [ox + extent, oy + extent, oz - 0.5], [ox, oy + extent, oz - 0.5]])
    xyz = np.concatenate([xyz, ground])
    tris = np.concatenate([tris, [[g, g + 1, g + 2], [g, g + 2, g + 3]]])
    return xyz, tris.astype(np.int32)


def uv_sphere(nlat=96, nlon=192, r=0.45):
    """A unit-scale UV sphere (rows, faces)."""
    th = np.pi * np.arange(1, nlat) / nlat
    ph = 2 * np.pi * np.arange(nlon) / nlon
    ring = np.stack([r * np.sin(th)[:, None] * np.cos(ph)[None], r * np.sin(th)[:, None] * np.sin(ph)[None],
                     np.repeat(r * np.cos(th)[:, None], nlon, 1)], -1).reshape(-1, 3)
    xyz = np.concatenate([[[0.0, 0.0, r]], ring, [[0.0, 0.0, -r]]])
    south = len(xyz) - 1
    vid = lambda i, j: 1 + (i - 1) * nlon + (j % nlon)                      # noqa: E731
    tris = []
    for j in range(nlon):
        tris += [[0, vid(1, j), vid(1, j + 1)], [south, vid(nlat - 1, j + 1), vid(nlat - 1, j)]]
    for i in range(1, nlat - 1):
        for j in range(nlon):
            tris += [[vid(i, j), vid(i + 1, j), vid(i + 1, j + 1)], [vid(i, j), vid(i + 1, j + 1), vid(i, j + 1)]]
    return xyz, np.asarray(tris, np.int32)
