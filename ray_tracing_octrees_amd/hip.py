"""ctypes binding of the C ABI in include/rto_hip.h (librto_hip.so).

There is no CPU fallback: if the HIP library is missing or no gfx950 device is
usable, `load()` / `Context()` raise `RtoError`.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _build

RTO_OK = 0
RTO_E_INVALID, RTO_E_NO_OCTREE, RTO_E_HIP, RTO_E_NO_DEVICE, RTO_E_UNSUPPORTED, RTO_E_TIMEOUT = -1, -2, -3, -4, -5, -6
RTO_E_INTERNAL = -7
KERNEL_AUTO, KERNEL_GENERIC, KERNEL_PACKED, KERNEL_PACKED_V1, KERNEL_PACKED_PERSISTENT, KERNEL_PACKED_V3 = 0, 1, 2, 3, 4, 5

# struct GPUNodes (453-skeleton/RayTracerBVH.h:21-26)
NODE_DTYPE = np.dtype(
    [("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("size", "<i4"),
     ("isLeaf", "<i4"), ("isSolid", "<i4"), ("isUniform", "<i4"), ("child", "<i4", (8,))]
)

# every symbol include/rto_hip.h declares
SYMBOLS = (
    "rto_create", "rto_destroy", "rto_last_error", "rto_device_name",
    "rto_upload_octree", "rto_build_octree", "rto_download_nodes", "rto_debug_set_build_path", "rto_last_build_ms", "rto_octree_info_get", "rto_set_kernel", "rto_set_launch_order", "rto_forget_stream",
    "rto_update_frustum", "rto_debug_update_frustum_planes", "rto_debug_set_frustum_shortcut", "rto_debug_last_frustum_update_proven", "rto_download_visible_nodes",
    "rto_render_device", "rto_render_host", "rto_partition_rows", "rto_assemble_device",
    "rto_render_shade_device", "rto_assemble_shade_device", "rto_assemble_batch_device", "rto_render_batch_device", "rto_assemble_batch_all_device", "rto_render_resident", "rto_resident_frame", "rto_download_resident",
    "rto_upload_leaf_triangles", "rto_build_leaf_triangles", "rto_download_leaf_triangles", "rto_render_triangles_device", "rto_render_triangles_host", "rto_render_triangles_shade_device",
    "rto_octree_ray_skip", "rto_frame_stats", "rto_render_steps_host", "rto_debug_timeline", "rto_debug_tile_cost", "rto_debug_set_tile_order", "rto_debug_sort_violations", "rto_last_kernel_ms", "rto_timing_begin", "rto_timing_read", "rto_stream", "rto_synchronize",
    "rto_comm_unique_id", "rto_comm_create", "rto_comm_create_all", "rto_comm_destroy", "rto_comm_last_error", "rto_comm_submit",
    "rto_comm_submit_all", "rto_comm_render_resident_all", "rto_comm_flush", "rto_comm_flush_timeout", "rto_comm_is_dead", "rto_comm_ranks_seen", "rto_comm_debug_abort", "rto_comm_stream", "rto_comm_debug_rehearse", "rto_comm_debug_last_payload", "rto_comm_debug_set_timing", "rto_comm_debug_last_timing", "rto_comm_debug_set_rehearsal_clear", "rto_debug_fault_alloc", "rto_render_triangles_batch_device",
    "rto_debug_set_tile_mask", "rto_debug_tile_mask_info", "rto_render_closest_device", "rto_render_closest_host", "rto_render_skip_device", "rto_render_skip_host", "rto_probe_skip_device", "rto_probe_skip_host",
    "rto_scene_bounds_get", "rto_scene_bounds_of_nodes", "rto_split_plan_make", "rto_split_part_of_rank", "rto_split_rows_of_part", "rto_split_row_source",
    "rto_query_rays_device", "rto_query_rays_host", "rto_query_pixels_device", "rto_query_pixels_host",
    "rto_query_triangles_device", "rto_query_triangles_host", "rto_query_triangle_pixels_device", "rto_query_triangle_pixels_host",
    "rto_query_spans_device", "rto_query_spans_host", "rto_query_span_pixels_device", "rto_query_span_pixels_host",
    "rto_edit_voxels", "rto_download_voxels", "rto_last_edit_ms", "rto_brush_quantize",
    "rto_render_lit_device", "rto_render_lit_host", "rto_ao_directions",
    "rto_render_lit_triangles_device", "rto_render_lit_triangles_host",
    "rto_voxelize_mesh", "rto_last_voxelize_ms",
    "rto_frustum_planes", "rto_extract_mesh", "rto_mesh_device", "rto_download_mesh", "rto_last_mesh_ms",
    "rto_query_points_device", "rto_query_points_host", "rto_query_regions_device", "rto_query_regions_host",
    "rto_query_nearest_device", "rto_query_nearest_host", "rto_point_quantize",
    "rto_label_components", "rto_download_components", "rto_download_labels", "rto_labels_device", "rto_last_components_ms",
    "rto_debug_components_passes", "rto_edit_components",
    "rto_distance_field", "rto_download_distance", "rto_distance_device", "rto_last_distance_ms", "rto_edit_morphology",
    "rto_last_morphology_ms",
    "rto_geodesic_field", "rto_download_geodesic", "rto_geodesic_device", "rto_geodesic_paths", "rto_edit_geodesic",
    "rto_last_geodesic_ms", "rto_last_geodesic_edit_ms", "rto_debug_geodesic_passes", "rto_debug_set_geodesic_look",
    "rto_skeleton_field", "rto_download_skeleton", "rto_skeleton_device", "rto_edit_skeleton", "rto_last_skeleton_ms",
    "rto_last_skeleton_edit_ms", "rto_debug_skeleton_passes", "rto_debug_set_skeleton_look",
    "rto_exposure_field", "rto_download_exposure", "rto_exposure_device", "rto_last_exposure_ms",
    "rto_dose_field", "rto_download_dose", "rto_dose_device", "rto_download_dose_coverage", "rto_last_dose_ms",
    "rto_thickness_field", "rto_download_thickness", "rto_thickness_device", "rto_thickness_histogram", "rto_last_thickness_ms",
    "rto_debug_thickness_table",
    "rto_measure_components", "rto_download_measures", "rto_measures_device", "rto_last_measure_ms",
    "rto_segment_parts", "rto_download_part_labels", "rto_download_parts", "rto_download_necks", "rto_parts_device", "rto_edit_parts",
    "rto_last_parts_ms", "rto_debug_parts", "rto_debug_parts_capacity",
    "rto_render_field_device", "rto_render_field_host", "rto_last_field_view_ms",
    "rto_project_field_device", "rto_project_field_host", "rto_last_projection_ms", "rto_debug_set_projection_table",
    "rto_composite_field_device", "rto_composite_field_host", "rto_last_composite_ms",
    "rto_extract_isosurface_device", "rto_extract_isosurface_host", "rto_isosurface_device", "rto_download_isosurface",
    "rto_last_isosurface_ms",
    "rto_extract_dual_contour", "rto_dual_contour_device", "rto_download_dual_contour", "rto_last_dual_contour_ms",
    "rto_query_dual_vertices_device", "rto_query_dual_vertices_host",
)
MESH_MC, MESH_CUBES = 0, 1
SPLIT_MAX_FRAMES = 32
QUERY_FIRST, QUERY_CLOSEST, QUERY_ANY = 0, 1, 2

# struct rto_ray / rto_hit (include/rto_hip.h), 32 bytes each
RAY_DTYPE = np.dtype([("ox", "<f4"), ("oy", "<f4"), ("oz", "<f4"), ("t_min", "<f4"),
                      ("dx", "<f4"), ("dy", "<f4"), ("dz", "<f4"), ("t_max", "<f4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("node", "<i4"), ("face", "<i4"), ("size", "<i4"),
                      ("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("reserved", "<i4")])
# struct rto_tri_hit, 32 bytes
TRI_HIT_DTYPE = np.dtype([("t", "<f4"), ("tri", "<i4"), ("node", "<i4"), ("u", "<f4"), ("v", "<f4"),
                          ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")])
# struct rto_span, 32 bytes: span queries (rto_query_spans_*)
SPAN_DTYPE = np.dtype([("length", "<f4"), ("t_enter", "<f4"), ("t_exit", "<f4"), ("leaves", "<i4"),
                       ("node", "<i4"), ("face", "<i4"), ("reserved", "<i4", (2,))])
# struct rto_brush, 32 bytes: voxel edits (rto_edit_voxels)
BRUSH_SPHERE, BRUSH_BOX = 0, 1
EDIT_CARVE, EDIT_FILL = 0, 1
EDIT_MAX_BRUSHES = 65536
BRUSH_DTYPE = np.dtype([("centre", "<f4", (3,)), ("extent", "<f4", (3,)), ("shape", "<i4"), ("op", "<i4")])
# struct rto_point_hit / rto_region / rto_near_point / rto_nearest: region queries (rto_query_points_*, _regions_*, _nearest_*)
POINT_HIT_DTYPE = np.dtype([("node", "<i4"), ("solid", "<i4"), ("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("size", "<i4"),
                            ("depth", "<i4"), ("reserved", "<i4")])
REGION_DTYPE = np.dtype([("filled", "<i8"), ("covered", "<i8"), ("solid_leaves", "<i4"), ("first_node", "<i4"),
                         ("reserved", "<i4", (2,))])
NEAR_POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("max_dist", "<f4")])
NEAREST_DTYPE = np.dtype([("dist2", "<i8"), ("node", "<i4"), ("size", "<i4"), ("cq", "<i4", (3,)), ("reserved", "<i4")])
# struct rto_component, 48 bytes: connected components (rto_label_components, rto_edit_components)
SET_EMPTY, SET_SOLID = 0, 1
CONN_FACE, CONN_FULL = 6, 26
SELECT_SMALLER_THAN, SELECT_ALL_BUT_LARGEST, SELECT_ENCLOSED, SELECT_CONTAINING, SELECT_NOT_CONTAINING = 0, 1, 2, 3, 4
COMPONENT_DTYPE = np.dtype([("root", "<i8"), ("voxels", "<i8"), ("lo", "<i4", (3,)), ("hi", "<i4", (3,)), ("touches", "<i4"),
                            ("reserved", "<i4")])
# struct rto_dist_summary, 32 bytes: distance fields and morphology (rto_distance_field, rto_edit_morphology)
DIST_NONE = 0x7fffffff
MORPH_DILATE, MORPH_ERODE, MORPH_OPEN, MORPH_CLOSE = 0, 1, 2, 3
DIST_SUMMARY_DTYPE = np.dtype([("max_d2", "<i8"), ("argmax", "<i8"), ("finite", "<i8"), ("reserved", "<i8")])
# struct rto_geo_summary, 32 bytes: geodesic fields (rto_geodesic_field)
GEO_SUMMARY_DTYPE = np.dtype([("max_g", "<i8"), ("argmax", "<i8"), ("reached", "<i8"), ("reserved", "<i8")])
GEO_NO_LIMIT = 0x7fffffff
# struct rto_skel_summary, 32 bytes: skeleton fields (rto_skeleton_field)
SKEL_SUMMARY_DTYPE = np.dtype([("kept", "<i8"), ("removed", "<i8"), ("passes", "<i8"), ("reserved", "<i8")])
SKEL_TOPOLOGY, SKEL_CURVE = 0, 1
SKEL_NO_LIMIT = 0x7fffffff
# struct rto_expo_summary, 32 bytes: exposure fields (rto_exposure_field)
EXPO_SUMMARY_DTYPE = np.dtype([("evaluated", "<i8"), ("total", "<i8"), ("dark", "<i8"), ("open", "<i8")])
EXPO_ALL, EXPO_SKIN = 0, 1
EXPO_MAX_COMP = 255      # RTO_EXPO_MAX_COMP: the largest |component| of a direction
EXPO_MAX_DIRS = 1024     # RTO_EXPO_MAX_DIRS
EXPO_NO_LIMIT = 0x7fffffff
# struct rto_dose_summary, 48 bytes: dose fields (rto_dose_field)
DOSE_SUMMARY_DTYPE = np.dtype([("evaluated", "<i8"), ("total", "<i8"), ("dark", "<i8"), ("seen", "<i8"), ("peak", "<i8"), ("peak_voxel", "<i8")])
DOSE_ALL, DOSE_SKIN = 0, 1
DOSE_FALLOFF_NONE, DOSE_FALLOFF_INVERSE_SQUARE = 0, 1
DOSE_MAX_SOURCES = 1024  # RTO_DOSE_MAX_SOURCES
DOSE_MAX_REACH = 1023    # RTO_DOSE_MAX_REACH: what DOSE_NO_LIMIT, and every reach above it, stands for
DOSE_MAX_TABLE = 64      # RTO_DOSE_MAX_TABLE: the longest transmission table
DOSE_NO_LIMIT = 0x7fffffff
# struct rto_thick_summary, 32 bytes: local thickness fields (rto_thickness_field)
THICK_SUMMARY_DTYPE = np.dtype([("min_t2", "<i8"), ("argmin", "<i8"), ("thin", "<i8"), ("medium", "<i8")])
THICK_MAX_C = 64         # RTO_THICK_MAX_C: balls of up to 8 voxels
# struct rto_measure, 160 bytes: component measures (rto_measure_components)
MEASURE_DTYPE = np.dtype([("voxels", "<i8"), ("faces", "<i8", (6,)), ("cells", "<i8", (3,)), ("euler", "<i8"), ("sum", "<i8", (3,)),
                          ("sum2", "<i8", (6,))])
MEASURE_MAX_DIM = 32768  # RTO_MEASURE_MAX_DIM: the largest dimension rto_measure_components takes
# struct rto_part (64 bytes), rto_neck (32), rto_parts_summary (32): part segmentation (rto_segment_parts, rto_edit_parts)
PART_DTYPE = np.dtype([("root", "<i8"), ("voxels", "<i8"), ("lo", "<i4", (3,)), ("hi", "<i4", (3,)), ("touches", "<i4"), ("basins", "<i4"),
                       ("peak", "<i8"), ("peak_h", "<i4"), ("reserved", "<i4")])
NECK_DTYPE = np.dtype([("part_lo", "<i4"), ("part_hi", "<i4"), ("h", "<i4"), ("reserved", "<i4"), ("at", "<i8"), ("pairs", "<i8")])
PARTS_SUMMARY_DTYPE = np.dtype([("parts", "<i8"), ("basins", "<i8"), ("necks", "<i8"), ("pairs", "<i8")])
PARTS_RATIO_MAX = 1001   # RTO_PARTS_RATIO_MAX: joins nothing, the parts are the basins
# field views (rto_render_field_*): RTO_FIELD_*, RTO_SAMPLE_*, RTO_SCALE_* and the two pixel codes of the value buffer
FIELD_DISTANCE, FIELD_GEODESIC, FIELD_THICKNESS, FIELD_SKELETON, FIELD_EXPOSURE, FIELD_PARTS, FIELD_LABELS, FIELD_CALLER = 0, 1, 2, 3, 4, 5, 6, 7
SAMPLE_HIT, SAMPLE_FRONT = 0, 1
SCALE_LINEAR, SCALE_SQRT, SCALE_CATEGORY = 0, 1, 2
FIELD_PIXEL_MISS, FIELD_PIXEL_NONE = -2**31, -2**31 + 1
FIELD_VIEW_SUMMARY_DTYPE = np.dtype([("hits", "<i8"), ("valued", "<i8"), ("vmin", "<i4"), ("vmax", "<i4"), ("lo", "<i4"), ("hi", "<i4")])
# field projections (rto_project_field_*): RTO_PROJECT_*
PROJECT_MAX, PROJECT_MIN, PROJECT_MEAN, PROJECT_COUNT, PROJECT_FIRST = 0, 1, 2, 3, 4
# field compositing (rto_composite_field_*): struct rto_composite_summary
COMPOSITE_SUMMARY_DTYPE = np.dtype([("visited", "<i8"), ("contributing", "<i8"), ("saturated", "<i8"), ("occluded", "<i8")])
AO_MAX_SAMPLES = 64      # RTO_AO_MAX_SAMPLES: the lit render's AO rays per pixel at most
COMM_ID_BYTES = 128
RESIDENT_OCTREE, RESIDENT_TRIANGLES, RESIDENT_TRIANGLES_SHADOW = 0, 1, 2


def measure_physical(m, grid_min, voxel_size):
    """World-space quantities of MEASURE_DTYPE records (an array or one record), in float64: a dict of volume (voxels vs^3), area
    (all exposed faces, vs^2 each), centroid (grid_min + (sum / voxels + 0.5) vs: a voxel spans [grid_min + i vs, grid_min +
    (i + 1) vs]), covariance (3 x 3, of the voxel centres, world units squared), and its principal axes by numpy.linalg.eigh:
    axes_variance ascending and axes with the unit axis k in column k.  Records with no voxel give NaN."""
    m = np.asarray(m)
    gm = np.asarray(grid_min, np.float64).reshape(3)
    vs = float(voxel_size)
    n = m["voxels"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = m["sum"].astype(np.float64) / n[..., None]
        s2 = m["sum2"].astype(np.float64) / n[..., None]
    cov = np.empty(m.shape + (3, 3), np.float64)
    for k, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        cov[..., a, b] = cov[..., b, a] = (s2[..., k] - mean[..., a] * mean[..., b]) * vs * vs
    ok = np.isfinite(cov).all(axis=(-1, -2))
    var, axes = np.linalg.eigh(np.where(ok[..., None, None], cov, np.eye(3)))
    var = np.where(ok[..., None], var, np.nan)
    axes = np.where(ok[..., None, None], axes, np.nan)
    return {"volume": n * vs ** 3, "area": m["faces"].sum(axis=-1).astype(np.float64) * vs * vs, "centroid": gm + (mean + 0.5) * vs,
            "covariance": cov, "axes_variance": var, "axes": axes}


def quantize_directions(float_dirs, max_comp: int = EXPO_MAX_COMP) -> np.ndarray:
    """Integer directions for Context.exposure_field from float vectors (n, 3), as (n, 3) int32: each vector is scaled so that its
    largest |component| is max_comp, rounded to nearest (numpy.rint) and divided by the gcd of its components.  A zero or
    non-finite vector is refused (ValueError), and so is a max_comp outside 1 .. EXPO_MAX_COMP."""
    if not 1 <= int(max_comp) <= EXPO_MAX_COMP:
        raise ValueError("max_comp must be in 1 .. EXPO_MAX_COMP")
    d = np.asarray(float_dirs, np.float64).reshape(-1, 3)
    top = np.abs(d).max(axis=1) if len(d) else np.empty(0)
    if not np.isfinite(d).all() or (top == 0).any():
        raise ValueError("a direction is zero or not finite")
    q = np.rint(d / top[:, None] * int(max_comp)).astype(np.int64)
    g = np.gcd.reduce(np.abs(q), axis=1)
    return np.ascontiguousarray(q // g[:, None], np.int32)


class RtoError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"rto error {code}: {msg}")
        self.code = code


class Frame(C.Structure):
    _fields_ = [("view", C.c_float * 16), ("cam_pos", C.c_float * 3), ("aspect", C.c_float),
                ("fov_deg", C.c_float), ("width", C.c_int32), ("height", C.c_int32)]


class Partition(C.Structure):
    _fields_ = [("num_parts", C.c_int32), ("part", C.c_int32), ("band_rows", C.c_int32)]


class Ray(C.Structure):
    _fields_ = [("ox", C.c_float), ("oy", C.c_float), ("oz", C.c_float), ("t_min", C.c_float),
                ("dx", C.c_float), ("dy", C.c_float), ("dz", C.c_float), ("t_max", C.c_float)]


class TriHit(C.Structure):
    _fields_ = [("t", C.c_float), ("tri", C.c_int32), ("node", C.c_int32), ("u", C.c_float), ("v", C.c_float),
                ("nx", C.c_float), ("ny", C.c_float), ("nz", C.c_float)]


class Brush(C.Structure):
    _fields_ = [("centre", C.c_float * 3), ("extent", C.c_float * 3), ("shape", C.c_int32), ("op", C.c_int32)]


# struct rto_voxelize_params (40 bytes) / rto_voxelize_result (48 bytes): mesh voxelization (rto_voxelize_mesh)
VOXELIZE_AUTO, VOXELIZE_FIXED = 0, 1


class VoxelizeParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("voxel_size", C.c_float), ("dims", C.c_int32 * 3), ("grid_min", C.c_float * 3),
                ("recenter_passes", C.c_int32), ("triangles", C.c_int32)]


class VoxelizeResult(C.Structure):
    _fields_ = [("dims", C.c_int32 * 3), ("grid_min", C.c_float * 3), ("voxel_size", C.c_float), ("reserved", C.c_int32),
                ("filled", C.c_int64), ("pairs", C.c_int64)]


# struct rto_lighting, 32 bytes: the lit render (rto_render_lit_*)
class Lighting(C.Structure):
    _fields_ = [("light_dir", C.c_float * 3), ("shadow", C.c_int32), ("ao_samples", C.c_int32), ("ao_radius", C.c_float),
                ("seed", C.c_uint32), ("reserved", C.c_int32)]


def make_lighting(light_dir=(-1.0, -1.0, -1.0), shadow=True, ao_samples=0, ao_radius=1.0, seed=0) -> Lighting:
    """An rto_lighting: light_dir is the direction the light travels ((-1, -1, -1) is the renders' light)."""
    L = Lighting()
    for a in range(3):
        L.light_dir[a] = _f(light_dir[a])
    L.shadow = 1 if shadow else 0
    L.ao_samples = int(ao_samples)
    L.ao_radius = _f(ao_radius)
    L.seed = int(seed) & 0xFFFFFFFF
    L.reserved = 0
    return L


def ao_directions() -> np.ndarray:
    """rto_ao_directions: the lit render's 64 AO directions, (64, 3) float32 (pure host function)."""
    out = np.zeros((AO_MAX_SAMPLES, 3), np.float32)
    rc = load().rto_ao_directions(out.ctypes.data)
    if rc != RTO_OK:
        raise RtoError(rc, "rto_ao_directions failed")
    return out


# struct rto_field_view (112 bytes) and rto_field_view_summary (32): field views (rto_render_field_*)
class FieldView(C.Structure):
    _fields_ = [("source", C.c_int32), ("sample", C.c_int32), ("mode", C.c_int32), ("scale", C.c_int32),
                ("valid_lo", C.c_int32), ("valid_hi", C.c_int32), ("range_lo", C.c_int32), ("range_hi", C.c_int32),
                ("clip", C.c_int32), ("clip_lo", C.c_int32 * 3), ("clip_hi", C.c_int32 * 3), ("shade", C.c_int32),
                ("miss_rgba", C.c_float * 4), ("none_rgba", C.c_float * 4), ("reserved", C.c_int32 * 4)]


class FieldViewSummary(C.Structure):
    _fields_ = [("hits", C.c_int64), ("valued", C.c_int64), ("vmin", C.c_int32), ("vmax", C.c_int32), ("lo", C.c_int32), ("hi", C.c_int32)]


def make_field_view(source, sample=SAMPLE_HIT, mode=QUERY_FIRST, scale=SCALE_LINEAR, valid=(0, 0x7ffffffe), range=(0, 0), clip=None,
                    shade=False, miss_rgba=(0.0, 0.0, 0.0, 1.0), none_rgba=(0.25, 0.25, 0.25, 1.0)) -> FieldView:
    """An rto_field_view with the header's defaults.  range: (lo, hi), equal for auto range; clip: None or ((x0, y0, z0),
    (x1, y1, z1)) in voxel indices."""
    v = FieldView()
    v.source, v.sample, v.mode, v.scale = int(source), int(sample), int(mode), int(scale)
    v.valid_lo, v.valid_hi = int(valid[0]), int(valid[1])
    v.range_lo, v.range_hi = int(range[0]), int(range[1])
    v.clip = 0 if clip is None else 1
    for a in (0, 1, 2):
        v.clip_lo[a] = 0 if clip is None else int(clip[0][a])
        v.clip_hi[a] = 0 if clip is None else int(clip[1][a])
    v.shade = 1 if shade else 0
    for k in (0, 1, 2, 3):
        v.miss_rgba[k] = _f(miss_rgba[k])
        v.none_rgba[k] = _f(none_rgba[k])
    return v


# struct rto_field_projection (112 bytes): field projections (rto_project_field_*)
class FieldProjection(C.Structure):
    _fields_ = [("source", C.c_int32), ("op", C.c_int32), ("scale", C.c_int32), ("valid_lo", C.c_int32), ("valid_hi", C.c_int32),
                ("range_lo", C.c_int32), ("range_hi", C.c_int32), ("clip", C.c_int32), ("clip_lo", C.c_int32 * 3),
                ("clip_hi", C.c_int32 * 3), ("miss_rgba", C.c_float * 4), ("none_rgba", C.c_float * 4), ("reserved", C.c_int32 * 6)]


def make_field_projection(source, op=PROJECT_MAX, scale=SCALE_LINEAR, valid=(0, 0x7ffffffe), range=(0, 0), clip=None,
                          miss_rgba=(0.0, 0.0, 0.0, 1.0), none_rgba=(0.25, 0.25, 0.25, 1.0)) -> FieldProjection:
    """An rto_field_projection with the header's defaults.  range: (lo, hi), equal for auto range; clip: None or ((x0, y0, z0),
    (x1, y1, z1)) in voxel indices."""
    v = FieldProjection()
    v.source, v.op, v.scale = int(source), int(op), int(scale)
    v.valid_lo, v.valid_hi = int(valid[0]), int(valid[1])
    v.range_lo, v.range_hi = int(range[0]), int(range[1])
    v.clip = 0 if clip is None else 1
    for a in (0, 1, 2):
        v.clip_lo[a] = 0 if clip is None else int(clip[0][a])
        v.clip_hi[a] = 0 if clip is None else int(clip[1][a])
    for k in (0, 1, 2, 3):
        v.miss_rgba[k] = _f(miss_rgba[k])
        v.none_rgba[k] = _f(none_rgba[k])
    return v


# struct rto_field_composite (112 bytes): field compositing (rto_composite_field_*)
class FieldComposite(C.Structure):
    _fields_ = [("source", C.c_int32), ("scale", C.c_int32), ("valid_lo", C.c_int32), ("valid_hi", C.c_int32),
                ("range_lo", C.c_int32), ("range_hi", C.c_int32), ("clip", C.c_int32), ("clip_lo", C.c_int32 * 3),
                ("clip_hi", C.c_int32 * 3), ("stop_q16", C.c_int32), ("occlude", C.c_int32), ("background_rgba", C.c_float * 4),
                ("miss_rgba", C.c_float * 4), ("reserved", C.c_int32 * 5)]


def make_field_composite(source, scale=SCALE_LINEAR, valid=(0, 0x7ffffffe), range=(0, 1), clip=None, stop_q16=0, occlude=False,
                         background_rgba=(0.0, 0.0, 0.0, 0.0), miss_rgba=(0.0, 0.0, 0.0, 0.0)) -> FieldComposite:
    """An rto_field_composite.  range: (lo, hi) with lo < hi under LINEAR and SQRT (there is no auto range); clip: None or ((x0,
    y0, z0), (x1, y1, z1)) in voxel indices; stop_q16: 0 .. 65535, the transmittance (of 65536) at which a ray ends; occlude: the
    ray ends at the first FILLED voxel."""
    v = FieldComposite()
    v.source, v.scale = int(source), int(scale)
    v.valid_lo, v.valid_hi = int(valid[0]), int(valid[1])
    v.range_lo, v.range_hi = int(range[0]), int(range[1])
    v.clip = 0 if clip is None else 1
    for a in (0, 1, 2):
        v.clip_lo[a] = 0 if clip is None else int(clip[0][a])
        v.clip_hi[a] = 0 if clip is None else int(clip[1][a])
    v.stop_q16, v.occlude = int(stop_q16), int(occlude)
    for k in (0, 1, 2, 3):
        v.background_rgba[k] = _f(background_rgba[k])
        v.miss_rgba[k] = _f(miss_rgba[k])
    return v


# struct rto_iso_params (64 bytes) / rto_iso_summary (32 bytes): field isosurfaces (rto_extract_isosurface_*)
class IsoParams(C.Structure):
    _fields_ = [("source", C.c_int32), ("valid_lo", C.c_int32), ("valid_hi", C.c_int32), ("level", C.c_float), ("outside", C.c_float),
                ("pad", C.c_int32), ("clip", C.c_int32), ("clip_lo", C.c_int32 * 3), ("clip_hi", C.c_int32 * 3),
                ("reserved", C.c_int32 * 3)]


class IsoSummary(C.Structure):
    _fields_ = [("triangles", C.c_int64), ("active_cells", C.c_int64), ("degenerate", C.c_int64), ("reserved", C.c_int64)]


def make_iso_params(source, level, outside=0.0, valid=(0, 0x7ffffffe), pad=True, clip=None) -> IsoParams:
    """An rto_iso_params.  level: the iso value; half-integer levels avoid degenerate triangles.  outside: the value of every
    sample that is unvalued, outside the box or in the pad ring.  The default 0 closes the surface around what lies above the
    level; a field that grows away from its object, such as the distance to the solids, wants a large value.  pad: True or False
    (an integer is handed on as it is).  clip: None or ((x0, y0, z0), (x1, y1, z1)) in voxel indices."""
    v = IsoParams()
    v.source = int(source)
    v.valid_lo, v.valid_hi = int(valid[0]), int(valid[1])
    v.level, v.outside = _f(level), _f(outside)
    v.pad = int(pad)
    v.clip = 0 if clip is None else 1
    for a in (0, 1, 2):
        v.clip_lo[a] = 0 if clip is None else int(clip[0][a])
        v.clip_hi[a] = 0 if clip is None else int(clip[1][a])
    return v


# struct rto_dc_params (48 bytes) / rto_dc_summary (48 bytes) / rto_dual_vertex (16 bytes): dual contouring (rto_extract_dual_contour)
DC_AREA_REFERENCE, DC_AREA_NONE = 0, 1


class DcParams(C.Structure):
    _fields_ = [("area_rule", C.c_int32), ("clip", C.c_int32), ("clip_lo", C.c_int32 * 3), ("clip_hi", C.c_int32 * 3),
                ("reserved", C.c_int32 * 4)]


class DcSummary(C.Structure):
    _fields_ = [("faces", C.c_int64), ("triangles", C.c_int64), ("dropped", C.c_int64), ("degenerate", C.c_int64),
                ("vertex_voxels", C.c_int64), ("reserved", C.c_int64)]


DUAL_VERTEX_DTYPE = np.dtype([("p", np.float32, 3), ("points", np.int32)])


def make_dc_params(area_rule=DC_AREA_REFERENCE, clip=None) -> DcParams:
    """An rto_dc_params.  area_rule: DC_AREA_REFERENCE drops triangles of area <= 1e-6 as the reference does (at voxel sizes near
    1 / 512 that drops real ones), DC_AREA_NONE keeps all.  clip: None or ((x0, y0, z0), (x1, y1, z1)) in cell indices."""
    v = DcParams()
    v.area_rule = int(area_rule)
    v.clip = 0 if clip is None else 1
    for a in (0, 1, 2):
        v.clip_lo[a] = 0 if clip is None else int(clip[0][a])
        v.clip_hi[a] = 0 if clip is None else int(clip[1][a])
    return v


def ramp_lut(anchors) -> np.ndarray:
    """256 LUT entries (uint32, bytes r, g, b, a in memory order) interpolated between n >= 1 RGBA anchor colours (bytes), in
    integers: with p = i * (n - 1), j = p // 255 and f = p % 255, entry i is anchors[j] for f == 0, else per channel
    (a[j] * (255 - f) + a[j + 1] * f + 127) // 255.  Entry 0 is the first anchor, entry 255 the last."""
    a = np.asarray(anchors, np.int64).reshape(-1, 4)
    if len(a) < 1 or a.min() < 0 or a.max() > 255:
        raise ValueError("ramp_lut: anchors are RGBA bytes")
    n = len(a)
    p = np.arange(256, dtype=np.int64) * (n - 1)
    j, f = p // 255, (p % 255)[:, None]
    nxt = a[np.minimum(j + 1, n - 1)]
    rgba = (a[j] * (255 - f) + nxt * f + 127) // 255
    return np.ascontiguousarray(rgba.astype(np.uint8)).view("<u4").reshape(256)


class Hit(C.Structure):
    _fields_ = [("t", C.c_float), ("node", C.c_int32), ("face", C.c_int32), ("size", C.c_int32),
                ("x", C.c_int32), ("y", C.c_int32), ("z", C.c_int32), ("reserved", C.c_int32)]


class Span(C.Structure):
    _fields_ = [("length", C.c_float), ("t_enter", C.c_float), ("t_exit", C.c_float), ("leaves", C.c_int32),
                ("node", C.c_int32), ("face", C.c_int32), ("reserved", C.c_int32 * 2)]


def make_rays(origins, dirs, t_min=0.0, t_max=1e30) -> np.ndarray:
    """A RAY_DTYPE array from (n, 3) origins (or one origin for all rays), (n, 3) directions and scalar or per-ray windows."""
    d = np.asarray(dirs, np.float32).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(origins, np.float32).reshape(-1, 3), d.shape)
    r = np.zeros(len(d), RAY_DTYPE)
    r["ox"], r["oy"], r["oz"] = o[:, 0], o[:, 1], o[:, 2]
    r["dx"], r["dy"], r["dz"] = d[:, 0], d[:, 1], d[:, 2]
    r["t_min"] = np.broadcast_to(np.asarray(t_min, np.float32), len(d))
    r["t_max"] = np.broadcast_to(np.asarray(t_max, np.float32), len(d))
    return r


def make_brushes(centres, extents, shape=BRUSH_SPHERE, op=EDIT_CARVE) -> np.ndarray:
    """A BRUSH_DTYPE array from (n, 3) centres; extents as (n, 3) per-axis half-sizes, or (n,) / one scalar (a radius, or the
    half-size on every axis); shape and op as one scalar or one per brush."""
    c = np.asarray(centres, np.float32).reshape(-1, 3)
    e = np.asarray(extents, np.float32)
    e = np.broadcast_to(e, c.shape) if e.ndim == 2 else np.repeat(np.broadcast_to(e, (len(c),))[:, None], 3, axis=1)
    b = np.zeros(len(c), BRUSH_DTYPE)
    b["centre"], b["extent"] = c, e
    b["shape"] = np.broadcast_to(np.asarray(shape, np.int32), len(c))
    b["op"] = np.broadcast_to(np.asarray(op, np.int32), len(c))
    return b


def brush_quantize(brush, grid_min, voxel_size):
    """rto_brush_quantize: (cq, eq) as two tuples of int for one BRUSH_DTYPE record; RtoError(RTO_E_INVALID) for an invalid brush."""
    L = load()
    b = np.ascontiguousarray(np.asarray(brush, BRUSH_DTYPE).reshape(1))
    gm = (C.c_float * 3)(*[_f(x) for x in grid_min])
    cq, eq = (C.c_int64 * 3)(), (C.c_int64 * 3)()
    rc = L.rto_brush_quantize(b.ctypes.data, gm, _f(voxel_size), cq, eq)
    if rc != RTO_OK:
        raise RtoError(rc, "rto_brush_quantize: invalid brush")
    return tuple(cq), tuple(eq)


def point_quantize(p, grid_min, voxel_size):
    """rto_point_quantize: pq as a tuple of int for one point; RtoError(RTO_E_INVALID) for an invalid point."""
    L = load()
    pt = (C.c_float * 3)(*[_f(x) for x in p])
    gm = (C.c_float * 3)(*[_f(x) for x in grid_min])
    pq = (C.c_int64 * 3)()
    rc = L.rto_point_quantize(pt, gm, _f(voxel_size), pq)
    if rc != RTO_OK:
        raise RtoError(rc, "rto_point_quantize: invalid point")
    return tuple(pq)


def make_near_points(points, max_dist=np.inf) -> np.ndarray:
    """A NEAR_POINT_DTYPE array from (n, 3) points and one max_dist or one per point."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    r = np.zeros(len(p), NEAR_POINT_DTYPE)
    r["x"], r["y"], r["z"] = p[:, 0], p[:, 1], p[:, 2]
    r["max_dist"] = np.broadcast_to(np.asarray(max_dist, np.float32), len(p))
    return r


class Stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("pops", C.c_uint64), ("hits", C.c_uint64), ("capped", C.c_uint64)]


class OctreeInfo(C.Structure):
    _fields_ = [("num_nodes", C.c_int64), ("num_internal", C.c_int64), ("root_size", C.c_int32),
                ("depth", C.c_int32), ("canonical", C.c_int32), ("culling_active", C.c_int32),
                ("visible_nodes", C.c_int64)]


class SceneBounds(C.Structure):
    """rto_scene_bounds: what the screen rectangles and the split plan need to know of a scene."""
    _fields_ = [("grid_min", C.c_float * 3), ("voxel_size", C.c_float), ("root_size", C.c_int32),
                ("solid_lo", C.c_int32 * 3), ("solid_hi", C.c_int32 * 3)]


class MeshCull(C.Structure):
    """rto_mesh_cull (include/rto_hip.h), 100 bytes: six normalised planes and renderOctree's extraMargin."""
    _fields_ = [("planes", C.c_float * 24), ("margin", C.c_float)]


def frustum_planes(view, fov_deg, aspect) -> np.ndarray:
    """rto_frustum_planes (pure host): the 24 floats Frustum(perspective(radians(fov_deg), aspect, 0.01, 5000) * view) holds."""
    v = np.ascontiguousarray(np.asarray(view, dtype=np.float32).reshape(16))
    out = np.zeros(24, np.float32)
    rc = load().rto_frustum_planes(v.ctypes.data_as(C.POINTER(C.c_float)), _f(fov_deg), _f(aspect), out.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != RTO_OK:
        raise RtoError(rc, "rto_frustum_planes")
    return out


class SplitPlan(C.Structure):
    """rto_split_plan (include/rto_hip.h): everything the ranks of a screen split must agree on."""
    _fields_ = [("world", C.c_int32), ("band_rows", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("n_frames", C.c_int32),
                ("render_parts", C.c_int32), ("first_render_rank", C.c_int32), ("rows_part0", C.c_int32), ("cropped", C.c_int32),
                ("win_x0", C.c_int32 * SPLIT_MAX_FRAMES), ("win_w", C.c_int32 * SPLIT_MAX_FRAMES), ("win_off", C.c_int64 * SPLIT_MAX_FRAMES),
                ("frame_floats", C.c_int64), ("full_floats", C.c_int64), ("pack_floats", C.c_int64)]


_lib = None


def _f(x) -> float:
    """A Python float that holds exactly the binary32 value of x."""
    return float(np.float32(x))


def lib_path() -> str:
    # RTO_HIP_LIB: developer aid for A/B builds of the kernels (another librto_hip.so with the same ABI)
    return os.environ.get("RTO_HIP_LIB") or _build.LIB_HIP


def load():
    """dlopen librto_hip.so and declare prototypes.  Raises RtoError when the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise RtoError(RTO_E_NO_DEVICE, f"{path} is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                        "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    _build.preload_torch_runtime()     # one HIP runtime per process (see _build.preload_torch_runtime)
    L = C.CDLL(path)
    vp = C.c_void_p
    L.rto_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.rto_destroy.argtypes = [vp]
    L.rto_destroy.restype = None
    L.rto_last_error.argtypes = [vp]
    L.rto_last_error.restype = C.c_char_p
    L.rto_device_name.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.rto_upload_octree.argtypes = [vp, vp, C.c_int64, C.POINTER(C.c_float), C.c_float]
    L.rto_octree_info_get.argtypes = [vp, C.POINTER(OctreeInfo)]
    L.rto_build_octree.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_float]
    L.rto_download_nodes.argtypes = [vp, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.rto_debug_set_build_path.argtypes = [vp, C.c_int]
    L.rto_last_build_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.rto_set_kernel.argtypes = [vp, C.c_int]
    L.rto_set_launch_order.argtypes = [vp, C.c_int, C.c_int]
    L.rto_forget_stream.argtypes = [vp, vp]
    L.rto_debug_update_frustum_planes.argtypes = [vp, C.POINTER(C.c_float), C.c_float]
    L.rto_debug_set_frustum_shortcut.argtypes = [vp, C.c_int]
    L.rto_debug_last_frustum_update_proven.argtypes = [vp, C.POINTER(C.c_int)]
    L.rto_debug_sort_violations.argtypes = [vp, C.POINTER(C.c_int)]
    L.rto_debug_set_tile_mask.argtypes = [vp, C.c_int]
    L.rto_debug_tile_mask_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.rto_update_frustum.argtypes = [vp, C.POINTER(C.c_float), C.c_float, C.c_float, C.c_int]
    L.rto_download_visible_nodes.argtypes = [vp, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.rto_render_device.argtypes = [vp, C.POINTER(Frame), C.POINTER(Partition), vp, vp]
    L.rto_render_host.argtypes = [vp, C.POINTER(Frame), vp]
    L.rto_partition_rows.argtypes = [C.POINTER(Frame), C.POINTER(Partition)]
    L.rto_assemble_device.argtypes = [vp, C.POINTER(Frame), C.POINTER(Partition), vp, vp, vp]
    L.rto_render_resident.argtypes = [vp, C.POINTER(Frame), C.c_int]
    L.rto_resident_frame.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.rto_download_resident.argtypes = [vp, vp]
    L.rto_render_shade_device.argtypes = [vp, C.POINTER(Frame), C.POINTER(Partition), vp, vp]
    L.rto_assemble_shade_device.argtypes = [vp, C.POINTER(Frame), C.POINTER(Partition), vp, vp, vp]
    L.rto_assemble_batch_device.argtypes = [vp, C.POINTER(Frame), C.POINTER(Partition), vp, C.c_int, C.c_int, C.c_int, vp, vp]
    L.rto_render_batch_device.argtypes = [vp, C.POINTER(Frame), C.c_int, C.POINTER(Partition), C.c_int, vp, C.c_size_t, vp]
    L.rto_assemble_batch_all_device.argtypes = [vp, C.POINTER(Frame), C.c_int, C.POINTER(Partition), vp, C.c_int, vp, C.c_size_t, vp]
    L.rto_render_triangles_shade_device.argtypes = [vp, C.POINTER(Frame), C.POINTER(Partition), C.c_int, vp, vp]
    L.rto_frame_stats.argtypes = [vp, C.POINTER(Frame), C.POINTER(Stats)]
    L.rto_upload_leaf_triangles.argtypes = [vp, vp, C.c_int64, vp]
    L.rto_render_triangles_device.argtypes = [vp, C.POINTER(Frame), C.POINTER(Partition), C.c_int, vp, vp]
    L.rto_build_leaf_triangles.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int]
    L.rto_download_leaf_triangles.argtypes = [vp, vp, C.c_int64, vp, C.POINTER(C.c_int64)]
    L.rto_render_triangles_host.argtypes = [vp, C.POINTER(Frame), C.c_int, vp, C.POINTER(Stats)]
    L.rto_octree_ray_skip.argtypes = [vp, C.POINTER(C.c_float), vp, C.c_int64, C.c_float, C.c_float, C.c_int, vp]
    L.rto_render_steps_host.argtypes = [vp, C.POINTER(Frame), vp]
    L.rto_render_closest_device.argtypes = [vp, C.POINTER(Frame), C.POINTER(Partition), vp, vp]
    L.rto_render_closest_host.argtypes = [vp, C.POINTER(Frame), vp, C.POINTER(Stats)]
    L.rto_render_skip_device.argtypes = [vp, C.POINTER(Frame), C.POINTER(Partition), C.c_int, vp, vp, vp]
    L.rto_render_skip_host.argtypes = [vp, C.POINTER(Frame), C.c_int, vp, vp]
    L.rto_probe_skip_device.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_int, vp, vp]
    L.rto_probe_skip_host.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_int, C.POINTER(C.c_float), vp]
    L.rto_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rto_debug_tile_cost.argtypes = [vp, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.rto_debug_set_tile_order.argtypes = [vp, vp, C.c_int64]
    L.rto_debug_timeline.argtypes = [vp, C.POINTER(Frame), vp, C.c_int64, C.POINTER(C.c_int64)]
    L.rto_synchronize.argtypes = [vp]
    L.rto_timing_begin.argtypes = [vp, C.c_int]
    L.rto_timing_read.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.rto_stream.argtypes = [vp]
    L.rto_stream.restype = vp
    L.rto_comm_unique_id.argtypes = [vp]
    L.rto_comm_create.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, C.POINTER(vp)]
    L.rto_comm_create_all.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(vp)]
    L.rto_comm_destroy.argtypes = [vp]
    L.rto_comm_destroy.restype = None
    L.rto_comm_last_error.argtypes = [vp]
    L.rto_comm_last_error.restype = C.c_char_p
    L.rto_comm_submit.argtypes = [vp, C.POINTER(Frame), C.c_int, C.c_int, vp, C.c_size_t]
    L.rto_comm_submit_all.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(Frame), C.c_int, C.c_int, vp, C.c_size_t]
    L.rto_comm_render_resident_all.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(Frame), C.c_int]
    L.rto_comm_flush.argtypes = [vp]
    L.rto_comm_flush_timeout.argtypes = [vp, C.c_int]
    L.rto_comm_is_dead.argtypes = [vp]
    L.rto_comm_ranks_seen.argtypes = [vp, C.POINTER(C.c_int)]
    L.rto_comm_debug_abort.argtypes = [vp]
    L.rto_comm_debug_rehearse.argtypes = [vp, C.c_int, C.c_int]
    L.rto_comm_debug_set_rehearsal_clear.argtypes = [vp, C.c_int]
    L.rto_comm_debug_set_timing.argtypes = [vp, C.c_int]
    L.rto_comm_debug_last_timing.argtypes = [vp, C.POINTER(C.c_float)]
    L.rto_debug_fault_alloc.argtypes = [C.c_long]
    L.rto_comm_debug_last_payload.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.rto_render_triangles_batch_device.argtypes = [vp, C.POINTER(Frame), C.c_int, C.POINTER(Partition), C.c_int, C.c_int, vp, C.c_size_t, vp]
    L.rto_comm_stream.argtypes = [vp]
    L.rto_comm_stream.restype = vp
    L.rto_scene_bounds_get.argtypes = [vp, C.POINTER(SceneBounds)]
    L.rto_scene_bounds_of_nodes.argtypes = [vp, C.c_int64, C.POINTER(C.c_float), C.c_float, C.POINTER(SceneBounds)]
    L.rto_split_plan_make.argtypes = [C.POINTER(SceneBounds), C.POINTER(Frame), C.c_int, C.c_int, C.c_int, C.POINTER(SplitPlan)]
    L.rto_split_part_of_rank.argtypes = [C.POINTER(SplitPlan), C.c_int]
    L.rto_split_rows_of_part.argtypes = [C.POINTER(SplitPlan), C.c_int]
    L.rto_split_row_source.argtypes = [C.POINTER(SplitPlan), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.rto_query_rays_device.argtypes = [vp, C.c_int, vp, C.c_int64, vp, vp]
    L.rto_query_rays_host.argtypes = [vp, C.c_int, vp, C.c_int64, vp]
    L.rto_query_pixels_device.argtypes = [vp, C.c_int, C.POINTER(Frame), vp, C.c_int64, vp, vp]
    L.rto_query_pixels_host.argtypes = [vp, C.c_int, C.POINTER(Frame), vp, C.c_int64, vp]
    L.rto_query_spans_device.argtypes = [vp, vp, C.c_int64, vp, vp]
    L.rto_query_spans_host.argtypes = [vp, vp, C.c_int64, vp]
    L.rto_query_span_pixels_device.argtypes = [vp, C.POINTER(Frame), vp, C.c_int64, vp, vp]
    L.rto_query_span_pixels_host.argtypes = [vp, C.POINTER(Frame), vp, C.c_int64, vp]
    L.rto_query_triangles_device.argtypes = [vp, C.c_int, vp, C.c_int64, vp, vp]
    L.rto_query_triangles_host.argtypes = [vp, C.c_int, vp, C.c_int64, vp]
    L.rto_query_triangle_pixels_device.argtypes = [vp, C.c_int, C.POINTER(Frame), vp, C.c_int64, vp, vp]
    L.rto_query_triangle_pixels_host.argtypes = [vp, C.c_int, C.POINTER(Frame), vp, C.c_int64, vp]
    L.rto_edit_voxels.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int64)]
    L.rto_download_voxels.argtypes = [vp, vp, C.c_int64, C.POINTER(C.c_int)]
    L.rto_last_edit_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rto_query_points_device.argtypes = [vp, vp, C.c_int64, vp, vp]
    L.rto_query_points_host.argtypes = [vp, vp, C.c_int64, vp]
    L.rto_query_regions_device.argtypes = [vp, vp, C.c_int64, vp, vp]
    L.rto_query_regions_host.argtypes = [vp, vp, C.c_int64, vp]
    L.rto_query_nearest_device.argtypes = [vp, vp, C.c_int64, vp, vp]
    L.rto_query_nearest_host.argtypes = [vp, vp, C.c_int64, vp]
    L.rto_point_quantize.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_int64)]
    L.rto_brush_quantize.argtypes = [vp, C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.rto_render_lit_device.argtypes = [vp, C.POINTER(Frame), C.POINTER(Lighting), vp, vp, vp]
    L.rto_render_lit_host.argtypes = [vp, C.POINTER(Frame), C.POINTER(Lighting), vp, vp]
    L.rto_render_lit_triangles_device.argtypes = [vp, C.POINTER(Frame), C.POINTER(Lighting), vp, vp, vp]
    L.rto_render_lit_triangles_host.argtypes = [vp, C.POINTER(Frame), C.POINTER(Lighting), vp, vp]
    L.rto_ao_directions.argtypes = [vp]
    L.rto_voxelize_mesh.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, C.POINTER(VoxelizeParams), C.POINTER(VoxelizeResult)]
    L.rto_last_voxelize_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rto_frustum_planes.argtypes = [C.POINTER(C.c_float), C.c_float, C.c_float, C.POINTER(C.c_float)]
    L.rto_extract_mesh.argtypes = [vp, C.c_int, C.POINTER(MeshCull), C.POINTER(C.c_int64)]
    L.rto_mesh_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int64)]
    L.rto_download_mesh.argtypes = [vp, vp, C.c_int64, vp, C.POINTER(C.c_int64)]
    L.rto_last_mesh_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rto_label_components.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int64)]
    L.rto_download_components.argtypes = [vp, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.rto_download_labels.argtypes = [vp, vp, C.c_int64]
    L.rto_labels_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int64)]
    L.rto_last_components_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rto_debug_components_passes.argtypes = [vp, C.POINTER(C.c_int)]
    L.rto_edit_components.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_int64)]
    L.rto_distance_field.argtypes = [vp, C.c_int, C.c_float, vp]
    L.rto_download_distance.argtypes = [vp, vp, C.c_int64]
    L.rto_distance_device.argtypes = [vp, C.POINTER(vp)]
    L.rto_last_distance_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rto_edit_morphology.argtypes = [vp, C.c_int, C.c_float, C.POINTER(C.c_int64)]
    L.rto_last_morphology_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rto_geodesic_field.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int64, C.c_int64, vp]
    L.rto_download_geodesic.argtypes = [vp, vp, C.c_int64]
    L.rto_geodesic_device.argtypes = [vp, C.POINTER(vp)]
    L.rto_geodesic_paths.argtypes = [vp, vp, C.c_int64, C.c_int64, vp, vp]
    L.rto_edit_geodesic.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
    L.rto_last_geodesic_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rto_last_geodesic_edit_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rto_debug_geodesic_passes.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.rto_debug_set_geodesic_look.argtypes = [vp, C.c_int]
    L.rto_skeleton_field.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int64, C.c_int64, vp]
    L.rto_download_skeleton.argtypes = [vp, vp, C.c_int64]
    L.rto_skeleton_device.argtypes = [vp, C.POINTER(vp)]
    L.rto_edit_skeleton.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
    L.rto_last_skeleton_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rto_last_skeleton_edit_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rto_debug_skeleton_passes.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.rto_debug_set_skeleton_look.argtypes = [vp, C.c_int]
    L.rto_exposure_field.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]
    L.rto_download_exposure.argtypes = [vp, vp, C.c_int64]
    L.rto_exposure_device.argtypes = [vp, C.POINTER(vp)]
    L.rto_last_exposure_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rto_dose_field.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.rto_download_dose.argtypes = [vp, vp, C.c_int64]
    L.rto_dose_device.argtypes = [vp, C.POINTER(vp)]
    L.rto_download_dose_coverage.argtypes = [vp, vp, C.c_int64]
    L.rto_last_dose_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rto_thickness_field.argtypes = [vp, C.c_int, C.c_float, vp]
    L.rto_download_thickness.argtypes = [vp, vp, C.c_int64]
    L.rto_thickness_device.argtypes = [vp, C.POINTER(vp)]
    L.rto_thickness_histogram.argtypes = [vp, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.rto_last_thickness_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rto_debug_thickness_table.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int64)]
    L.rto_measure_components.argtypes = [vp, vp]
    L.rto_download_measures.argtypes = [vp, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.rto_measures_device.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64)]
    L.rto_last_measure_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rto_segment_parts.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    L.rto_download_part_labels.argtypes = [vp, vp, C.c_int64]
    L.rto_download_parts.argtypes = [vp, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.rto_download_necks.argtypes = [vp, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.rto_parts_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(vp), C.POINTER(C.c_int64)]
    L.rto_edit_parts.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]
    L.rto_last_parts_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rto_debug_parts.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int64)]
    L.rto_debug_parts_capacity.argtypes = [vp, C.c_int64]
    L.rto_render_field_device.argtypes = [vp, C.POINTER(Frame), C.POINTER(FieldView), vp, vp, vp, vp, vp, vp, vp]
    L.rto_render_field_host.argtypes = [vp, C.POINTER(Frame), C.POINTER(FieldView), vp, vp, vp, vp, vp, vp]
    L.rto_last_field_view_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rto_project_field_device.argtypes = [vp, C.POINTER(Frame), C.POINTER(FieldProjection), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rto_project_field_host.argtypes = [vp, C.POINTER(Frame), C.POINTER(FieldProjection), vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rto_last_projection_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rto_debug_set_projection_table.argtypes = [vp, C.c_int]
    L.rto_composite_field_device.argtypes = [vp, C.POINTER(Frame), C.POINTER(FieldComposite), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rto_composite_field_host.argtypes = [vp, C.POINTER(Frame), C.POINTER(FieldComposite), vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rto_last_composite_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rto_extract_isosurface_device.argtypes = [vp, C.POINTER(IsoParams), vp, C.POINTER(IsoSummary)]
    L.rto_extract_isosurface_host.argtypes = [vp, C.POINTER(IsoParams), vp, C.POINTER(IsoSummary)]
    L.rto_isosurface_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int64)]
    L.rto_download_isosurface.argtypes = [vp, vp, C.c_int64, vp, C.POINTER(C.c_int64)]
    L.rto_last_isosurface_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rto_extract_dual_contour.argtypes = [vp, C.POINTER(DcParams), C.POINTER(DcSummary)]
    L.rto_dual_contour_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int64)]
    L.rto_download_dual_contour.argtypes = [vp, vp, C.c_int64, vp, C.POINTER(C.c_int64)]
    L.rto_last_dual_contour_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rto_query_dual_vertices_device.argtypes = [vp, vp, C.c_int64, vp]
    L.rto_query_dual_vertices_host.argtypes = [vp, vp, C.c_int64, vp]
    _lib = L
    return L


def make_frame(view, cam_pos, aspect, fov_deg, width, height) -> Frame:
    f = Frame()
    v = np.asarray(view, dtype=np.float32).reshape(16)
    p = np.asarray(cam_pos, dtype=np.float32).reshape(3)
    v = np.ascontiguousarray(v)
    p = np.ascontiguousarray(p)
    C.memmove(f.view, v.ctypes.data, 64)       # bit copies: no double rounding
    C.memmove(f.cam_pos, p.ctypes.data, 12)
    f.aspect = _f(aspect)
    f.fov_deg = _f(fov_deg)
    f.width, f.height = int(width), int(height)
    return f


class Context:
    """One rto_context == one GPU."""

    def __init__(self, device: int = 0):
        self._L = load()
        h = C.c_void_p()
        rc = self._L.rto_create(device, C.byref(h))
        if rc != RTO_OK:
            raise RtoError(rc, self._L.rto_last_error(None).decode())
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._L.rto_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != RTO_OK:
            raise RtoError(rc, self._L.rto_last_error(self._h).decode())

    def _last_ms(self, symbol: str, n: int):
        """The n device times an rto_last_*_ms entry reports, as a tuple."""
        ms = (C.c_float * n)()
        self._check(getattr(self._L, symbol)(self._h, ms))
        return tuple(ms)

    def _device_pointer(self, symbol: str) -> int:
        """The device pointer an rto_*_device entry of a resident int32 field reports."""
        p = C.c_void_p()
        self._check(getattr(self._L, symbol)(self._h, C.byref(p)))
        return p.value or 0

    def _resident_field(self, device_symbol: str, download_symbol: str, outputs: int = 1) -> np.ndarray:
        """A resident per-voxel int32 product as (dimZ, dimY, dimX).  The device getter is asked first, with none of its `outputs`
        wanted: when nothing is resident the error is its own, raised before the dims are asked for."""
        self._check(getattr(self._L, device_symbol)(self._h, *([None] * outputs)))
        dims = (C.c_int * 3)()
        self._check(self._L.rto_download_voxels(self._h, None, 0, dims))
        out = np.empty((dims[2], dims[1], dims[0]), np.int32)
        self._check(getattr(self._L, download_symbol)(self._h, out.ctypes.data, out.size))
        return out

    @property
    def device_name(self) -> str:
        buf = C.create_string_buffer(256)
        self._check(self._L.rto_device_name(self._h, buf, 256))
        return buf.value.decode()

    # -- octree ------------------------------------------------------------
    def upload_octree(self, nodes: np.ndarray, grid_min, voxel_size):
        nodes = np.ascontiguousarray(nodes)
        if nodes.dtype.itemsize != 60:
            raise RtoError(RTO_E_INVALID, "nodes must be an array of 60-byte GPUNodes records")
        gm = (C.c_float * 3)(*[_f(x) for x in grid_min])
        self._check(self._L.rto_upload_octree(self._h, nodes.ctypes.data, len(nodes), gm, _f(voxel_size)))

    def build_octree(self, voxels: np.ndarray, grid_min, voxel_size):
        """N4: createOctreeFromVoxelGrid + setOctree on the GPU. voxels: uint8 (dimZ, dimY, dimX), 0 EMPTY / 1 FILLED."""
        v = np.ascontiguousarray(voxels, dtype=np.uint8)
        dz, dy, dx = v.shape
        gm = (C.c_float * 3)(*[_f(x) for x in grid_min])
        self._check(self._L.rto_build_octree(self._h, v.ctypes.data, dx, dy, dz, gm, _f(voxel_size)))

    def debug_set_build_path(self, level_by_level: bool):
        """Force rto_build_octree's level-by-level form (True) or restore the automatic choice (False)."""
        self._check(self._L.rto_debug_set_build_path(self._h, 1 if level_by_level else 0))

    def download_nodes(self) -> np.ndarray:
        cnt = C.c_int64()
        self._check(self._L.rto_download_nodes(self._h, None, 0, C.byref(cnt)))
        out = np.zeros(cnt.value, NODE_DTYPE)
        self._check(self._L.rto_download_nodes(self._h, out.ctypes.data, cnt.value, C.byref(cnt)))
        return out

    def last_build_ms(self):
        k, u = C.c_float(), C.c_float()
        self._check(self._L.rto_last_build_ms(self._h, C.byref(k), C.byref(u)))
        return k.value, u.value

    def info(self) -> OctreeInfo:
        o = OctreeInfo()
        self._check(self._L.rto_octree_info_get(self._h, C.byref(o)))
        return o

    def set_kernel(self, kernel: int):
        self._check(self._L.rto_set_kernel(self._h, kernel))

    def set_launch_order(self, policy: int, refresh_period: int = 0):
        """0 = centre-out, 1 = temporal (an earlier frame's per-tile cost; default). refresh_period: rebuild the
        table every n-th frame (0 keeps the current period, default 4)."""
        self._check(self._L.rto_set_launch_order(self._h, policy, refresh_period))

    # -- culling -----------------------------------------------------------
    def update_frustum(self, view, fov_deg, aspect, enable=True):
        v = np.ascontiguousarray(np.asarray(view, dtype=np.float32).reshape(16))
        self._check(self._L.rto_update_frustum(self._h, v.ctypes.data_as(C.POINTER(C.c_float)),
                                               _f(fov_deg), _f(aspect), 1 if enable else 0))

    def debug_update_frustum_planes(self, planes, margin: float):
        """Developer aid: a frustum update with caller-supplied planes (6 x (nx, ny, nz, d), normalised) and margin."""
        pl = np.ascontiguousarray(np.asarray(planes, dtype=np.float32).reshape(24))
        self._check(self._L.rto_debug_update_frustum_planes(self._h, pl.ctypes.data_as(C.POINTER(C.c_float)), _f(margin)))

    def debug_set_frustum_shortcut(self, enabled: bool):
        """False: rto_update_frustum always runs its kernel (the host-side proof that no node can be culled is skipped)."""
        self._check(self._L.rto_debug_set_frustum_shortcut(self._h, 1 if enabled else 0))

    def debug_last_frustum_update_proven(self) -> bool:
        v = C.c_int()
        self._check(self._L.rto_debug_last_frustum_update_proven(self._h, C.byref(v)))
        return bool(v.value)

    def forget_stream(self, stream: int):
        """Drop the launch-order tables kept for `stream` (call before destroying the stream)."""
        self._check(self._L.rto_forget_stream(self._h, C.c_void_p(stream) if stream else None))

    def debug_set_exact_grid(self, enabled: bool = True):
        """Test / A-B hook (not part of rto_hip.h): False = the general 12-plane child test even on a grid whose node planes are computed
        without rounding; True = automatic (default).  Returns (the resident grid is exact, the 9-plane form is in use).  Pixels never depend on it."""
        fn = self._L.rto_debug_set_exact_grid
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        info = (C.c_int * 2)()
        self._check(fn(self._h, 1 if enabled else 0, info))
        return bool(info[0]), bool(info[1])

    def debug_set_tile_mask(self, mode):
        """0 / False: occupancy mask off; 1 / True: on (default); 2: on, built by a launch of its own in front of the frame and
        consulted by every wave (tests).  Pixels never depend on it."""
        self._check(self._L.rto_debug_set_tile_mask(self._h, int(mode)))

    def debug_tile_mask_info(self):
        """(depth the mask's cells are taken from, number of cells); (0, 0): no mask for this octree."""
        lv, n = C.c_int(), C.c_int()
        self._check(self._L.rto_debug_tile_mask_info(self._h, C.byref(lv), C.byref(n)))
        return lv.value, n.value

    def debug_sort_violations(self) -> int:
        n = C.c_int()
        self._check(self._L.rto_debug_sort_violations(self._h, C.byref(n)))
        return n.value

    def download_visible_nodes(self) -> np.ndarray:
        cnt = C.c_int64()
        self._check(self._L.rto_download_visible_nodes(self._h, None, 0, C.byref(cnt)))
        out = np.zeros(cnt.value, NODE_DTYPE)
        if cnt.value:
            self._check(self._L.rto_download_visible_nodes(self._h, out.ctypes.data, cnt.value, C.byref(cnt)))
        return out

    # -- render ------------------------------------------------------------
    def render_host(self, frame: Frame) -> np.ndarray:
        out = np.empty((frame.height, frame.width, 4), np.float32)
        self._check(self._L.rto_render_host(self._h, C.byref(frame), out.ctypes.data))
        return out

    def render_resident(self, frame: Frame, mode: int = 0):
        """Asynchronous render into the context's own device framebuffer (0 octree, 1 triangles, 2 triangles + shadow)."""
        self._check(self._L.rto_render_resident(self._h, C.byref(frame), mode))

    def resident_frame(self):
        """(device pointer, width, height) of the frame render_resident left on the GPU."""
        p, w, h = C.c_void_p(), C.c_int(), C.c_int()
        self._check(self._L.rto_resident_frame(self._h, C.byref(p), C.byref(w), C.byref(h)))
        return p.value, w.value, h.value

    def download_resident(self) -> np.ndarray:
        _, w, h = self.resident_frame()
        out = np.empty((h, w, 4), np.float32)
        self._check(self._L.rto_download_resident(self._h, out.ctypes.data))
        return out

    def render_device(self, frame: Frame, d_out: int, part: Partition | None = None, stream: int = 0):
        self._check(self._L.rto_render_device(self._h, C.byref(frame), C.byref(part) if part else None,
                                              C.c_void_p(d_out), C.c_void_p(stream) if stream else None))

    def assemble_device(self, frame: Frame, part: Partition, d_gathered: int, d_frame: int, stream: int = 0):
        self._check(self._L.rto_assemble_device(self._h, C.byref(frame), C.byref(part), C.c_void_p(d_gathered),
                                                C.c_void_p(d_frame), C.c_void_p(stream) if stream else None))

    def render_shade_device(self, frame: Frame, d_shade: int, part: Partition | None = None, stream: int = 0):
        """4 bytes per pixel (Lambert term of the hit, -1 = miss): the multi-GPU gather payload."""
        self._check(self._L.rto_render_shade_device(self._h, C.byref(frame), C.byref(part) if part else None,
                                                    C.c_void_p(d_shade), C.c_void_p(stream) if stream else None))

    def assemble_shade_device(self, frame: Frame, part: Partition, d_gathered: int, d_frame: int, stream: int = 0):
        self._check(self._L.rto_assemble_shade_device(self._h, C.byref(frame), C.byref(part), C.c_void_p(d_gathered),
                                                      C.c_void_p(d_frame), C.c_void_p(stream) if stream else None))

    def assemble_batch_device(self, frame: Frame, part: Partition, d_gathered: int, batch: int, index: int, shade: bool, d_frame: int,
                              stream: int = 0):
        """Frame `index` of a gather that carried `batch` frames per rank ([rank][batch][rows][width])."""
        self._check(self._L.rto_assemble_batch_device(self._h, C.byref(frame), C.byref(part), C.c_void_p(d_gathered), batch, index,
                                                      1 if shade else 0, C.c_void_p(d_frame), C.c_void_p(stream) if stream else None))

    @staticmethod
    def frame_array(frames):
        """ctypes array of rto_frame for the batch entry points (build once per batch)."""
        return (Frame * len(frames))(*frames)

    def render_batch_device(self, frames_arr, d_out: int, frame_stride_bytes: int, part: Partition | None, shade: bool, stream: int = 0):
        self._check(self._L.rto_render_batch_device(self._h, frames_arr, len(frames_arr), C.byref(part) if part else None, 1 if shade else 0,
                                                    C.c_void_p(d_out), frame_stride_bytes, C.c_void_p(stream) if stream else None))

    def render_triangles_batch_device(self, frames_arr, d_out: int, frame_stride_bytes: int, shadow: bool = True, part: Partition | None = None,
                                      shade: bool = False, stream: int = 0):
        """Config 5's frames, up to 8 per kernel launch (rto_render_triangles_batch_device)."""
        self._check(self._L.rto_render_triangles_batch_device(self._h, frames_arr, len(frames_arr), C.byref(part) if part else None,
                                                              1 if shadow else 0, 1 if shade else 0, C.c_void_p(d_out), frame_stride_bytes,
                                                              C.c_void_p(stream) if stream else None))

    def assemble_batch_all_device(self, frames_arr, part: Partition, d_gathered: int, shade: bool, d_frames: int, frame_stride_bytes: int,
                                  stream: int = 0):
        self._check(self._L.rto_assemble_batch_all_device(self._h, frames_arr, len(frames_arr), C.byref(part), C.c_void_p(d_gathered),
                                                          1 if shade else 0, C.c_void_p(d_frames), frame_stride_bytes,
                                                          C.c_void_p(stream) if stream else None))

    def partition_rows(self, frame: Frame, part: Partition | None) -> int:
        return self._L.rto_partition_rows(C.byref(frame), C.byref(part) if part else None)

    def upload_leaf_triangles(self, tris: np.ndarray, tri_offset: np.ndarray):
        """Config 5: tris (n, 12) float32 = v0, v1, v2, face normal; tri_offset (numNodes+1,) int32."""
        tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 12)
        off = np.ascontiguousarray(tri_offset, dtype=np.int32)
        self._keep_tris = (tris, off)
        self._check(self._L.rto_upload_leaf_triangles(self._h, tris.ctypes.data if len(tris) else None, len(tris), off.ctypes.data))

    def build_leaf_triangles(self, voxels: np.ndarray | None = None):
        """Config 5: the leaf-triangle buffer built on the GPU for the resident octree.  voxels: uint8 (dimZ, dimY, dimX);
        None reuses the voxels rto_build_octree kept in HBM."""
        if voxels is None:
            self._check(self._L.rto_build_leaf_triangles(self._h, None, 0, 0, 0))
            return
        v = np.ascontiguousarray(voxels, dtype=np.uint8)
        dz, dy, dx = v.shape
        self._check(self._L.rto_build_leaf_triangles(self._h, v.ctypes.data, dx, dy, dz))

    def download_leaf_triangles(self):
        n = C.c_int64()
        self._check(self._L.rto_download_leaf_triangles(self._h, None, 0, None, C.byref(n)))
        tris = np.zeros((n.value, 12), np.float32)
        off = np.zeros(self.info().num_nodes + 1, np.int32)
        self._check(self._L.rto_download_leaf_triangles(self._h, tris.ctypes.data if n.value else None, n.value, off.ctypes.data, C.byref(n)))
        return tris, off

    def render_triangles_host(self, frame: Frame, shadow: bool = True, stats: bool = False):
        out = np.empty((frame.height, frame.width, 4), np.float32)
        s = Stats()
        self._check(self._L.rto_render_triangles_host(self._h, C.byref(frame), 1 if shadow else 0, out.ctypes.data,
                                                      C.byref(s) if stats else None))
        return (out, {"rays": s.rays, "pops": s.pops, "hits": s.hits}) if stats else out

    def render_triangles_device(self, frame: Frame, d_out: int, shadow: bool = True, part: Partition | None = None, stream: int = 0):
        self._check(self._L.rto_render_triangles_device(self._h, C.byref(frame), C.byref(part) if part else None,
                                                        1 if shadow else 0, C.c_void_p(d_out), C.c_void_p(stream) if stream else None))

    def render_triangles_shade_device(self, frame: Frame, d_shade: int, shadow: bool = True, part: Partition | None = None, stream: int = 0):
        self._check(self._L.rto_render_triangles_shade_device(self._h, C.byref(frame), C.byref(part) if part else None,
                                                              1 if shadow else 0, C.c_void_p(d_shade), C.c_void_p(stream) if stream else None))

    def octree_ray_skip(self, ro, rd, t_min=0.0, t_max=1e30, use_visibility=False) -> np.ndarray:
        """octreeRaySkip (VolumeRaycastRenderer.cpp:50-155) for n rays sharing the origin ro; rd: (n, 3)."""
        rd = np.ascontiguousarray(rd, dtype=np.float32).reshape(-1, 3)
        out = np.empty(len(rd), np.float32)
        o = (C.c_float * 3)(*[_f(x) for x in ro])
        self._check(self._L.rto_octree_ray_skip(self._h, o, rd.ctypes.data, len(rd), _f(t_min), _f(t_max),
                                                1 if use_visibility else 0, out.ctypes.data))
        return out

    # -- ray queries -------------------------------------------------------
    def query_rays(self, origins, dirs, t_min=0.0, t_max=1e30, mode: int = QUERY_CLOSEST) -> np.ndarray:
        """Trace caller-supplied rays through the whole resident octree (rto_query_rays_host).  origins: (n, 3) or one origin,
        dirs: (n, 3), t_min / t_max: scalars or per-ray arrays.  Returns a HIT_DTYPE array (node -1, t 1e30 for a miss)."""
        return self.query_ray_records(make_rays(origins, dirs, t_min, t_max), mode)

    def query_ray_records(self, rays: np.ndarray, mode: int = QUERY_CLOSEST) -> np.ndarray:
        """The same for a RAY_DTYPE array."""
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        hits = np.zeros(len(rays), HIT_DTYPE)
        self._check(self._L.rto_query_rays_host(self._h, int(mode), rays.ctypes.data, len(rays), hits.ctypes.data))
        return hits

    def query_rays_device(self, mode: int, d_rays: int, n: int, d_hits: int, stream: int = 0):
        """Asynchronous: n rto_ray records at d_rays -> n rto_hit records at d_hits (device pointers, 16-byte aligned)."""
        self._check(self._L.rto_query_rays_device(self._h, int(mode), C.c_void_p(d_rays) if d_rays else None, int(n),
                                                  C.c_void_p(d_hits) if d_hits else None, C.c_void_p(stream) if stream else None))

    def query_pixels(self, frame: Frame, xy, mode: int = QUERY_FIRST) -> np.ndarray:
        """The renders' own rays through pixels (x, y) of `frame` (row 0 = top): xy (n, 2) int; a HIT_DTYPE array."""
        xy = np.ascontiguousarray(np.asarray(xy, np.int32).reshape(-1, 2))
        hits = np.zeros(len(xy), HIT_DTYPE)
        self._check(self._L.rto_query_pixels_host(self._h, int(mode), C.byref(frame), xy.ctypes.data, len(xy), hits.ctypes.data))
        return hits

    def query_pixels_device(self, mode: int, frame: Frame, d_xy: int, n: int, d_hits: int, stream: int = 0):
        self._check(self._L.rto_query_pixels_device(self._h, int(mode), C.byref(frame), C.c_void_p(d_xy) if d_xy else None, int(n),
                                                    C.c_void_p(d_hits) if d_hits else None, C.c_void_p(stream) if stream else None))

    # -- span queries ------------------------------------------------------
    def query_spans(self, origins, dirs, t_min=0.0, t_max=1e30) -> np.ndarray:
        """How much solid each ray passes through (rto_query_spans_host): origins (n, 3) or one origin, dirs (n, 3), t_min / t_max
        scalars or per-ray arrays.  Returns a SPAN_DTYPE array (length 0, leaves 0, node -1, t_enter = t_exit = 1e30 for a miss)."""
        return self.query_span_records(make_rays(origins, dirs, t_min, t_max))

    def query_span_records(self, rays: np.ndarray) -> np.ndarray:
        """The same for a RAY_DTYPE array."""
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        spans = np.zeros(len(rays), SPAN_DTYPE)
        self._check(self._L.rto_query_spans_host(self._h, rays.ctypes.data, len(rays), spans.ctypes.data))
        return spans

    def query_spans_device(self, d_rays: int, n: int, d_spans: int, stream: int = 0):
        """Asynchronous: n rto_ray records at d_rays -> n rto_span records at d_spans (device pointers, 16-byte aligned)."""
        self._check(self._L.rto_query_spans_device(self._h, C.c_void_p(d_rays) if d_rays else None, int(n),
                                                   C.c_void_p(d_spans) if d_spans else None, C.c_void_p(stream) if stream else None))

    def query_span_pixels(self, frame: Frame, xy) -> np.ndarray:
        """The renders' own rays through pixels (x, y) of `frame` (row 0 = top): xy (n, 2) int; a SPAN_DTYPE array."""
        xy = np.ascontiguousarray(np.asarray(xy, np.int32).reshape(-1, 2))
        spans = np.zeros(len(xy), SPAN_DTYPE)
        self._check(self._L.rto_query_span_pixels_host(self._h, C.byref(frame), xy.ctypes.data, len(xy), spans.ctypes.data))
        return spans

    def query_span_pixels_device(self, frame: Frame, d_xy: int, n: int, d_spans: int, stream: int = 0):
        self._check(self._L.rto_query_span_pixels_device(self._h, C.byref(frame), C.c_void_p(d_xy) if d_xy else None, int(n),
                                                         C.c_void_p(d_spans) if d_spans else None, C.c_void_p(stream) if stream else None))

    # -- lit render ----------------------------------------------------------
    def render_lit_host(self, frame: Frame, lighting: Lighting | None = None, vis: bool = False, **kw):
        """The box render's frame with a shadow ray and ambient occlusion (rto_render_lit_host).  lighting: a Lighting, or
        make_lighting's keywords.  Returns the (H, W, 4) float32 frame, or (frame, (H, W) int32 visibility) with vis=True."""
        L = lighting if lighting is not None else make_lighting(**kw)
        out = np.empty((frame.height, frame.width, 4), np.float32)
        v = np.empty((frame.height, frame.width), np.int32) if vis else None
        self._check(self._L.rto_render_lit_host(self._h, C.byref(frame), C.byref(L), out.ctypes.data,
                                                v.ctypes.data if vis else None))
        return (out, v) if vis else out

    def render_lit_device(self, frame: Frame, lighting: Lighting, d_rgba: int, d_vis: int = 0, stream: int = 0):
        """Asynchronous: the lit frame into d_rgba (W*H*16 bytes) and, if d_vis, the visibility into d_vis (W*H int32)."""
        self._check(self._L.rto_render_lit_device(self._h, C.byref(frame), C.byref(lighting), C.c_void_p(d_rgba) if d_rgba else None,
                                                  C.c_void_p(d_vis) if d_vis else None, C.c_void_p(stream) if stream else None))

    def render_lit_triangles_host(self, frame: Frame, lighting: Lighting | None = None, vis: bool = False, **kw):
        """The triangle render's frame with a shadow ray and ambient occlusion (rto_render_lit_triangles_host); arguments and
        result as render_lit_host."""
        L = lighting if lighting is not None else make_lighting(**kw)
        out = np.empty((frame.height, frame.width, 4), np.float32)
        v = np.empty((frame.height, frame.width), np.int32) if vis else None
        self._check(self._L.rto_render_lit_triangles_host(self._h, C.byref(frame), C.byref(L), out.ctypes.data,
                                                          v.ctypes.data if vis else None))
        return (out, v) if vis else out

    def render_lit_triangles_device(self, frame: Frame, lighting: Lighting, d_rgba: int, d_vis: int = 0, stream: int = 0):
        """Asynchronous: the lit triangle frame into d_rgba (W*H*16 bytes) and, if d_vis, the visibility into d_vis (W*H int32)."""
        self._check(self._L.rto_render_lit_triangles_device(self._h, C.byref(frame), C.byref(lighting),
                                                            C.c_void_p(d_rgba) if d_rgba else None, C.c_void_p(d_vis) if d_vis else None,
                                                            C.c_void_p(stream) if stream else None))

    @staticmethod
    def ao_directions() -> np.ndarray:
        return ao_directions()

    # -- field views ---------------------------------------------------------
    def render_field_host(self, frame: Frame, view: FieldView, lut, volume=None):
        """A frame coloured by an int32 volume of the resident grid (rto_render_field_host).  lut: 256 uint32 (ramp_lut);
        volume: the (dimZ, dimY, dimX) int32 array of FIELD_CALLER, None for every other source.  Returns (rgba (H, W, 4)
        float32, values (H, W) int32, summary (one FIELD_VIEW_SUMMARY_DTYPE record), bins (256,) int64)."""
        lut = np.ascontiguousarray(lut, dtype=np.uint32)
        if lut.shape != (256,):
            raise ValueError("render_field_host: the LUT has 256 entries")
        if volume is not None:
            volume = np.ascontiguousarray(volume, dtype=np.int32)
            dims = (C.c_int * 3)()
            if self._L.rto_download_voxels(self._h, None, 0, dims) == RTO_OK and volume.shape != (dims[2], dims[1], dims[0]):
                raise ValueError(f"render_field_host: the volume must be {(dims[2], dims[1], dims[0])}, not {volume.shape}")
        rgba = np.empty((frame.height, frame.width, 4), np.float32)
        values = np.empty((frame.height, frame.width), np.int32)
        summary = np.zeros(1, FIELD_VIEW_SUMMARY_DTYPE)
        bins = np.zeros(256, np.int64)
        self._check(self._L.rto_render_field_host(self._h, C.byref(frame), C.byref(view), lut.ctypes.data,
                                                  volume.ctypes.data if volume is not None else None, rgba.ctypes.data,
                                                  values.ctypes.data, summary.ctypes.data, bins.ctypes.data))
        return rgba, values, summary[0], bins

    def render_field_device(self, frame: Frame, view: FieldView, d_lut: int, d_rgba: int, d_volume: int = 0, d_values: int = 0,
                            d_summary: int = 0, d_bins: int = 0, stream: int = 0):
        """Asynchronous: the field view into d_rgba (W*H*16 bytes) and, where given, the values (W*H int32), the summary (32 bytes)
        and the 256 int64 bins; d_lut: 256 uint32 on the device; d_volume: the device volume of FIELD_CALLER."""
        p = lambda x: C.c_void_p(x) if x else None
        self._check(self._L.rto_render_field_device(self._h, C.byref(frame), C.byref(view), p(d_lut), p(d_volume), p(d_rgba),
                                                    p(d_values), p(d_summary), p(d_bins), p(stream)))

    def last_field_view_ms(self):
        """(sample kernel, shade kernel) of the last field view in ms; -1: not run."""
        return self._last_ms("rto_last_field_view_ms", 2)

    # -- field projections -----------------------------------------------------
    def project_field_host(self, frame: Frame, projection: FieldProjection, lut, volume=None, totals: bool = True):
        """A frame whose pixels reduce an int32 volume of the resident grid along their rays (rto_project_field_host).  lut: 256
        uint32 (ramp_lut); volume: the (dimZ, dimY, dimX) int32 array of FIELD_CALLER, None for every other source.  Returns (rgba
        (H, W, 4) float32, values (H, W) int32, voxels (H, W) int32, sums (H, W) int64, counts (H, W) int32, summary (one
        FIELD_VIEW_SUMMARY_DTYPE record), bins (256,) int64); totals=False asks for neither sums nor counts (both None), which lets
        MAX, MIN and FIRST skip or stop on more than empty bricks."""
        lut = np.ascontiguousarray(lut, dtype=np.uint32)
        if lut.shape != (256,):
            raise ValueError("project_field_host: the LUT has 256 entries")
        if volume is not None:
            volume = np.ascontiguousarray(volume, dtype=np.int32)
            dims = (C.c_int * 3)()
            if self._L.rto_download_voxels(self._h, None, 0, dims) == RTO_OK and volume.shape != (dims[2], dims[1], dims[0]):
                raise ValueError(f"project_field_host: the volume must be {(dims[2], dims[1], dims[0])}, not {volume.shape}")
        shape = (frame.height, frame.width)
        rgba = np.empty(shape + (4,), np.float32)
        values, voxels = np.empty(shape, np.int32), np.empty(shape, np.int32)
        sums = np.empty(shape, np.int64) if totals else None
        counts = np.empty(shape, np.int32) if totals else None
        summary = np.zeros(1, FIELD_VIEW_SUMMARY_DTYPE)
        bins = np.zeros(256, np.int64)
        self._check(self._L.rto_project_field_host(self._h, C.byref(frame), C.byref(projection), lut.ctypes.data,
                                                   volume.ctypes.data if volume is not None else None, rgba.ctypes.data,
                                                   values.ctypes.data, voxels.ctypes.data, sums.ctypes.data if totals else None,
                                                   counts.ctypes.data if totals else None, summary.ctypes.data, bins.ctypes.data))
        return rgba, values, voxels, sums, counts, summary[0], bins

    def project_field_device(self, frame: Frame, projection: FieldProjection, d_lut: int, d_rgba: int, d_volume: int = 0,
                             d_values: int = 0, d_voxels: int = 0, d_sums: int = 0, d_counts: int = 0, d_summary: int = 0,
                             d_bins: int = 0, stream: int = 0):
        """Asynchronous: the projection into d_rgba (W*H*16 bytes) and, where given, the values, voxels and counts (W*H int32
        each), the sums (W*H int64), the summary (32 bytes) and the 256 int64 bins; d_lut: 256 uint32 on the device; d_volume: the
        device volume of FIELD_CALLER."""
        p = lambda x: C.c_void_p(x) if x else None
        self._check(self._L.rto_project_field_device(self._h, C.byref(frame), C.byref(projection), p(d_lut), p(d_volume), p(d_rgba),
                                                     p(d_values), p(d_voxels), p(d_sums), p(d_counts), p(d_summary), p(d_bins),
                                                     p(stream)))

    def last_projection_ms(self):
        """(brick table, march, shade kernel) of the last projection in ms; -1: not run."""
        return self._last_ms("rto_last_projection_ms", 3)

    def debug_set_projection_table(self, enabled: bool):
        """rto_debug_set_projection_table: whether the march consults the brick table (default) or walks every voxel."""
        self._check(self._L.rto_debug_set_projection_table(self._h, 1 if enabled else 0))

    # -- field compositing -----------------------------------------------------
    def composite_field_host(self, frame: Frame, composite: FieldComposite, lut, volume=None, under=None, in_place: bool = False):
        """A frame in which an int32 volume of the resident grid is seen through: LUT colour and opacity per valued voxel,
        composited front to back along the pixel rays (rto_composite_field_host).  lut: 256 uint32 (ramp_lut; the alpha byte is
        the voxel's opacity); volume: the (dimZ, dimY, dimX) int32 array of FIELD_CALLER, None for every other source; under: an (H,
        W, 4) float32 frame to composite over, None for the composite's background_rgba and miss_rgba; in_place: the frame is
        composited over `under` in one buffer, on the host and on the device.  Returns (rgba (H, W, 4) float32, transmittance (H, W)
        uint32, first (H, W) int32, stops (H, W) int32, counts (H, W) int32, summary (one COMPOSITE_SUMMARY_DTYPE record))."""
        lut = np.ascontiguousarray(lut, dtype=np.uint32)
        if lut.shape != (256,):
            raise ValueError("composite_field_host: the LUT has 256 entries")
        if volume is not None:
            volume = np.ascontiguousarray(volume, dtype=np.int32)
            dims = (C.c_int * 3)()
            if self._L.rto_download_voxels(self._h, None, 0, dims) == RTO_OK and volume.shape != (dims[2], dims[1], dims[0]):
                raise ValueError(f"composite_field_host: the volume must be {(dims[2], dims[1], dims[0])}, not {volume.shape}")
        shape = (frame.height, frame.width)
        if under is not None:
            under = np.array(under, dtype=np.float32, order="C") if in_place else np.ascontiguousarray(under, dtype=np.float32)
            if under.shape != shape + (4,):
                raise ValueError(f"composite_field_host: under must be {shape + (4,)}, not {under.shape}")
        elif in_place:
            raise ValueError("composite_field_host: in_place needs a frame to composite over")
        rgba = under if in_place else np.empty(shape + (4,), np.float32)
        trans = np.empty(shape, np.uint32)
        first, stops, counts = np.empty(shape, np.int32), np.empty(shape, np.int32), np.empty(shape, np.int32)
        summary = np.zeros(1, COMPOSITE_SUMMARY_DTYPE)
        self._check(self._L.rto_composite_field_host(self._h, C.byref(frame), C.byref(composite), lut.ctypes.data,
                                                     volume.ctypes.data if volume is not None else None,
                                                     under.ctypes.data if under is not None else None, rgba.ctypes.data,
                                                     trans.ctypes.data, first.ctypes.data, stops.ctypes.data, counts.ctypes.data,
                                                     summary.ctypes.data))
        return rgba, trans, first, stops, counts, summary[0]

    def composite_field_device(self, frame: Frame, composite: FieldComposite, d_lut: int, d_rgba: int, d_volume: int = 0,
                               d_under: int = 0, d_transmittance: int = 0, d_first: int = 0, d_stops: int = 0, d_counts: int = 0,
                               d_summary: int = 0, stream: int = 0):
        """Asynchronous: the composite into d_rgba (W*H*16 bytes), over d_under (the same size; it may be d_rgba) when given, and,
        where given, the transmittance (W*H uint32), the first and the stopping voxel and the counts (W*H int32 each) and the
        summary (32 bytes); d_lut: 256 uint32 on the device; d_volume: the device volume of FIELD_CALLER."""
        p = lambda x: C.c_void_p(x) if x else None
        self._check(self._L.rto_composite_field_device(self._h, C.byref(frame), C.byref(composite), p(d_lut), p(d_volume), p(d_under),
                                                       p(d_rgba), p(d_transmittance), p(d_first), p(d_stops), p(d_counts), p(d_summary),
                                                       p(stream)))

    def last_composite_ms(self):
        """(tables, march, summary fold) of the last composite in ms; -1: not run."""
        return self._last_ms("rto_last_composite_ms", 3)

    # -- triangle queries (the resident leaf triangles) --------------------
    def query_triangles(self, origins, dirs, t_min=0.0, t_max=1e30, mode: int = QUERY_CLOSEST) -> np.ndarray:
        """Caller-supplied rays against the resident leaf triangles (rto_query_triangles_host): origins (n, 3) or one origin,
        dirs (n, 3), t_min / t_max scalars or per-ray arrays.  Returns a TRI_HIT_DTYPE array (tri -1, t 1e30 for a miss)."""
        return self.query_triangle_records(make_rays(origins, dirs, t_min, t_max), mode)

    def query_triangle_records(self, rays: np.ndarray, mode: int = QUERY_CLOSEST) -> np.ndarray:
        """The same for a RAY_DTYPE array."""
        rays = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
        hits = np.zeros(len(rays), TRI_HIT_DTYPE)
        self._check(self._L.rto_query_triangles_host(self._h, int(mode), rays.ctypes.data, len(rays), hits.ctypes.data))
        return hits

    def query_triangles_device(self, mode: int, d_rays: int, n: int, d_hits: int, stream: int = 0):
        """Asynchronous: n rto_ray records at d_rays -> n rto_tri_hit records at d_hits (device pointers, 16-byte aligned)."""
        self._check(self._L.rto_query_triangles_device(self._h, int(mode), C.c_void_p(d_rays) if d_rays else None, int(n),
                                                       C.c_void_p(d_hits) if d_hits else None, C.c_void_p(stream) if stream else None))

    def query_triangle_pixels(self, frame: Frame, xy, mode: int = QUERY_FIRST) -> np.ndarray:
        """The renders' own rays through pixels (x, y) of `frame` against the leaf triangles: a TRI_HIT_DTYPE array.  FIRST gives
        the triangle and t render_triangles_* shades there."""
        xy = np.ascontiguousarray(np.asarray(xy, np.int32).reshape(-1, 2))
        hits = np.zeros(len(xy), TRI_HIT_DTYPE)
        self._check(self._L.rto_query_triangle_pixels_host(self._h, int(mode), C.byref(frame), xy.ctypes.data, len(xy),
                                                           hits.ctypes.data))
        return hits

    def query_triangle_pixels_device(self, mode: int, frame: Frame, d_xy: int, n: int, d_hits: int, stream: int = 0):
        self._check(self._L.rto_query_triangle_pixels_device(self._h, int(mode), C.byref(frame), C.c_void_p(d_xy) if d_xy else None,
                                                             int(n), C.c_void_p(d_hits) if d_hits else None,
                                                             C.c_void_p(stream) if stream else None))

    def render_closest_host(self, frame: Frame, stats: bool = False):
        """The reference's closest-hit traversal (its earlier, block-commented shader): RGBA frame [, {rays, pops, hits}]."""
        out = np.empty((frame.height, frame.width, 4), np.float32)
        st = Stats()
        self._check(self._L.rto_render_closest_host(self._h, C.byref(frame), out.ctypes.data, C.byref(st) if stats else None))
        return (out, {"rays": st.rays, "pops": st.pops, "hits": st.hits}) if stats else out

    def render_closest_device(self, frame: Frame, d_out: int, part: Partition | None = None, stream: int = 0):
        self._check(self._L.rto_render_closest_device(self._h, C.byref(frame), C.byref(part) if part else None, C.c_void_p(d_out), C.c_void_p(stream)))

    def render_skip_host(self, frame: Frame, use_visibility=False, rgba=True, dist=True):
        """Nearest-hit render mode (octreeRaySkip per pixel): (rgba (H, W, 4) or None, dist (H, W) or None)."""
        o_rgba = np.empty((frame.height, frame.width, 4), np.float32) if rgba else None
        o_dist = np.empty((frame.height, frame.width), np.float32) if dist else None
        self._check(self._L.rto_render_skip_host(self._h, C.byref(frame), 1 if use_visibility else 0,
                                                 o_rgba.ctypes.data if rgba else None, o_dist.ctypes.data if dist else None))
        return o_rgba, o_dist

    def render_skip_device(self, frame: Frame, d_rgba: int, d_dist: int, use_visibility=False, part: Partition | None = None, stream: int = 0):
        self._check(self._L.rto_render_skip_device(self._h, C.byref(frame), C.byref(part) if part else None, 1 if use_visibility else 0,
                                                   C.c_void_p(d_rgba) if d_rgba else None, C.c_void_p(d_dist) if d_dist else None,
                                                   C.c_void_p(stream) if stream else None))

    def probe_skip_host(self, view, cam_pos, aspect, last=0.0, use_visibility=False, with_probes=False):
        """octreeSkipT as drawRaycast computes it, one launch: returns the new value (and the 49 probe distances)."""
        v = np.ascontiguousarray(np.asarray(view, dtype=np.float32).reshape(16))
        p = np.ascontiguousarray(np.asarray(cam_pos, dtype=np.float32).reshape(3))
        io = C.c_float(_f(last))
        probes = np.zeros(49, np.float32) if with_probes else None
        self._check(self._L.rto_probe_skip_host(self._h, v.ctypes.data_as(C.POINTER(C.c_float)), p.ctypes.data_as(C.POINTER(C.c_float)), _f(aspect),
                                                1 if use_visibility else 0, C.byref(io), probes.ctypes.data if with_probes else None))
        return (np.float32(io.value), probes) if with_probes else np.float32(io.value)

    def probe_skip_device(self, view, cam_pos, aspect, d_skip: int, use_visibility=False, stream: int = 0):
        v = np.ascontiguousarray(np.asarray(view, dtype=np.float32).reshape(16))
        p = np.ascontiguousarray(np.asarray(cam_pos, dtype=np.float32).reshape(3))
        self._check(self._L.rto_probe_skip_device(self._h, v.ctypes.data_as(C.POINTER(C.c_float)), p.ctypes.data_as(C.POINTER(C.c_float)), _f(aspect),
                                                  1 if use_visibility else 0, C.c_void_p(d_skip), C.c_void_p(stream) if stream else None))

    def frame_stats(self, frame: Frame) -> dict:
        s = Stats()
        self._check(self._L.rto_frame_stats(self._h, C.byref(frame), C.byref(s)))
        return {"rays": s.rays, "pops": s.pops, "hits": s.hits, "capped": s.capped}

    def render_steps(self, frame: Frame) -> np.ndarray:
        out = np.zeros((frame.height, frame.width), np.int32)
        self._check(self._L.rto_render_steps_host(self._h, C.byref(frame), out.ctypes.data))
        return out

    def debug_timeline(self, frame: Frame) -> np.ndarray:
        """(tiles, 8) int32 records, see rto_debug_timeline."""
        n = C.c_int64()
        self._check(self._L.rto_debug_timeline(self._h, C.byref(frame), None, 0, C.byref(n)))
        out = np.zeros((n.value, 8), np.int32)
        self._check(self._L.rto_debug_timeline(self._h, C.byref(frame), out.ctypes.data, n.value, C.byref(n)))
        return out

    def debug_tile_cost(self) -> np.ndarray:
        n = C.c_int64()
        self._check(self._L.rto_debug_tile_cost(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.int32)
        self._check(self._L.rto_debug_tile_cost(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def debug_set_tile_order(self, order):
        if order is None:
            self._check(self._L.rto_debug_set_tile_order(self._h, None, 0))
            return
        o = np.ascontiguousarray(order, dtype=np.int32)
        self._check(self._L.rto_debug_set_tile_order(self._h, o.ctypes.data, len(o)))

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        self._check(self._L.rto_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def timing_begin(self, capacity: int):
        self._check(self._L.rto_timing_begin(self._h, capacity))

    def timing_read(self) -> np.ndarray:
        n = C.c_int()
        self._check(self._L.rto_timing_read(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.float32)
        if n.value:
            self._check(self._L.rto_timing_read(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out

    # -- voxel edits -----------------------------------------------------------
    def edit_voxels(self, brushes) -> int:
        """rto_edit_voxels: apply BRUSH_DTYPE brushes (make_brushes) to the resident grid in order and rebuild; the number of
        voxels that changed."""
        b = np.ascontiguousarray(np.asarray(brushes, BRUSH_DTYPE).reshape(-1))
        changed = C.c_int64()
        self._check(self._L.rto_edit_voxels(self._h, b.ctypes.data if len(b) else None, len(b), C.byref(changed)))
        return changed.value

    def download_voxels(self) -> np.ndarray:
        """The resident grid as uint8 (dimZ, dimY, dimX): build_octree's input layout."""
        dims = (C.c_int * 3)()
        self._check(self._L.rto_download_voxels(self._h, None, 0, dims))
        out = np.empty((dims[2], dims[1], dims[0]), np.uint8)
        self._check(self._L.rto_download_voxels(self._h, out.ctypes.data, out.size, dims))
        return out

    def last_edit_ms(self):
        """Device ms of the last edit: (brushes, octree rebuild, triangle rebuild); -1 for a step that did not run."""
        return self._last_ms("rto_last_edit_ms", 3)

    # -- connected components --------------------------------------------------
    def label_components(self, set: int = SET_SOLID, connectivity: int = CONN_FACE) -> np.ndarray:
        """rto_label_components: label the resident grid's SET_SOLID or SET_EMPTY voxels under CONN_FACE (6) or CONN_FULL (26); the
        table as a COMPONENT_DTYPE array in ascending order of root.  Labels and table stay resident until the grid changes."""
        n = C.c_int64()
        self._check(self._L.rto_label_components(self._h, int(set), int(connectivity), C.byref(n)))
        out = np.zeros(n.value, COMPONENT_DTYPE)
        if n.value:
            self._check(self._L.rto_download_components(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def components(self) -> np.ndarray:
        """The resident table (rto_download_components)."""
        n = C.c_int64()
        self._check(self._L.rto_download_components(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, COMPONENT_DTYPE)
        if n.value:
            self._check(self._L.rto_download_components(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def component_labels(self) -> np.ndarray:
        """The resident label volume as int32 (dimZ, dimY, dimX): the component's number, -1 outside the set."""
        return self._resident_field("rto_labels_device", "rto_download_labels", outputs=3)

    def component_labels_device(self):
        """(device pointer of the int32 label volume, device pointer of the 48-byte table records, count)."""
        l, t, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        self._check(self._L.rto_labels_device(self._h, C.byref(l), C.byref(t), C.byref(n)))
        return l.value or 0, t.value or 0, n.value

    def last_components_ms(self):
        """Device ms of the last labelling: (tile-local labelling, merging, flatten + ranking, statistics); -1: not run."""
        return self._last_ms("rto_last_components_ms", 4)

    def components_passes(self) -> int:
        """Merge launches of the last labelling (2: one merge, one clean check)."""
        n = C.c_int()
        self._check(self._L.rto_debug_components_passes(self._h, C.byref(n)))
        return n.value

    def edit_components(self, set: int, connectivity: int, select: int, arg: int = 0) -> int:
        """rto_edit_components: label afresh, flip every voxel of the selected components (SELECT_*), rebuild as edit_voxels
        does; the number of voxels flipped."""
        changed = C.c_int64()
        self._check(self._L.rto_edit_components(self._h, int(set), int(connectivity), int(select), int(arg), C.byref(changed)))
        return changed.value

    # -- part segmentation ---------------------------------------------------------
    def segment_parts(self, set: int = SET_SOLID, connectivity: int = CONN_FACE, ratio: int = 800):
        """rto_segment_parts: the watershed of the squared distance field of SET_SOLID or SET_EMPTY under CONN_FACE or CONN_FULL,
        basins merged where 1,000,000 s >= ratio^2 min(P, P') (0: the components, PARTS_RATIO_MAX: the basins); the summary as a
        PARTS_SUMMARY_DTYPE scalar.  Labels and both tables stay resident until the grid changes."""
        summary = np.zeros((), PARTS_SUMMARY_DTYPE)
        self._check(self._L.rto_segment_parts(self._h, int(set), int(connectivity), int(ratio), summary.ctypes.data))
        return summary

    def _parts_table(self, symbol: str, dtype) -> np.ndarray:
        n = C.c_int64()
        self._check(getattr(self._L, symbol)(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype)
        if n.value:
            self._check(getattr(self._L, symbol)(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def part_labels(self) -> np.ndarray:
        """The resident part labels as int32 (dimZ, dimY, dimX): the part's number, -1 outside the set."""
        return self._resident_field("rto_parts_device", "rto_download_part_labels", outputs=5)

    def parts(self) -> np.ndarray:
        """The resident part table as a PART_DTYPE array, in ascending order of the parts' smallest voxel."""
        return self._parts_table("rto_download_parts", PART_DTYPE)

    def necks(self) -> np.ndarray:
        """The resident neck table as a NECK_DTYPE array, sorted by (part_lo, part_hi)."""
        return self._parts_table("rto_download_necks", NECK_DTYPE)

    def parts_device(self):
        """(device pointer of the int32 label volume, of the 64-byte part records, parts, of the 32-byte neck records, necks)."""
        l, p, q = C.c_void_p(), C.c_void_p(), C.c_void_p()
        n, m = C.c_int64(), C.c_int64()
        self._check(self._L.rto_parts_device(self._h, C.byref(l), C.byref(p), C.byref(n), C.byref(q), C.byref(m)))
        return l.value or 0, p.value or 0, n.value, q.value or 0, m.value

    def edit_parts(self, set: int = SET_SOLID, connectivity: int = CONN_FACE, ratio: int = 800) -> int:
        """rto_edit_parts: segment afresh, flip every voxel of the set that has a neighbour of a larger part number, rebuild as
        edit_voxels does; the number of voxels flipped."""
        changed = C.c_int64()
        self._check(self._L.rto_edit_parts(self._h, int(set), int(connectivity), int(ratio), C.byref(changed)))
        return changed.value

    def last_parts_ms(self):
        """ms of the last segment_parts: (transform, ascent + flatten, ranking + basin table, edges, host merge + relabel); -1: not run."""
        return self._last_ms("rto_last_parts_ms", 5)

    def debug_parts(self):
        """(basins, basin edges downloaded, flatten rounds, edge-table slots) of the last segment_parts."""
        b, e, cap, r = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
        self._check(self._L.rto_debug_parts(self._h, C.byref(b), C.byref(e), C.byref(r), C.byref(cap)))
        return b.value, e.value, r.value, cap.value

    def debug_parts_capacity(self, first_capacity: int):
        """The first capacity of the basin-edge table from now on (0: sized from the basin count); changes no value."""
        self._check(self._L.rto_debug_parts_capacity(self._h, int(first_capacity)))

    # -- component measures -------------------------------------------------------
    def measure_components(self):
        """rto_measure_components: measure every component of the resident labelling (the set and connectivity of the last
        label_components): (the table as a MEASURE_DTYPE array in the component table's order, the total row as a MEASURE_DTYPE
        scalar).  The table stays resident beside the labels and goes when they go."""
        total = np.zeros((), MEASURE_DTYPE)
        self._check(self._L.rto_measure_components(self._h, total.ctypes.data))
        return self.component_measures(), total

    def component_measures(self) -> np.ndarray:
        """The resident measures (rto_download_measures)."""
        n = C.c_int64()
        self._check(self._L.rto_download_measures(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, MEASURE_DTYPE)
        if n.value:
            self._check(self._L.rto_download_measures(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def component_measures_device(self):
        """(device pointer of the 160-byte measure records, count)."""
        p, n = C.c_void_p(), C.c_int64()
        self._check(self._L.rto_measures_device(self._h, C.byref(p), C.byref(n)))
        return p.value or 0, n.value

    def last_measure_ms(self):
        """Device ms of the last measure_components: (the measuring kernels, the total); -1: not run."""
        return self._last_ms("rto_last_measure_ms", 2)

    def topology(self, set: int = SET_SOLID, connectivity: int = CONN_FACE):
        """(pieces, tunnels, cavities) of the set under `connectivity`.  Three steps: label the complement under the dual
        connectivity (6 <-> 26) and count its components that touch no grid face, the cavities; label the set and count the
        pieces; measure, and take tunnels = pieces + cavities - total euler.  The SET's labels and measures are what is resident
        afterwards (the complement's labelling is replaced by step two)."""
        other = SET_EMPTY if int(set) == SET_SOLID else SET_SOLID
        dual = CONN_FULL if int(connectivity) == CONN_FACE else CONN_FACE
        if int(connectivity) not in (CONN_FACE, CONN_FULL):
            dual = int(connectivity)                                          # refused below, by the library, with its message
        outside = self.label_components(other, dual)
        cavities = int((outside["touches"] == 0).sum())
        pieces = len(self.label_components(set, connectivity))
        _, total = self.measure_components()
        return pieces, pieces + cavities - int(total["euler"]), cavities

    # -- distance fields and morphology ------------------------------------------
    def distance_field(self, set: int = SET_SOLID, max_dist: float = float("inf")):
        """rto_distance_field: (the int32 (dimZ, dimY, dimX) volume of squared distances, in voxel-index units, to the nearest voxel
        of SET_SOLID or SET_EMPTY, DIST_NONE beyond max_dist (world units); the summary as a DIST_SUMMARY_DTYPE scalar).  The field
        stays resident until the grid changes."""
        summary = np.zeros((), DIST_SUMMARY_DTYPE)
        self._check(self._L.rto_distance_field(self._h, int(set), float(max_dist), summary.ctypes.data))
        return self.distance(), summary

    def distance(self) -> np.ndarray:
        """The resident field (rto_download_distance)."""
        return self._resident_field("rto_distance_device", "rto_download_distance")

    def distance_device(self) -> int:
        """The device pointer of the resident int32 field."""
        return self._device_pointer("rto_distance_device")

    def last_distance_ms(self):
        """Device ms of the last distance_field: (x pass, y pass, z pass, summary); -1: not run."""
        return self._last_ms("rto_last_distance_ms", 4)

    def edit_morphology(self, op: int, radius: float) -> int:
        """rto_edit_morphology: MORPH_DILATE / MORPH_ERODE / MORPH_OPEN / MORPH_CLOSE by `radius` (world units), rebuilt as
        edit_voxels does; the number of voxels whose value differs from the one before the call."""
        changed = C.c_int64()
        self._check(self._L.rto_edit_morphology(self._h, int(op), float(radius), C.byref(changed)))
        return changed.value

    def last_morphology_ms(self):
        """Device ms of the last edit_morphology: (transforms and flips, octree rebuild, triangle rebuild); -1: not run."""
        return self._last_ms("rto_last_morphology_ms", 3)

    # -- geodesic fields, paths and flood edits ---------------------------------------
    def _voxel_indices(self, voxels) -> np.ndarray:
        """Linear indices as contiguous int64: `voxels` is a sequence of them, or an (n, 3) array of (i, j, k) in the resident
        grid's dims."""
        a = np.asarray(voxels)
        if a.ndim == 2 and a.shape[1] == 3:
            dims = (C.c_int * 3)()
            self._check(self._L.rto_download_voxels(self._h, None, 0, dims))
            a = a.astype(np.int64)
            a = a[:, 0] + dims[0] * (a[:, 1] + dims[1] * a[:, 2])
        return np.ascontiguousarray(a.reshape(-1), np.int64)

    def geodesic_field(self, seeds, medium: int = SET_EMPTY, connectivity: int = CONN_FACE, limit=None):
        """rto_geodesic_field: (the int32 (dimZ, dimY, dimX) volume of shortest-path lengths inside `medium` from `seeds` (linear
        indices, or an (n, 3) array of (i, j, k)): steps under CONN_FACE, 3 / 4 / 5 per move under CONN_FULL; DIST_NONE outside the
        medium, out of reach or above `limit` (None: no limit); the summary as a GEO_SUMMARY_DTYPE scalar).  The field stays
        resident until the grid changes."""
        s = self._voxel_indices(seeds)
        summary = np.zeros((), GEO_SUMMARY_DTYPE)
        self._check(self._L.rto_geodesic_field(self._h, int(medium), int(connectivity), s.ctypes.data, s.size,
                                               GEO_NO_LIMIT if limit is None else int(limit), summary.ctypes.data))
        return self.geodesic(), summary

    def geodesic(self) -> np.ndarray:
        """The resident geodesic field (rto_download_geodesic)."""
        return self._resident_field("rto_geodesic_device", "rto_download_geodesic")

    def geodesic_device(self) -> int:
        """The device pointer of the resident int32 geodesic field."""
        return self._device_pointer("rto_geodesic_device")

    def geodesic_paths(self, targets, max_len: int):
        """rto_geodesic_paths on the resident field: (rows, lengths) -- rows (n, max_len) int64, each the first voxels of the path
        from its target down to a seed and -1 behind them; lengths (n,) int64, the full length of each path, -1 for a target the
        field does not reach."""
        t = self._voxel_indices(targets)
        rows = np.empty((t.size, int(max_len)), np.int64) if int(max_len) >= 0 else np.empty((t.size, 0), np.int64)
        lengths = np.empty(t.size, np.int64)
        self._check(self._L.rto_geodesic_paths(self._h, t.ctypes.data, t.size, int(max_len), rows.ctypes.data if rows.size else None,
                                               lengths.ctypes.data))
        return rows, lengths

    def edit_geodesic(self, seeds, medium: int = SET_EMPTY, connectivity: int = CONN_FACE, limit=None) -> int:
        """rto_edit_geodesic: flips every voxel of `medium` within `limit` of the seeds along paths inside the medium, rebuilt as
        edit_voxels does; the number of voxels flipped."""
        s = self._voxel_indices(seeds)
        changed = C.c_int64()
        self._check(self._L.rto_edit_geodesic(self._h, int(medium), int(connectivity), s.ctypes.data, s.size,
                                              GEO_NO_LIMIT if limit is None else int(limit), C.byref(changed)))
        return changed.value

    def last_geodesic_ms(self):
        """Device ms of the last geodesic_field: (init, relaxation, summary); -1: not run."""
        return self._last_ms("rto_last_geodesic_ms", 3)

    def last_geodesic_edit_ms(self):
        """Device ms of the last edit_geodesic: (field and flip, octree rebuild, triangle rebuild); -1: not run."""
        return self._last_ms("rto_last_geodesic_edit_ms", 3)

    def geodesic_passes(self, tiles: bool = False):
        """Relaxation launches of the last geodesic_field, the closing one that found no tile included; with tiles=True the pair
        (launches, tiles run summed over them)."""
        p, t = C.c_int64(), C.c_int64()
        self._check(self._L.rto_debug_geodesic_passes(self._h, C.byref(p), C.byref(t)))
        return (p.value, t.value) if tiles else p.value

    def debug_set_geodesic_look(self, passes_per_look: int) -> None:
        """How many relaxation launches go out between two looks at the device (1 .. 64): changes no value."""
        self._check(self._L.rto_debug_set_geodesic_look(self._h, int(passes_per_look)))

    # -- skeletons: topology-preserving thinning ------------------------------------------
    def skeleton_field(self, set: int = SET_SOLID, connectivity: int = CONN_FULL, mode: int = SKEL_TOPOLOGY, anchors=(), max_passes=None):
        """rto_skeleton_field: (the int32 (dimZ, dimY, dimX) volume k of the thinning of `set`: -1 outside the set, 0 for the voxels
        that stay (the skeleton), p >= 1 for the pass that removed the voxel; the summary as a SKEL_SUMMARY_DTYPE scalar).
        `anchors` (linear indices, or an (n, 3) array of (i, j, k)) are never removed; max_passes None: no limit.  The field stays
        resident until the grid changes."""
        a = self._voxel_indices(anchors) if len(anchors) else np.empty(0, np.int64)
        summary = np.zeros((), SKEL_SUMMARY_DTYPE)
        self._check(self._L.rto_skeleton_field(self._h, int(set), int(connectivity), int(mode), a.ctypes.data if a.size else None, a.size,
                                               SKEL_NO_LIMIT if max_passes is None else int(max_passes), summary.ctypes.data))
        return self.skeleton(), summary

    def skeleton(self) -> np.ndarray:
        """The resident skeleton field (rto_download_skeleton)."""
        return self._resident_field("rto_skeleton_device", "rto_download_skeleton")

    def skeleton_device(self) -> int:
        """The device pointer of the resident int32 skeleton field."""
        return self._device_pointer("rto_skeleton_device")

    def edit_skeleton(self, set: int = SET_SOLID, connectivity: int = CONN_FULL, mode: int = SKEL_TOPOLOGY, anchors=(), max_passes=None) -> int:
        """rto_edit_skeleton: replaces `set` by its skeleton (every voxel the thinning removes is flipped), rebuilt as edit_voxels
        does; the number of voxels flipped."""
        a = self._voxel_indices(anchors) if len(anchors) else np.empty(0, np.int64)
        changed = C.c_int64()
        self._check(self._L.rto_edit_skeleton(self._h, int(set), int(connectivity), int(mode), a.ctypes.data if a.size else None, a.size,
                                              SKEL_NO_LIMIT if max_passes is None else int(max_passes), C.byref(changed)))
        return changed.value

    def last_skeleton_ms(self):
        """Device ms of the last skeleton_field: (init, thinning, summary); -1: not run."""
        return self._last_ms("rto_last_skeleton_ms", 3)

    def last_skeleton_edit_ms(self):
        """Device ms of the last edit_skeleton: (field and flip, octree rebuild, triangle rebuild); -1: not run."""
        return self._last_ms("rto_last_skeleton_edit_ms", 3)

    def skeleton_passes(self):
        """(kernel launches, tiles run summed over the sub-steps) of the last skeleton_field's thinning."""
        p, t = C.c_int64(), C.c_int64()
        self._check(self._L.rto_debug_skeleton_passes(self._h, C.byref(p), C.byref(t)))
        return p.value, t.value

    def debug_set_skeleton_look(self, passes_per_look: int) -> None:
        """How many passes go out between two looks at the device (1 .. 64): changes no value."""
        self._check(self._L.rto_debug_set_skeleton_look(self._h, int(passes_per_look)))

    # -- exposure fields: sun hours and sky view per voxel -------------------------------
    def exposure_field(self, dirs, weights=None, mode: int = EXPO_SKIN, reach=None):
        """rto_exposure_field: (the int32 (dimZ, dimY, dimX) volume e: for every evaluated EMPTY voxel (EXPO_ALL: all of them;
        EXPO_SKIN: those with a SOLID face neighbour) the sum of the weights of the directions along which no SOLID voxel is crossed
        within `reach` voxels, -1 for every other voxel; the summary as an EXPO_SUMMARY_DTYPE scalar).  `dirs` is (n, 3) integers
        (quantize_directions makes them from floats), `weights` n non-negative integers or None for ones; reach None: no limit.
        The field stays resident until the grid changes."""
        d = np.ascontiguousarray(np.asarray(dirs, np.int64).reshape(-1, 3))
        if d.size and (np.abs(d) > 0x7fffffff).any():
            raise ValueError("a direction's component does not fit int32")
        d = np.ascontiguousarray(d, np.int32)
        w = None
        if weights is not None:
            w = np.asarray(weights, np.int64).reshape(-1)
            if w.size != len(d):
                raise ValueError("one weight per direction")
            if w.size and (np.abs(w) > 0x7fffffff).any():
                raise ValueError("a weight does not fit int32")
            w = np.ascontiguousarray(w, np.int32)
        summary = np.zeros((), EXPO_SUMMARY_DTYPE)
        self._check(self._L.rto_exposure_field(self._h, d.ctypes.data if d.size else None, None if w is None else w.ctypes.data, len(d),
                                               int(mode), EXPO_NO_LIMIT if reach is None else int(reach), summary.ctypes.data))
        return self.exposure(), summary

    def exposure(self) -> np.ndarray:
        """The resident exposure field (rto_download_exposure)."""
        return self._resident_field("rto_exposure_device", "rto_download_exposure")

    def exposure_device(self) -> int:
        """The device pointer of the resident int32 exposure field."""
        return self._device_pointer("rto_exposure_device")

    def last_exposure_ms(self):
        """Device ms of the last exposure_field: (prepare, march, summary); -1: not run."""
        return self._last_ms("rto_last_exposure_ms", 3)

    # -- dose fields: point sources seen through the grid ---------------------------------
    def dose_field(self, sources, transmit=None, falloff: int = DOSE_FALLOFF_NONE, mode: int = DOSE_ALL, reach=None):
        """rto_dose_field: (the int32 (dimZ, dimY, dimX) volume e: for every evaluated EMPTY voxel (DOSE_ALL: all of them; DOSE_SKIN:
        those with a SOLID face neighbour) the sum over the sources within `reach` voxels of floor((w T[k] >> 16) / D), k the SOLID
        voxels the segment to the source crosses and D the squared distance under DOSE_FALLOFF_INVERSE_SQUARE, -1 for every other
        voxel; the summary as a DOSE_SUMMARY_DTYPE scalar).  `sources` is (n, 4) integers: the voxel i, j, k of the grid and the
        weight; `transmit` the Q16 table T (65536 is 1.0) or None for plain line of sight; reach None: DOSE_MAX_REACH.  The field
        and its coverage table (dose_coverage) stay resident until the grid changes.  There is no FIELD_* code for it: the views,
        projections, composites and isosurfaces take dose_device() with FIELD_CALLER."""
        s = np.ascontiguousarray(np.asarray(sources, np.int64).reshape(-1, 4))
        if s.size and (np.abs(s) > 0x7fffffff).any():
            raise ValueError("a source's coordinate or weight does not fit int32")
        s = np.ascontiguousarray(s, np.int32)
        t = None
        if transmit is not None:
            t = np.asarray(transmit, np.int64).reshape(-1)
            if t.size and ((t < 0) | (t > 0xffffffff)).any():
                raise ValueError("a table entry does not fit uint32")
            t = np.ascontiguousarray(t, np.uint32)
        summary = np.zeros((), DOSE_SUMMARY_DTYPE)
        self._check(self._L.rto_dose_field(self._h, s.ctypes.data if s.size else None, len(s), None if t is None else t.ctypes.data,
                                           0 if t is None else t.size, int(falloff), int(mode), DOSE_NO_LIMIT if reach is None else int(reach),
                                           summary.ctypes.data))
        return self.dose(), summary

    def dose(self) -> np.ndarray:
        """The resident dose field (rto_download_dose)."""
        return self._resident_field("rto_dose_device", "rto_download_dose")

    def dose_device(self) -> int:
        """The device pointer of the resident int32 dose field: the volume for FIELD_CALLER."""
        return self._device_pointer("rto_dose_device")

    def dose_coverage(self) -> np.ndarray:
        """covered[s] of the resident dose field's sources (rto_download_dose_coverage): int64, one per source."""
        out = np.full(DOSE_MAX_SOURCES, -1, np.int64)                   # a count is never negative: the entries written are the table
        self._check(self._L.rto_download_dose_coverage(self._h, out.ctypes.data, out.size))
        return out[:int((out >= 0).sum())].copy()

    def last_dose_ms(self):
        """Device ms of the last dose_field: (prepare, march, summary); -1: not run."""
        return self._last_ms("rto_last_dose_ms", 3)

    # -- local thickness fields ----------------------------------------------------------
    def thickness_field(self, medium: int = SET_SOLID, max_radius: float | None = None):
        """rto_thickness_field: (the int32 (dimZ, dimY, dimX) volume of the squared radius, in voxel-index units, of the largest ball
        inside `medium` (SET_SOLID: the material, SET_EMPTY: the free space) that contains each of its voxels, for balls up to
        max_radius (world units, at least 1 and at most 8 voxels), 0 outside the medium; the summary as a THICK_SUMMARY_DTYPE
        scalar).  The field stays resident until the grid changes."""
        if max_radius is None:
            raise ValueError("thickness_field: max_radius (world units, 1 to 8 voxels) has no default")
        summary = np.zeros((), THICK_SUMMARY_DTYPE)
        self._check(self._L.rto_thickness_field(self._h, int(medium), float(max_radius), summary.ctypes.data))
        return self.thickness(), summary

    def thickness(self) -> np.ndarray:
        """The resident thickness field (rto_download_thickness)."""
        return self._resident_field("rto_thickness_device", "rto_download_thickness")

    def thickness_device(self) -> int:
        """The device pointer of the resident int32 thickness field."""
        return self._device_pointer("rto_thickness_device")

    def thickness_histogram(self) -> np.ndarray:
        """rto_thickness_histogram: int64 bins[t], t = 0 .. c: the medium voxels of the resident field with t2 = t."""
        bins = C.c_int64()
        self._check(self._L.rto_thickness_histogram(self._h, None, 0, C.byref(bins)))
        out = np.zeros(bins.value, np.int64)
        self._check(self._L.rto_thickness_histogram(self._h, out.ctypes.data, out.size, None))
        return out

    def last_thickness_ms(self):
        """Device ms of the last thickness_field: (transform, gather, summary); -1: not run."""
        return self._last_ms("rto_last_thickness_ms", 3)

    def thickness_table(self):
        """rto_debug_thickness_table: (the c the gather's kept offset table was made for, 0: none yet; tables built so far)."""
        c, built = C.c_int(), C.c_int64()
        self._check(self._L.rto_debug_thickness_table(self._h, C.byref(c), C.byref(built)))
        return c.value, built.value

    # -- region queries --------------------------------------------------------
    def query_points(self, points) -> np.ndarray:
        """Which leaf holds each point (rto_query_points_host): points (n, 3) world positions.  A POINT_HIT_DTYPE array; node -1
        for a point outside every leaf or an invalid one (NaN, infinite, beyond 2^21 voxels)."""
        p = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
        hits = np.zeros(len(p), POINT_HIT_DTYPE)
        self._check(self._L.rto_query_points_host(self._h, p.ctypes.data if len(p) else None, len(p), hits.ctypes.data if len(p) else None))
        return hits

    def query_points_device(self, d_points: int, n: int, d_hits: int, stream: int = 0):
        """Asynchronous: n points of 3 floats at d_points -> n rto_point_hit records at d_hits (device pointers, 16-byte aligned)."""
        self._check(self._L.rto_query_points_device(self._h, C.c_void_p(d_points) if d_points else None, int(n),
                                                    C.c_void_p(d_hits) if d_hits else None, C.c_void_p(stream) if stream else None))

    def query_regions(self, brushes) -> np.ndarray:
        """How much solid each brush covers (rto_query_regions_host): BRUSH_DTYPE records (make_brushes; the op is ignored).  A
        REGION_DTYPE array; filled = covered = -1 for an invalid brush.  A CARVE of the brush would change `filled` voxels, a FILL
        `covered - filled`."""
        b = np.ascontiguousarray(np.asarray(brushes, BRUSH_DTYPE).reshape(-1))
        out = np.zeros(len(b), REGION_DTYPE)
        self._check(self._L.rto_query_regions_host(self._h, b.ctypes.data if len(b) else None, len(b), out.ctypes.data if len(b) else None))
        return out

    def query_regions_device(self, d_brushes: int, n: int, d_regions: int, stream: int = 0):
        """Asynchronous: n rto_brush records at d_brushes -> n rto_region records at d_regions (device pointers, 16-byte aligned)."""
        self._check(self._L.rto_query_regions_device(self._h, C.c_void_p(d_brushes) if d_brushes else None, int(n),
                                                     C.c_void_p(d_regions) if d_regions else None, C.c_void_p(stream) if stream else None))

    def query_nearest_records(self, points, max_dist=np.inf) -> np.ndarray:
        """The NEAREST_DTYPE records of rto_query_nearest_host: points (n, 3), max_dist one value or one per point (+inf: no limit)."""
        p = make_near_points(points, max_dist)
        out = np.zeros(len(p), NEAREST_DTYPE)
        self._check(self._L.rto_query_nearest_host(self._h, p.ctypes.data if len(p) else None, len(p), out.ctypes.data if len(p) else None))
        return out

    def query_nearest(self, points, max_dist=np.inf):
        """The nearest solid to each point: (records, distance).  records: NEAREST_DTYPE (dist2 -1: none within max_dist, or an
        invalid record); distance: float64 world units, sqrt(dist2) / 64 * voxelSize computed on the host in double, inf where
        dist2 is -1."""
        rec = self.query_nearest_records(points, max_dist)
        vs = float(self.scene_bounds().voxel_size) if len(rec) else 0.0
        d2 = rec["dist2"].astype(np.float64)
        dist = np.where(rec["dist2"] >= 0, np.sqrt(np.maximum(d2, 0.0)) / 64.0 * vs, np.inf)
        return rec, dist

    def query_nearest_device(self, d_points: int, n: int, d_out: int, stream: int = 0):
        """Asynchronous: n rto_near_point records at d_points -> n rto_nearest records at d_out (device pointers, 16-byte aligned)."""
        self._check(self._L.rto_query_nearest_device(self._h, C.c_void_p(d_points) if d_points else None, int(n),
                                                     C.c_void_p(d_out) if d_out else None, C.c_void_p(stream) if stream else None))

    # -- mesh voxelization -----------------------------------------------------
    def voxelize_mesh(self, xyz, tris, voxel_size, grid=None, recenter=0, triangles=False) -> VoxelizeResult:
        """rto_voxelize_mesh: xyz (n, 3) rows (float64), tris (m, 3) row indices; grid None = AUTO (the reference's grid from
        voxel_size), else FIXED (dims (x, y, z), grid_min, voxel_size).  recenter: 0, 1 or 2 passes; triangles: also build the
        leaf triangles.  The octree is then resident, as build_octree of the voxelized grid leaves it."""
        v = np.ascontiguousarray(np.asarray(xyz, np.float64).reshape(-1, 3))
        t = np.ascontiguousarray(np.asarray(tris, np.int32).reshape(-1, 3))
        p = VoxelizeParams()
        p.voxel_size = _f(voxel_size)
        p.recenter_passes = int(recenter)
        p.triangles = 1 if triangles else 0
        if grid is None:
            p.mode = VOXELIZE_AUTO
        else:
            dims, gmin, vs = grid
            p.mode = VOXELIZE_FIXED
            p.voxel_size = _f(vs)
            for a in range(3):
                p.dims[a] = int(dims[a])
                p.grid_min[a] = _f(gmin[a])
        r = VoxelizeResult()
        self._check(self._L.rto_voxelize_mesh(self._h, v.ctypes.data if len(v) else None, len(v), t.ctypes.data if len(t) else None,
                                              len(t), C.byref(p), C.byref(r)))
        return r

    def last_voxelize_ms(self):
        """Device ms of the last voxelization: (face setup + scan, fill, recentring reduction, octree build); -1: not run."""
        return self._last_ms("rto_last_voxelize_ms", 4)

    # -- mesh extraction ---------------------------------------------------
    @staticmethod
    def frustum_planes(view, fov_deg, aspect) -> np.ndarray:
        """The planes rto_update_frustum derives for this view (rto_frustum_planes, pure host): 24 float32."""
        return frustum_planes(view, fov_deg, aspect)

    def extract_mesh_count(self, kind: int, planes=None, margin: float = 50.0) -> int:
        """rto_extract_mesh alone: the mesh stays on the device (mesh_device / download_mesh); returns its triangle count."""
        cull = None
        if planes is not None:
            cull = MeshCull()
            pl = np.ascontiguousarray(np.asarray(planes, dtype=np.float32).reshape(24))
            C.memmove(cull.planes, pl.ctypes.data, 96)
            cull.margin = float(np.float32(margin)) if np.isfinite(margin) else float(margin)
        n = C.c_int64(-1)
        self._check(self._L.rto_extract_mesh(self._h, int(kind), C.byref(cull) if cull is not None else None, C.byref(n)))
        return n.value

    def download_mesh(self):
        """The last extracted mesh: (tris float32 (n, 12): v0, v1, v2, normal; tri_node int32 (n,): the owning leaf)."""
        n = C.c_int64()
        self._check(self._L.rto_download_mesh(self._h, None, 0, None, C.byref(n)))
        tris = np.zeros((n.value, 12), np.float32)
        node = np.zeros(n.value, np.int32)
        if n.value:
            self._check(self._L.rto_download_mesh(self._h, tris.ctypes.data, n.value, node.ctypes.data, C.byref(n)))
        return tris, node

    def extract_mesh(self, kind: int, planes=None, margin: float = 50.0):
        """The triangle list of what the planes see: kind MESH_MC (the resident leaf triangles) or MESH_CUBES
        (exposed faces of the solid leaves), in the reference's depth-first order; planes (24 floats, frustum_planes' layout) or
        None for no culling, margin = renderOctree's extraMargin.  Returns (tris (n, 12), tri_node (n,))."""
        self.extract_mesh_count(kind, planes, margin)
        return self.download_mesh()

    def mesh_device(self):
        """(device pointer of the 48-byte records, device pointer of tri_node, count) of the last extracted mesh."""
        t, nd, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        self._check(self._L.rto_mesh_device(self._h, C.byref(t), C.byref(nd), C.byref(n)))
        return t.value or 0, nd.value or 0, n.value

    def last_mesh_ms(self):
        """Device ms of the last extraction: (count + cull, ranking passes, emit); -1: not run."""
        return self._last_ms("rto_last_mesh_ms", 3)

    # -- field isosurfaces -------------------------------------------------
    def extract_isosurface_count(self, params: IsoParams, volume=None) -> IsoSummary:
        """rto_extract_isosurface_*: the list stays on the device (isosurface_device / download_isosurface).  volume (source
        FIELD_CALLER only): a host array of dimZ x dimY x dimX int32, or a device pointer (an int, or a device tensor)."""
        summary = IsoSummary()
        if volume is None or isinstance(volume, int):
            rc = self._L.rto_extract_isosurface_device(self._h, C.byref(params) if params is not None else None, volume or None, C.byref(summary))
        elif hasattr(volume, "data_ptr") and getattr(volume, "is_cuda", False):
            rc = self._L.rto_extract_isosurface_device(self._h, C.byref(params) if params is not None else None, volume.data_ptr(), C.byref(summary))
        else:
            vol = np.ascontiguousarray(np.asarray(volume, dtype=np.int32))
            rc = self._L.rto_extract_isosurface_host(self._h, C.byref(params) if params is not None else None, vol.ctypes.data, C.byref(summary))
        self._check(rc)
        return summary

    def download_isosurface(self):
        """The last isosurface: (tris float32 (n, 12): v0, v1, v2, normal; tri_cell int32 (n,): the owning cell)."""
        n = C.c_int64()
        self._check(self._L.rto_download_isosurface(self._h, None, 0, None, C.byref(n)))
        tris = np.zeros((n.value, 12), np.float32)
        cell = np.zeros(n.value, np.int32)
        if n.value:
            self._check(self._L.rto_download_isosurface(self._h, tris.ctypes.data, n.value, cell.ctypes.data, C.byref(n)))
        return tris, cell

    def extract_isosurface(self, params: IsoParams, volume=None):
        """Marching cubes of a voxel field at params.level, in the reference's cell order.  Returns
        (tris (n, 12), tri_cell (n,), summary)."""
        summary = self.extract_isosurface_count(params, volume)
        tris, cell = self.download_isosurface()
        return tris, cell, summary

    def isosurface_device(self):
        """(device pointer of the 48-byte records, device pointer of tri_cell, count) of the last isosurface."""
        t, cl, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        self._check(self._L.rto_isosurface_device(self._h, C.byref(t), C.byref(cl), C.byref(n)))
        return t.value or 0, cl.value or 0, n.value

    def last_isosurface_ms(self):
        """Device ms of the last isosurface: (count, rank, emit); -1: not run."""
        return self._last_ms("rto_last_isosurface_ms", 3)

    # -- dual contouring ----------------------------------------------------
    def extract_dual_contour_count(self, params: DcParams) -> DcSummary:
        """rto_extract_dual_contour: the list stays on the device (dual_contour_device / download_dual_contour)."""
        summary = DcSummary()
        self._check(self._L.rto_extract_dual_contour(self._h, C.byref(params) if params is not None else None, C.byref(summary)))
        return summary

    def download_dual_contour(self):
        """The last dual-contour list: (tris float32 (n, 12): v0, v1, v2, normal; tri_cell int32 (n,): the owning cell)."""
        n = C.c_int64()
        self._check(self._L.rto_download_dual_contour(self._h, None, 0, None, C.byref(n)))
        tris = np.zeros((n.value, 12), np.float32)
        cell = np.zeros(n.value, np.int32)
        if n.value:
            self._check(self._L.rto_download_dual_contour(self._h, tris.ctypes.data, n.value, cell.ctypes.data, C.byref(n)))
        return tris, cell

    def extract_dual_contour(self, params: DcParams):
        """Dual contouring of the resident grid, in the reference's buildTrianglesCPU order.  Returns
        (tris (n, 12), tri_cell (n,), summary)."""
        summary = self.extract_dual_contour_count(params)
        tris, cell = self.download_dual_contour()
        return tris, cell, summary

    def dual_contour_device(self):
        """(device pointer of the 48-byte records, device pointer of tri_cell, count) of the last dual-contour list."""
        t, cl, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        self._check(self._L.rto_dual_contour_device(self._h, C.byref(t), C.byref(cl), C.byref(n)))
        return t.value or 0, cl.value or 0, n.value

    def last_dual_contour_ms(self):
        """Device ms of the last dual-contour extraction: (count, rank, emit); -1: not run."""
        return self._last_ms("rto_last_dual_contour_ms", 3)

    def query_dual_vertices(self, voxels, out=None):
        """rto_query_dual_vertices_*: the dual-contouring vertex of each voxel (linear indices, x fastest).  voxels: a host array
        of int64 -> a DUAL_VERTEX_DTYPE array (p, points; points = -1 outside the grid); or a device int64 tensor with `out` a
        device tensor of 16 bytes per voxel, which is filled and returned."""
        if hasattr(voxels, "data_ptr") and getattr(voxels, "is_cuda", False):
            n = int(voxels.numel())
            self._check(self._L.rto_query_dual_vertices_device(self._h, voxels.data_ptr(), n, out.data_ptr() if out is not None else None))
            return out
        v = np.ascontiguousarray(np.asarray(voxels, dtype=np.int64).reshape(-1))
        res = np.zeros(len(v), DUAL_VERTEX_DTYPE)
        self._check(self._L.rto_query_dual_vertices_host(self._h, v.ctypes.data, len(v), res.ctypes.data))
        return res

    def scene_bounds(self) -> SceneBounds:
        b = SceneBounds()
        self._check(self._L.rto_scene_bounds_get(self._h, C.byref(b)))
        return b

    @property
    def stream(self) -> int:
        """The context's own hipStream_t as an integer handle."""
        return self._L.rto_stream(self._h) or 0

    def synchronize(self):
        self._check(self._L.rto_synchronize(self._h))


def comm_unique_id() -> bytes:
    """rank 0: the 128 bytes every other rank needs for Comm(ctx, world, rank, id)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = load().rto_comm_unique_id(buf)
    if rc != RTO_OK:
        raise RtoError(rc, load().rto_last_error(None).decode())
    return buf.raw


class Comm:
    """rto_comm: one rank of the screen-split renderer (one process per GPU).  submit() renders this rank's bands of a batch
    of frames, ONE grouped RCCL send/recv lands them on rank 0, which assembles them into `d_frames`; flush() waits."""

    def __init__(self, ctx: Context, world: int, rank: int, unique_id: bytes, band_rows: int = 16):
        self._L = load()
        self.ctx, self.world, self.rank = ctx, world, rank
        h = C.c_void_p()
        idbuf = C.create_string_buffer(bytes(unique_id), COMM_ID_BYTES)
        rc = self._L.rto_comm_create(ctx._h, world, rank, idbuf, band_rows, C.byref(h))
        if rc != RTO_OK:
            raise RtoError(rc, self._L.rto_last_error(ctx._h).decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.rto_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != RTO_OK:
            raise RtoError(rc, self._L.rto_comm_last_error(self._h).decode())

    def submit(self, frames_arr, d_frames: int = 0, frame_stride_bytes: int = 0, mode: int = RESIDENT_OCTREE):
        """frames_arr: Context.frame_array([...]); d_frames (rank 0): device pointer of len(frames_arr) RGBA32F frames."""
        self._check(self._L.rto_comm_submit(self._h, frames_arr, len(frames_arr), mode, C.c_void_p(d_frames) if d_frames else None, frame_stride_bytes))

    def flush(self, timeout_ms: int = 0):
        """Waits for every submitted batch.  timeout_ms > 0: at most that long -- on expiry (a peer that never sent) the
        communicator is aborted and dead, RtoError(RTO_E_TIMEOUT)."""
        self._check(self._L.rto_comm_flush_timeout(self._h, int(timeout_ms)))

    def is_dead(self) -> bool:
        return bool(self._L.rto_comm_is_dead(self._h))

    def ranks_seen(self) -> int:
        """ncclCommCount: the ranks RCCL says take part in this communicator."""
        n = C.c_int(0)
        self._check(self._L.rto_comm_ranks_seen(self._h, C.byref(n)))
        return int(n.value)

    def debug_abort(self):
        """Test hook: what a flush timeout does (ncclCommAbort, the communicator is dead)."""
        self._check(self._L.rto_comm_debug_abort(self._h))

    def debug_last_payload(self):
        """(floats shipped for the last batch, floats whole rows would have been) for this rank."""
        a, b = C.c_int64(), C.c_int64()
        self._check(self._L.rto_comm_debug_last_payload(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def debug_set_rehearsal_clear(self, enabled: bool):
        self._check(self._L.rto_comm_debug_set_rehearsal_clear(self._h, 1 if enabled else 0))

    def debug_set_timing(self, enabled: bool):
        self._check(self._L.rto_comm_debug_set_timing(self._h, 1 if enabled else 0))

    def debug_last_timing(self):
        """(render ms, gather (+ assembly on rank 0) ms) of the batch submitted last; call after flush()."""
        ms = (C.c_float * 2)()
        self._check(self._L.rto_comm_debug_last_timing(self._h, ms))
        return float(ms[0]), float(ms[1])

    def debug_rehearse(self, as_world: int, as_rank: int = 0):
        """One-rank communicator only: split frames as rank `as_rank` of `as_world` GPUs (0 switches it off)."""
        self._check(self._L.rto_comm_debug_rehearse(self._h, as_world, as_rank))

    @property
    def stream(self) -> int:
        return self._L.rto_comm_stream(self._h) or 0


class CommGroup:
    """rto_comm_create_all: one process driving several GPUs (one Context each, all on different devices).  render_resident()
    sends one frame through every rank into rank 0's resident framebuffer; submit()/flush() are the batched, pipelined form."""

    def __init__(self, contexts, band_rows: int = 16):
        self._L = load()
        self.contexts = list(contexts)
        n = len(self.contexts)
        ctxs = (C.c_void_p * n)(*[c._h for c in self.contexts])
        self._handles = (C.c_void_p * n)()
        rc = self._L.rto_comm_create_all(ctxs, n, band_rows, self._handles)
        if rc != RTO_OK:
            self._handles = None
            raise RtoError(rc, self._L.rto_last_error(self.contexts[0]._h).decode())

    def close(self):
        if getattr(self, "_handles", None):
            for h in self._handles:
                if h:
                    self._L.rto_comm_destroy(h)
            self._handles = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != RTO_OK:
            raise RtoError(rc, self._L.rto_comm_last_error(self._handles[0]).decode())

    def render_resident(self, frame: Frame, mode: int = RESIDENT_OCTREE):
        self._check(self._L.rto_comm_render_resident_all(self._handles, len(self.contexts), C.byref(frame), mode))

    def submit(self, frames_arr, d_frames: int, frame_stride_bytes: int, mode: int = RESIDENT_OCTREE):
        self._check(self._L.rto_comm_submit_all(self._handles, len(self.contexts), frames_arr, len(frames_arr), mode,
                                                C.c_void_p(d_frames), frame_stride_bytes))

    def flush(self):
        for h in self._handles:
            self._check(self._L.rto_comm_flush(h))

    def ranks_seen(self) -> int:
        n = C.c_int(0)
        self._check(self._L.rto_comm_ranks_seen(self._handles[0], C.byref(n)))
        return int(n.value)

    def is_dead(self):
        """one flag per member"""
        return [bool(self._L.rto_comm_is_dead(h)) for h in self._handles]

    def debug_abort(self, member: int = 0):
        """Test hook: abort ONE member as a flush timeout would; the whole group is dead afterwards."""
        self._check(self._L.rto_comm_debug_abort(self._handles[member]))
