"""Python face of the C++ host layer (ray_tracing_octrees_amd/host/*.cpp, librto_host.so).

Names, argument meaning and error behaviour mirror the reference's host API:
  VoxelGrid, createOctreeFromVoxelGrid, freeOctree, getVoxelSafe   453-skeleton/OctreeVoxel.h
  Camera                                                           453-skeleton/Camera.h
  loadVoxelGrid / saveVoxelGrid / loadVoxelGridPartial             453-skeleton/CacheUtils.h
  RayTracerBVH                                                     453-skeleton/RayTracerBVH.h:28-80
Everything here is a thin ctypes wrapper: the work happens in C++ and, for rendering, in the HIP
library the C++ class loads (librto_hip.so).  No oracle, no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _build
from .hip import (BRUSH_DTYPE, COMPONENT_DTYPE, DIST_SUMMARY_DTYPE, DOSE_SUMMARY_DTYPE, EXPO_SUMMARY_DTYPE, FIELD_VIEW_SUMMARY_DTYPE, GEO_SUMMARY_DTYPE, HIT_DTYPE, MEASURE_DTYPE, NEAREST_DTYPE, NECK_DTYPE, NODE_DTYPE, PART_DTYPE, PARTS_SUMMARY_DTYPE, POINT_HIT_DTYPE, REGION_DTYPE, SKEL_SUMMARY_DTYPE, SPAN_DTYPE, TRI_HIT_DTYPE,
                  THICK_MAX_C, THICK_SUMMARY_DTYPE, IsoParams, IsoSummary, DcParams, DcSummary, DUAL_VERTEX_DTYPE, RtoError, _f)

_lib = None
_vp = C.c_void_p
_f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_build.LIB_HOST):
        raise RtoError(-4, f"{_build.LIB_HOST} is not built: run __graft_entry__.build()")
    _build.preload_torch_runtime()     # the C++ class dlopens librto_hip.so later: torch's runtime must come first
    L = C.CDLL(_build.LIB_HOST)
    L.rtoh_grid_new.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, _vp]
    L.rtoh_grid_new.restype = _vp
    L.rtoh_grid_test_sphere.argtypes = [C.c_int]
    L.rtoh_grid_test_sphere.restype = _vp
    L.rtoh_grid_load.argtypes = [C.c_char_p]
    L.rtoh_grid_load.restype = _vp
    L.rtoh_grid_load_partial.argtypes = [C.c_char_p, C.c_int, C.c_int]
    L.rtoh_grid_load_partial.restype = _vp
    L.rtoh_grid_save.argtypes = [_vp, C.c_char_p]
    L.rtoh_grid_free.argtypes = [_vp]
    L.rtoh_grid_free.restype = None
    L.rtoh_grid_info.argtypes = [_vp, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.rtoh_grid_info.restype = None
    L.rtoh_grid_data.argtypes = [_vp, _vp]
    L.rtoh_grid_data.restype = None
    L.rtoh_grid_count.argtypes = [_vp]
    L.rtoh_grid_count.restype = C.c_int64
    L.rtoh_grid_recenter.argtypes = [_vp]
    L.rtoh_get_voxel_safe.argtypes = [_vp, C.c_int, C.c_int, C.c_int]
    L.rtoh_octree_build.argtypes = [_vp]
    L.rtoh_octree_build.restype = _vp
    L.rtoh_octree_free.argtypes = [_vp]
    L.rtoh_octree_free.restype = None
    L.rtoh_octree_map_size.restype = C.c_int64
    L.rtoh_octree_flatten.argtypes = [_vp, _vp, C.c_int64]
    L.rtoh_octree_flatten.restype = C.c_int64
    L.rtoh_octree_neighbors.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.rtoh_local_mc.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int64]
    L.rtoh_local_mc.restype = C.c_int64
    L.rtoh_mc_renderer.argtypes = [_vp, _vp, _vp, C.c_int64]
    L.rtoh_mc_renderer.restype = C.c_int64
    L.rtoh_build_leaf_triangles.argtypes = [_vp, _vp, C.c_int64, _vp, C.c_int64, _vp]
    L.rtoh_build_leaf_triangles.restype = C.c_int64
    L.rtoh_camera_new.argtypes = [C.c_float, C.c_float, C.c_float]
    L.rtoh_camera_new.restype = _vp
    L.rtoh_camera_free.argtypes = [_vp]
    L.rtoh_camera_free.restype = None
    L.rtoh_camera_pan.argtypes = [_vp, C.c_float, C.c_float]
    L.rtoh_camera_pan.restype = None
    L.rtoh_camera_increment.argtypes = [_vp, C.c_float, C.c_float, C.c_float]
    L.rtoh_camera_increment.restype = None
    L.rtoh_camera_set_target.argtypes = [_vp, _f32p]
    L.rtoh_camera_set_target.restype = None
    L.rtoh_camera_get.argtypes = [_vp, _f32p, _f32p, _f32p, _f32p]
    L.rtoh_camera_get.restype = None
    L.rtoh_mat4_inverse.argtypes = [_f32p, _f32p]
    L.rtoh_mat4_mul.argtypes = [_f32p, _f32p, _f32p]
    L.rtoh_perspective.argtypes = [C.c_float, C.c_float, C.c_float, C.c_float, _f32p]
    L.rtoh_radians.argtypes = [C.c_float]
    L.rtoh_radians.restype = C.c_float
    L.rtoh_frustum_test.argtypes = [_f32p, _f32p, _f32p, C.c_int64, C.c_float, _vp]
    L.rtoh_frustum_test.restype = None
    L.rtoh_rt_new.argtypes = [C.c_int]
    L.rtoh_rt_new.restype = _vp
    L.rtoh_rt_free.argtypes = [_vp]
    L.rtoh_rt_free.restype = None
    L.rtoh_rt_set_devices.argtypes = [_vp, C.c_int, C.c_int]
    L.rtoh_rt_set_devices.restype = None
    L.rtoh_rt_ensure_compute_initialized.argtypes = [_vp]
    L.rtoh_rt_ensure_compute_initialized.restype = None
    L.rtoh_rt_set_octree.argtypes = [_vp, _vp, _vp]
    L.rtoh_rt_set_octree.restype = None
    L.rtoh_rt_set_octree_from_grid.argtypes = [_vp, _vp]
    L.rtoh_rt_set_octree_from_grid.restype = None
    L.rtoh_rt_set_frustum_culling_enabled.argtypes = [_vp, C.c_int]
    L.rtoh_rt_set_frustum_culling_enabled.restype = None
    L.rtoh_rt_render_scene_compute.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_float, C.c_float]
    L.rtoh_rt_render_scene_compute.restype = None
    L.rtoh_rt_render_scene_compute_with_culling.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int]
    L.rtoh_rt_render_scene_compute_with_culling.restype = None
    L.rtoh_rt_build_leaf_triangles.argtypes = [_vp]
    L.rtoh_rt_build_leaf_triangles.restype = None
    L.rtoh_rt_build_leaf_triangles_on_host.argtypes = [_vp]
    L.rtoh_rt_build_leaf_triangles_on_host.restype = None
    L.rtoh_rt_render_scene_triangles.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int]
    L.rtoh_rt_render_scene_triangles.restype = None
    L.rtoh_rt_num_nodes.argtypes = [_vp]
    L.rtoh_rt_num_nodes.restype = C.c_int64
    L.rtoh_rt_framebuffer.argtypes = [_vp, _vp, C.c_int64, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.rtoh_rt_finish.argtypes = [_vp]
    L.rtoh_rt_finish.restype = None
    L.rtoh_rt_context.argtypes = [_vp]
    L.rtoh_rt_context.restype = _vp
    L.rtoh_rt_last_error.argtypes = [_vp]
    L.rtoh_rt_last_error.restype = C.c_char_p
    L.rtoh_rt_intersect_rays.argtypes = [_vp, _vp, C.c_int64, C.c_int, C.c_float, C.c_float, _vp]
    L.rtoh_rt_intersect_rays.restype = None
    L.rtoh_rt_render_scene_lit.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_float), C.c_int, C.c_int,
                                           C.c_float, C.c_uint32]
    L.rtoh_rt_render_scene_lit.restype = None
    L.rtoh_rt_render_surface_lit.argtypes = L.rtoh_rt_render_scene_lit.argtypes
    L.rtoh_rt_render_surface_lit.restype = None
    L.rtoh_rt_render_field.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_float, C.c_float, _vp, _vp, _vp]
    L.rtoh_rt_render_field.restype = C.c_int
    L.rtoh_rt_field_values.argtypes = [_vp, _vp, C.c_int64, _vp]
    L.rtoh_rt_field_values.restype = C.c_int64
    L.rtoh_rt_project_field.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_float, C.c_float, _vp, _vp, _vp]
    L.rtoh_rt_project_field.restype = C.c_int
    L.rtoh_rt_projection_values.argtypes = [_vp, _vp, _vp, _vp, _vp, C.c_int64]
    L.rtoh_rt_projection_values.restype = C.c_int64
    L.rtoh_projection_walk.argtypes = [_vp, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int64]
    L.rtoh_projection_walk.restype = C.c_int64
    L.rtoh_projection_reduce.argtypes = [_vp, _vp, _vp, C.c_int64, C.c_int, C.c_int32, C.c_int32, _vp]
    L.rtoh_projection_reduce.restype = None
    L.rtoh_rt_composite_field.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_float, C.c_float, _vp, _vp, _vp, _vp]
    L.rtoh_rt_composite_field.restype = C.c_int
    L.rtoh_rt_composite_values.argtypes = [_vp, _vp, _vp, _vp, _vp, C.c_int64, _vp]
    L.rtoh_rt_composite_values.restype = C.c_int64
    L.rtoh_composite_ray.argtypes = [_vp, _vp, _vp, _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp]
    L.rtoh_composite_ray.restype = None
    L.rtoh_composite_index.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int]
    L.rtoh_composite_index.restype = C.c_int
    L.rtoh_composite_thresholds.argtypes = [C.c_int, C.c_int32, C.c_int32, _vp]
    L.rtoh_composite_thresholds.restype = None
    L.rtoh_rt_pick.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _vp]
    L.rtoh_rt_pick.restype = C.c_int
    L.rtoh_rt_intersect_spans.argtypes = [_vp, _vp, C.c_int64, C.c_float, C.c_float, _vp]
    L.rtoh_rt_intersect_spans.restype = None
    L.rtoh_rt_pick_span.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _vp]
    L.rtoh_rt_pick_span.restype = C.c_int
    L.rtoh_rt_intersect_triangles.argtypes = [_vp, _vp, C.c_int64, C.c_int, C.c_float, C.c_float, _vp, _vp]
    L.rtoh_rt_intersect_triangles.restype = None
    L.rtoh_rt_pick_surface.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _vp, _vp]
    L.rtoh_rt_pick_surface.restype = C.c_int
    L.rtoh_rt_locate.argtypes = [_vp, _vp, C.c_int64, _vp]
    L.rtoh_rt_locate.restype = C.c_int
    L.rtoh_rt_census.argtypes = [_vp, _vp, _vp, C.c_int64, _vp]
    L.rtoh_rt_census.restype = C.c_int
    L.rtoh_rt_nearest_solid.argtypes = [_vp, _vp, C.c_int64, C.c_float, _vp, _vp]
    L.rtoh_rt_nearest_solid.restype = C.c_int
    L.rtoh_components_cpu.argtypes = [_vp, C.c_int, C.c_int, _vp, _vp, C.c_int64]
    L.rtoh_components_cpu.restype = C.c_int64
    L.rtoh_components_select_cpu.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int64]
    L.rtoh_components_select_cpu.restype = C.c_int64
    L.rtoh_rt_label_components.argtypes = [_vp, C.c_int, C.c_int, _vp, C.c_int64]
    L.rtoh_rt_label_components.restype = C.c_int64
    L.rtoh_rt_component_labels.argtypes = [_vp, _vp, C.c_int64]
    L.rtoh_rt_component_labels.restype = C.c_int
    L.rtoh_rt_remove_debris.argtypes = [_vp, C.c_int64, C.c_int]
    L.rtoh_rt_remove_debris.restype = C.c_int64
    L.rtoh_rt_fill_cavities.argtypes = [_vp]
    L.rtoh_rt_fill_cavities.restype = C.c_int64
    L.rtoh_rt_keep_largest.argtypes = [_vp, C.c_int]
    L.rtoh_rt_keep_largest.restype = C.c_int64
    L.rtoh_rt_flip_component_at.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.rtoh_rt_flip_component_at.restype = C.c_int64
    L.rtoh_distance_quantize.argtypes = [C.c_float, C.c_float, C.POINTER(C.c_int64)]
    L.rtoh_distance_quantize.restype = C.c_int
    L.rtoh_distance_cpu.argtypes = [_vp, C.c_int, C.c_int64, _vp, _vp]
    L.rtoh_distance_cpu.restype = C.c_int
    L.rtoh_morphology_cpu.argtypes = [_vp, C.c_int, C.c_int64]
    L.rtoh_morphology_cpu.restype = C.c_int64
    L.rtoh_rt_distance_field.argtypes = [_vp, C.c_int, C.c_float, _vp, C.c_int64, _vp]
    L.rtoh_rt_distance_field.restype = C.c_int
    L.rtoh_rt_morphology.argtypes = [_vp, C.c_int, C.c_float]
    L.rtoh_rt_morphology.restype = C.c_int64
    L.rtoh_rt_thickest_point.argtypes = [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.rtoh_rt_thickest_point.restype = C.c_int
    L.rtoh_geodesic_cpu.argtypes = [_vp, C.c_int, C.c_int, _vp, C.c_int64, C.c_int64, _vp, _vp]
    L.rtoh_geodesic_cpu.restype = C.c_int
    L.rtoh_geodesic_paths_cpu.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int64, C.c_int64, _vp, _vp]
    L.rtoh_geodesic_paths_cpu.restype = C.c_int
    L.rtoh_geodesic_flood_cpu.argtypes = [_vp, C.c_int, C.c_int, _vp, C.c_int64, C.c_int64]
    L.rtoh_geodesic_flood_cpu.restype = C.c_int64
    L.rtoh_skeleton_cpu.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int64, C.c_int64, _vp, _vp]
    L.rtoh_skeleton_cpu.restype = C.c_int
    L.rtoh_skeleton_thin_cpu.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int64, C.c_int64]
    L.rtoh_skeleton_thin_cpu.restype = C.c_int64
    L.rtoh_skeleton_simple.argtypes = [C.c_uint32, C.c_int]
    L.rtoh_skeleton_simple.restype = C.c_int
    L.rtoh_rt_skeleton_field.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int64, C.c_int64, _vp, C.c_int64, _vp]
    L.rtoh_rt_skeleton_field.restype = C.c_int
    L.rtoh_rt_thin.argtypes = [_vp, C.c_int, C.c_int64]
    L.rtoh_rt_thin.restype = C.c_int64
    L.rtoh_rt_centreline.argtypes = [_vp, C.c_int64, C.c_int64, _vp, C.c_int64, C.POINTER(C.c_int64)]
    L.rtoh_rt_centreline.restype = C.c_int
    L.rtoh_exposure_cpu.argtypes = [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.POINTER(C.c_int64)]
    L.rtoh_exposure_cpu.restype = C.c_int
    L.rtoh_rt_exposure_field.argtypes = [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp]
    L.rtoh_rt_exposure_field.restype = C.c_int
    L.rtoh_rt_exposure.argtypes = [_vp, _vp, C.c_int64]
    L.rtoh_rt_exposure.restype = C.c_int
    L.rtoh_dose_cpu.argtypes = [_vp, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int)]
    L.rtoh_dose_cpu.restype = C.c_int
    L.rtoh_rt_dose_field.argtypes = [_vp, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp]
    L.rtoh_rt_dose_field.restype = C.c_int
    L.rtoh_rt_dose.argtypes = [_vp, _vp, C.c_int64]
    L.rtoh_rt_dose.restype = C.c_int
    L.rtoh_rt_dose_coverage.argtypes = [_vp, _vp, C.c_int64, C.POINTER(C.c_int64)]
    L.rtoh_rt_dose_coverage.restype = C.c_int
    L.rtoh_rt_hottest_voxel.argtypes = [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.rtoh_rt_hottest_voxel.restype = C.c_int
    L.rtoh_rt_geodesic_field.argtypes = [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int64, _vp, C.c_int64, _vp]
    L.rtoh_rt_geodesic_field.restype = C.c_int
    L.rtoh_parts_cpu.argtypes = [_vp, C.c_int, C.c_int, C.c_int]
    L.rtoh_parts_cpu.restype = _vp
    L.rtoh_parts_counts.argtypes = [_vp, _vp]
    L.rtoh_parts_counts.restype = None
    L.rtoh_parts_copy.argtypes = [_vp, _vp, _vp, _vp, _vp]
    L.rtoh_parts_copy.restype = None
    L.rtoh_parts_free.argtypes = [_vp]
    L.rtoh_parts_free.restype = None
    L.rtoh_parts_split_cpu.argtypes = [_vp, C.c_int, C.c_int, C.c_int]
    L.rtoh_parts_split_cpu.restype = C.c_int64
    L.rtoh_rt_segment_parts.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int64, _vp]
    L.rtoh_rt_segment_parts.restype = C.c_int
    L.rtoh_rt_parts.argtypes = [_vp, _vp, C.c_int64, C.POINTER(C.c_int64)]
    L.rtoh_rt_parts.restype = C.c_int
    L.rtoh_rt_necks.argtypes = [_vp, _vp, C.c_int64, C.POINTER(C.c_int64)]
    L.rtoh_rt_necks.restype = C.c_int
    L.rtoh_rt_part_labels.argtypes = [_vp, _vp, C.c_int64]
    L.rtoh_rt_part_labels.restype = C.c_int
    L.rtoh_rt_split_at_necks.argtypes = [_vp, C.c_int, C.c_int, C.c_int]
    L.rtoh_rt_split_at_necks.restype = C.c_int64
    L.rtoh_thickness_cpu.argtypes = [_vp, C.c_int, C.c_int64, _vp, _vp, C.c_int64, C.POINTER(C.c_int64), _vp]
    L.rtoh_thickness_cpu.restype = C.c_int
    L.rtoh_rt_thickness_field.argtypes = [_vp, C.c_int, C.c_float, _vp, C.c_int64, _vp]
    L.rtoh_rt_thickness_field.restype = C.c_int
    L.rtoh_rt_thinnest_point.argtypes = [_vp, C.c_int, C.c_float, C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.rtoh_rt_thinnest_point.restype = C.c_int
    L.rtoh_rt_thickness_histogram.argtypes = [_vp, _vp, C.c_int64, C.POINTER(C.c_int64)]
    L.rtoh_rt_thickness_histogram.restype = C.c_int
    L.rtoh_measure_cpu.argtypes = [_vp, _vp, C.c_int64, C.c_int, _vp, C.c_int64, _vp]
    L.rtoh_measure_cpu.restype = C.c_int
    L.rtoh_rt_measure_components.argtypes = [_vp, C.c_int, C.c_int, _vp, C.c_int64, C.POINTER(C.c_int64), _vp]
    L.rtoh_rt_measure_components.restype = C.c_int
    L.rtoh_rt_surface_area.argtypes = [_vp, C.c_int, C.POINTER(C.c_double)]
    L.rtoh_rt_surface_area.restype = C.c_int
    L.rtoh_rt_centroid.argtypes = [_vp, C.c_int, C.POINTER(C.c_double)]
    L.rtoh_rt_centroid.restype = C.c_int
    L.rtoh_rt_topology.argtypes = [_vp, C.c_int, C.c_int, C.POINTER(C.c_int64)]
    L.rtoh_rt_topology.restype = C.c_int
    L.rtoh_rt_paths_to.argtypes = [_vp, _vp, C.c_int64, C.c_int64, _vp, _vp]
    L.rtoh_rt_paths_to.restype = C.c_int
    L.rtoh_rt_flood_from.argtypes = [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.c_int64]
    L.rtoh_rt_flood_from.restype = C.c_int64
    L.rtoh_rt_farthest_point.argtypes = [_vp, _vp, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64)]
    L.rtoh_rt_farthest_point.restype = C.c_int
    L.rtoh_rt_edit_voxels.argtypes = [_vp, _vp, _vp, _vp, C.c_int]
    L.rtoh_rt_edit_voxels.restype = C.c_int64
    L.rtoh_rt_grid.argtypes = [_vp, C.POINTER(C.c_int), _vp]
    L.rtoh_grid_load_csv.argtypes = [C.c_char_p, C.c_char_p, C.c_float]
    L.rtoh_grid_load_csv.restype = _vp
    L.rtoh_rt_load_mesh.argtypes = [_vp, _vp, C.c_int64, _vp, C.c_int64, C.c_float, C.c_int, C.c_int]
    L.rtoh_cube_renderer.argtypes = [_vp, _vp, _vp, C.c_int64]
    L.rtoh_cube_renderer.restype = C.c_int64
    L.rtoh_render_octree_planes.argtypes = [_vp, _vp, C.c_int, _vp, C.c_float, _vp, C.c_int64]
    L.rtoh_render_octree_planes.restype = C.c_int64
    L.rtoh_render_octree.argtypes = [_vp, _vp, C.c_int, _vp, C.c_float, C.c_float, _vp, C.c_int64]
    L.rtoh_render_octree.restype = C.c_int64
    L.rtoh_render_octree_planes_ms.argtypes = [_vp, _vp, C.c_int, _vp, C.c_float, C.POINTER(C.c_int64)]
    L.rtoh_render_octree_planes_ms.restype = C.c_double
    L.rtoh_rt_extract_mesh.argtypes = [_vp, C.c_int, _vp, C.c_float, _vp, C.c_float, C.POINTER(C.c_int64)]
    L.rtoh_rt_extract_mesh.restype = _vp
    L.rtoh_tris_take.argtypes = [_vp, _vp]
    L.rtoh_tris_take.restype = None
    L.rtoh_marching_cubes_volume.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_float, C.c_float, C.POINTER(C.c_int64)]
    L.rtoh_marching_cubes_volume.restype = _vp
    L.rtoh_iso_surface_volume.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_float, C.POINTER(IsoParams), C.POINTER(IsoSummary),
                                          C.POINTER(C.c_int), C.POINTER(C.c_int64)]
    L.rtoh_iso_surface_volume.restype = _vp
    L.rtoh_iso_take.argtypes = [_vp, _vp, _vp]
    L.rtoh_iso_take.restype = None
    L.rtoh_iso_surface_volume_ms.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_float, C.POINTER(IsoParams), C.POINTER(C.c_int64)]
    L.rtoh_iso_surface_volume_ms.restype = C.c_double
    L.rtoh_rt_iso_surface.argtypes = [_vp, C.c_int, C.c_float, C.c_float, C.c_int, _vp, C.POINTER(C.c_int64)]
    L.rtoh_rt_iso_surface.restype = _vp
    L.rtoh_dual_contour_volume.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_float, C.POINTER(DcParams), C.POINTER(DcSummary),
                                           C.POINTER(C.c_int), C.POINTER(C.c_int64)]
    L.rtoh_dual_contour_volume.restype = _vp
    L.rtoh_dual_contour_volume_ms.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_float, C.POINTER(DcParams), C.POINTER(C.c_int64)]
    L.rtoh_dual_contour_volume_ms.restype = C.c_double
    L.rtoh_dual_vertex_volume.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_float, _vp]
    L.rtoh_dual_vertex_volume.restype = None
    L.rtoh_adc_render.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_float, C.c_int, _vp, C.POINTER(C.c_int64)]
    L.rtoh_adc_render.restype = _vp
    L.rtoh_rt_dual_contour.argtypes = [_vp, C.POINTER(DcParams), C.POINTER(DcSummary), C.POINTER(C.c_int64)]
    L.rtoh_rt_dual_contour.restype = _vp
    L.rtoh_rt_dual_vertices.argtypes = [_vp, _vp, C.c_int64, _vp]
    L.rtoh_rt_dual_vertices.restype = C.c_int
    _lib = L
    return L


def measureComponentsCPU(labels, count: int, connectivity: int = 6):
    """Addition: measureComponentsCPU (host/Measure.h) -- the rule of rto_measure_components as plain loops over an int32 label volume
    (dimZ, dimY, dimX) with labels in [0, count), -1 outside the set: (code, table as a hip.MEASURE_DTYPE array or None when refused,
    total as a hip.MEASURE_DTYPE scalar)."""
    l = np.ascontiguousarray(labels, np.int32)
    dims = (C.c_int * 3)(l.shape[2], l.shape[1], l.shape[0])
    table = np.zeros(max(int(count), 0), MEASURE_DTYPE)
    total = np.zeros((), MEASURE_DTYPE)
    rc = int(load().rtoh_measure_cpu(dims, l.ctypes.data, int(count), int(connectivity), table.ctypes.data, len(table), total.ctypes.data))
    return rc, (table if rc == 0 else None), total


class VoxelGrid:
    """453-skeleton/OctreeVoxel.h:28-42.  data is uint8 (0 EMPTY, 1 FILLED), shape (dimZ, dimY, dimX)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_array(cls, data: np.ndarray, grid_min, voxel_size) -> "VoxelGrid":
        d = np.ascontiguousarray(data, dtype=np.uint8)
        dz, dy, dx = d.shape
        return cls(load().rtoh_grid_new(dx, dy, dz, _f(grid_min[0]), _f(grid_min[1]), _f(grid_min[2]), _f(voxel_size),
                                        d.ctypes.data))

    @classmethod
    def test_sphere(cls, dim: int) -> "VoxelGrid":
        """The reference app's fallback scene (main.cpp:337-372, 1052-1070) after recenterFilledVoxels."""
        return cls(load().rtoh_grid_test_sphere(dim))

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.rtoh_grid_free(self._h)
            self._h = None

    def _info(self):
        dims = (C.c_int * 3)()
        mn = (C.c_float * 3)()
        vs = C.c_float()
        load().rtoh_grid_info(self._h, dims, mn, C.byref(vs))
        return tuple(dims), np.array(list(mn), np.float32), np.float32(vs.value)

    @property
    def dims(self):
        return self._info()[0]

    @property
    def min(self) -> np.ndarray:
        return self._info()[1]

    @property
    def voxelSize(self) -> np.float32:
        return self._info()[2]

    @property
    def data(self) -> np.ndarray:
        dx, dy, dz = self.dims
        out = np.empty((dz, dy, dx), np.uint8)
        load().rtoh_grid_data(self._h, out.ctypes.data)
        return out

    def recenter(self) -> bool:
        return bool(load().rtoh_grid_recenter(self._h))

    def labelComponents(self, set: int = 1, connectivity: int = 6):
        """Addition: labelComponentsCPU (host/Components.h) -- the rule of rto_label_components as a breadth-first search on the
        CPU: (labels int32 (dimZ, dimY, dimX), table as hip.COMPONENT_DTYPE)."""
        dx, dy, dz = self.dims
        labels = np.empty((dz, dy, dx), np.int32)
        n = load().rtoh_components_cpu(self._h, int(set), int(connectivity), labels.ctypes.data, None, 0)
        if n < 0:
            raise ValueError("labelComponents: unknown set or connectivity, or too large a grid")
        table = np.zeros(n, COMPONENT_DTYPE)
        if n:
            load().rtoh_components_cpu(self._h, int(set), int(connectivity), None, table.ctypes.data, n)
        return labels, table

    def applyComponentSelection(self, set: int, connectivity: int, select: int, arg: int = 0) -> int:
        """Addition: applyComponentSelectionCPU -- rto_edit_components' selection and flip on this grid, on the CPU; the number
        of voxels flipped (-1: refused, the grid untouched)."""
        return int(load().rtoh_components_select_cpu(self._h, int(set), int(connectivity), int(select), int(arg)))

    def distanceField(self, set: int = 1, mq: int = -1):
        """Addition: distanceFieldCPU (host/Distance.h) -- the rule of rto_distance_field on the CPU for mq quanta (-1: no cap):
        (d2 int32 (dimZ, dimY, dimX), summary as a hip.DIST_SUMMARY_DTYPE scalar)."""
        dx, dy, dz = self.dims
        d2 = np.empty((dz, dy, dx), np.int32)
        summary = np.zeros((), DIST_SUMMARY_DTYPE)
        if not load().rtoh_distance_cpu(self._h, int(set), int(mq), d2.ctypes.data, summary.ctypes.data):
            raise ValueError("distanceField: unknown set, or a grid the 32-bit field cannot serve")
        return d2, summary

    def applyMorphology(self, op: int, rq: int) -> int:
        """Addition: applyMorphologyCPU -- rto_edit_morphology's DILATE / ERODE / OPEN / CLOSE on this grid for rq quanta, on the
        CPU; the number of voxels changed (-1: refused, the grid untouched)."""
        return int(load().rtoh_morphology_cpu(self._h, int(op), int(rq)))

    def segmentParts(self, set: int = 1, connectivity: int = 6, ratio: int = 800):
        """Addition: segmentPartsCPU (host/Parts.h) -- the rule of rto_segment_parts as plain loops on the CPU: (labels int32 (dimZ,
        dimY, dimX), parts as hip.PART_DTYPE, necks as hip.NECK_DTYPE, summary as a hip.PARTS_SUMMARY_DTYPE scalar)."""
        dx, dy, dz = self.dims
        L = load()
        h = L.rtoh_parts_cpu(self._h, int(set), int(connectivity), int(ratio))      # the segmentation runs once; the rest are copies
        if not h:
            raise ValueError("segmentParts: unknown set, connectivity or ratio, or a grid the 32-bit field cannot serve")
        try:
            counts = (C.c_int64 * 2)()
            L.rtoh_parts_counts(h, counts)
            labels = np.empty((dz, dy, dx), np.int32)
            parts, necks = np.zeros(counts[0], PART_DTYPE), np.zeros(counts[1], NECK_DTYPE)
            summary = np.zeros((), PARTS_SUMMARY_DTYPE)
            L.rtoh_parts_copy(h, labels.ctypes.data, parts.ctypes.data, necks.ctypes.data, summary.ctypes.data)
        finally:
            L.rtoh_parts_free(h)
        return labels, parts, necks, summary

    def splitAtNecks(self, set: int = 1, connectivity: int = 6, ratio: int = 800) -> int:
        """Addition: splitAtNecksCPU -- rto_edit_parts' cut on this grid, on the CPU; the number of voxels flipped (-1: refused,
        the grid untouched)."""
        return int(load().rtoh_parts_split_cpu(self._h, int(set), int(connectivity), int(ratio)))

    def thicknessField(self, medium: int = 1, mq: int = 64):
        """Addition: thicknessFieldCPU (host/Thickness.h) -- the rule of rto_thickness_field on the CPU for a radius of mq quanta:
        (code, t2 int32 (dimZ, dimY, dimX), bins int64 (c + 1), summary as a hip.THICK_SUMMARY_DTYPE scalar); t2 and bins are None
        when refused."""
        dx, dy, dz = self.dims
        t2 = np.empty((dz, dy, dx), np.int32)
        bins = np.zeros(THICK_MAX_C + 1, np.int64)
        count = C.c_int64()
        summary = np.zeros((), THICK_SUMMARY_DTYPE)
        rc = int(load().rtoh_thickness_cpu(self._h, int(medium), int(mq), t2.ctypes.data, bins.ctypes.data, bins.size, C.byref(count),
                                           summary.ctypes.data))
        if rc != 0:
            return rc, None, None, summary
        return rc, t2, bins[:count.value].copy(), summary

    def geodesicField(self, seeds, medium: int = 0, connectivity: int = 6, limit: int = 0x7fffffff):
        """Addition: geodesicFieldCPU (host/Geodesic.h) -- the rule of rto_geodesic_field on the CPU (a bucket queue): (code, g int32
        (dimZ, dimY, dimX) or None when refused, summary as a hip.GEO_SUMMARY_DTYPE scalar)."""
        dx, dy, dz = self.dims
        s = np.ascontiguousarray(np.asarray(seeds).reshape(-1), np.int64)
        g = np.empty((dz, dy, dx), np.int32)
        summary = np.zeros((), GEO_SUMMARY_DTYPE)
        rc = int(load().rtoh_geodesic_cpu(self._h, int(medium), int(connectivity), s.ctypes.data if s.size else None, s.size, int(limit),
                                          g.ctypes.data, summary.ctypes.data))
        return rc, (g if rc == 0 else None), summary

    def geodesicPaths(self, g, targets, maxLen: int, connectivity: int = 6):
        """Addition: geodesicPathsCPU -- rto_geodesic_paths on a field `g` of this grid: (code, rows (n, maxLen) int64, lengths)."""
        f = np.ascontiguousarray(g, np.int32)
        t = np.ascontiguousarray(np.asarray(targets).reshape(-1), np.int64)
        rows = np.empty((t.size, max(int(maxLen), 0)), np.int64)
        lengths = np.empty(t.size, np.int64)
        rc = int(load().rtoh_geodesic_paths_cpu(self._h, int(connectivity), f.ctypes.data, t.ctypes.data if t.size else None, t.size,
                                                int(maxLen), rows.ctypes.data if rows.size else None, lengths.ctypes.data))
        return rc, rows, lengths

    def floodGeodesic(self, seeds, medium: int = 0, connectivity: int = 6, limit: int = 0x7fffffff) -> int:
        """Addition: floodGeodesicCPU -- rto_edit_geodesic on this grid, on the CPU; the number of voxels flipped, or the refusal's
        code (negative, the grid untouched)."""
        s = np.ascontiguousarray(np.asarray(seeds).reshape(-1), np.int64)
        return int(load().rtoh_geodesic_flood_cpu(self._h, int(medium), int(connectivity), s.ctypes.data if s.size else None, s.size, int(limit)))

    def skeletonField(self, set: int = 1, connectivity: int = 26, mode: int = 0, anchors=(), maxPasses: int = 0x7fffffff):
        """Addition: skeletonFieldCPU (host/Skeleton.h) -- the rule of rto_skeleton_field on the CPU: (code, k int32 (dimZ, dimY, dimX)
        or None when refused, summary as a hip.SKEL_SUMMARY_DTYPE scalar)."""
        dx, dy, dz = self.dims
        a = np.ascontiguousarray(np.asarray(anchors).reshape(-1), np.int64)
        k = np.empty((dz, dy, dx), np.int32)
        summary = np.zeros((), SKEL_SUMMARY_DTYPE)
        rc = int(load().rtoh_skeleton_cpu(self._h, int(set), int(connectivity), int(mode), a.ctypes.data if a.size else None, a.size,
                                          int(maxPasses), k.ctypes.data, summary.ctypes.data))
        return rc, (k if rc == 0 else None), summary

    def thin(self, set: int = 1, connectivity: int = 26, mode: int = 0, anchors=(), maxPasses: int = 0x7fffffff) -> int:
        """Addition: thinCPU -- rto_edit_skeleton on this grid, on the CPU; the number of voxels flipped, or the refusal's code
        (negative, the grid untouched)."""
        a = np.ascontiguousarray(np.asarray(anchors).reshape(-1), np.int64)
        return int(load().rtoh_skeleton_thin_cpu(self._h, int(set), int(connectivity), int(mode), a.ctypes.data if a.size else None, a.size,
                                                 int(maxPasses)))

    def exposureField(self, dirs, weights=None, mode: int = 1, reach: int = 0x7fffffff, withSteps: bool = False):
        """Addition: exposureFieldCPU (host/Exposure.h) -- the rule of rto_exposure_field on the CPU: (code, e int32 (dimZ, dimY, dimX)
        or None when refused, summary as a hip.EXPO_SUMMARY_DTYPE scalar), and with withSteps the template entries tested as a
        fourth value.  `dirs` None stands for the NULL pointer."""
        dx, dy, dz = self.dims
        d, w = _expo_args(dirs, weights)
        e = np.empty((dz, dy, dx), np.int32)
        summary = np.zeros((), EXPO_SUMMARY_DTYPE)
        steps = C.c_int64()
        rc = int(load().rtoh_exposure_cpu(self._h, None if d is None else d.ctypes.data, None if w is None else w.ctypes.data,
                                          0 if d is None else len(d), int(mode), int(reach), e.ctypes.data, summary.ctypes.data, C.byref(steps)))
        out = (rc, (e if rc == 0 else None), summary)
        return out + (steps.value,) if withSteps else out

    def doseField(self, sources, transmit=None, falloff: int = 0, mode: int = 0, reach: int = 0x7fffffff, withSteps: bool = False):
        """Addition: doseFieldCPU (host/Dose.h) -- the rule of rto_dose_field on the CPU: (code, e int32 (dimZ, dimY, dimX) or None when
        refused, covered int64 (n) or None, summary as a hip.DOSE_SUMMARY_DTYPE scalar), and with withSteps the crossed voxels tested
        as a fifth value.  `sources` is (n, 4) integers i, j, k, w (None stands for the NULL pointer), `transmit` the Q16 table or
        None for plain line of sight.  After a refusal for a source outside the grid, badSource is its index (else -1)."""
        dx, dy, dz = self.dims
        s, t = _dose_args(sources, transmit)
        e = np.empty((dz, dy, dx), np.int32)
        covered = np.zeros(0 if s is None else len(s), np.int64)
        summary = np.zeros((), DOSE_SUMMARY_DTYPE)
        steps, bad = C.c_int64(), C.c_int(-1)
        rc = int(load().rtoh_dose_cpu(self._h, None if s is None else s.ctypes.data, 0 if s is None else len(s), None if t is None else t.ctypes.data,
                                      0 if t is None else len(t), int(falloff), int(mode), int(reach), e.ctypes.data,
                                      covered.ctypes.data if covered.size else None, summary.ctypes.data, C.byref(steps), C.byref(bad)))
        self.badSource = bad.value
        out = (rc, (e if rc == 0 else None), (covered if rc == 0 else None), summary)
        return out + (steps.value,) if withSteps else out


def _dose_args(sources, transmit):
    """(sources as contiguous (n, 4) int32 or None, the table as contiguous uint32 or None) for the dose entry points.  An (n, 4)
    array of n = 0 sources stays an array: the entry point refuses it, not the wrapper."""
    s = None if sources is None else np.ascontiguousarray(np.asarray(sources, np.int32).reshape(-1, 4))
    t = None if transmit is None else np.ascontiguousarray(np.asarray(transmit, np.uint32).reshape(-1))
    return s, t


def _expo_args(dirs, weights):
    """(dirs as contiguous (n, 3) int32 or None, weights as contiguous int32 or None) for the exposure entry points."""
    d = None if dirs is None else np.ascontiguousarray(np.asarray(dirs, np.int32).reshape(-1, 3))
    w = None if weights is None else np.ascontiguousarray(np.asarray(weights, np.int32).reshape(-1))
    if d is not None and w is not None and len(w) != len(d):
        raise ValueError("one weight per direction")
    return d, w


def loadCSVDataIntoVoxelGrid(vertsFilename: str, facesFilename: str, voxelSize: float = 5.0) -> VoxelGrid:
    """The reference's CSV loader (host/BuildingLoader.h): the two CSVs parsed on the host, voxelized on GPU 0, not recentred.
    No vertex row or no face row: an empty grid (dims 0)."""
    return VoxelGrid(load().rtoh_grid_load_csv(str(vertsFilename).encode(), str(facesFilename).encode(), _f(voxelSize)))


def getVoxelSafe(grid: VoxelGrid, x: int, y: int, z: int) -> int:
    return load().rtoh_get_voxel_safe(grid._h, x, y, z)


def loadVoxelGrid(filename: str) -> VoxelGrid | None:
    h = load().rtoh_grid_load(filename.encode())
    return VoxelGrid(h) if h else None


def loadVoxelGridPartial(filename: str, startLayer: int, numLayers: int) -> VoxelGrid | None:
    h = load().rtoh_grid_load_partial(filename.encode(), startLayer, numLayers)
    return VoxelGrid(h) if h else None


def saveVoxelGrid(filename: str, grid: VoxelGrid) -> bool:
    return bool(load().rtoh_grid_save(grid._h, filename.encode()))


class OctreeNode:
    """Opaque handle of the root of a pointer octree (453-skeleton/OctreeVoxel.h:45-62)."""

    def __init__(self, handle):
        self._h = handle

    def flatten(self) -> np.ndarray:
        """BFS numbering of RayTracerBVH::setOctree (RayTracerBVH.cpp:443-490) as a GPUNodes array."""
        n = load().rtoh_octree_flatten(self._h, None, 0)
        out = np.zeros(n, NODE_DTYPE)
        load().rtoh_octree_flatten(self._h, out.ctypes.data, n)
        return out


def createOctreeFromVoxelGrid(grid: VoxelGrid) -> OctreeNode | None:
    h = load().rtoh_octree_build(grid._h)
    return OctreeNode(h) if h else None


def localMC(grid: VoxelGrid, x0: int, y0: int, z0: int, size: int) -> np.ndarray:
    """453-skeleton/OctreeVoxel.cpp:780-879.  Returns (n, 18) float32: v0,v1,v2 then the three (equal) normals."""
    n = load().rtoh_local_mc(grid._h, x0, y0, z0, size, None, 0)
    out = np.zeros((n, 18), np.float32)
    if n:
        load().rtoh_local_mc(grid._h, x0, y0, z0, size, out.ctypes.data, n)
    return out


def buildLeafTriangles(grid: VoxelGrid, nodes: np.ndarray):
    """Triangle buffer of the config-5 ray path: (tris (n, 12) float32, triOffset (numNodes+1,) int32)."""
    nodes = np.ascontiguousarray(nodes)
    n = load().rtoh_build_leaf_triangles(grid._h, nodes.ctypes.data, len(nodes), None, 0, None)
    tris = np.zeros((n, 12), np.float32)
    off = np.zeros(len(nodes) + 1, np.int32)
    load().rtoh_build_leaf_triangles(grid._h, nodes.ctypes.data, len(nodes), tris.ctypes.data, n, off.ctypes.data)
    return tris, off


class MarchingCubesRenderer:
    """453-skeleton/Renderer.h:18-24: localMC over every leaf of the tree, in child order."""

    def render(self, root: OctreeNode, grid: VoxelGrid) -> np.ndarray:
        n = load().rtoh_mc_renderer(root._h, grid._h, None, 0)
        out = np.zeros((n, 18), np.float32)
        if n:
            load().rtoh_mc_renderer(root._h, grid._h, out.ctypes.data, n)
        return out


class VoxelCubeRenderer:
    """453-skeleton/Renderer.h:29-55: a cube per solid leaf, the faces whose centre looks at an EMPTY voxel or out of the grid."""

    def render(self, root: OctreeNode, grid: VoxelGrid) -> np.ndarray:
        n = load().rtoh_cube_renderer(root._h, grid._h, None, 0)
        out = np.zeros((n, 18), np.float32)
        if n:
            load().rtoh_cube_renderer(root._h, grid._h, out.ctypes.data, n)
        return out


def _tris18(call) -> np.ndarray:
    n = call(None, 0)
    out = np.zeros((n, 18), np.float32)
    if n:
        call(out.ctypes.data, n)
    return out


def renderOctree(root: OctreeNode, grid: VoxelGrid, renderer, camera: "Camera", aspect: float, extraMargin: float = 50.0) -> np.ndarray:
    """453-skeleton/main.cpp:95-208 on the CPU: the depth-first walk with frustum culling, `renderer` (a MarchingCubesRenderer or
    a VoxelCubeRenderer) on every leaf it reaches.  (n, 18) float32 as localMC returns them."""
    kind = 1 if isinstance(renderer, VoxelCubeRenderer) else 0
    return _tris18(lambda p, n: load().rtoh_render_octree(root._h, grid._h, kind, camera._h, _f(aspect), _f(extraMargin), p, n))


def renderOctreePlanes(root: OctreeNode, grid: VoxelGrid, renderer, planes, extraMargin: float) -> np.ndarray:
    """Addition: the same walk over caller-supplied planes (24 floats; None: nothing is culled)."""
    kind = 1 if isinstance(renderer, VoxelCubeRenderer) else 0
    pl = None if planes is None else np.ascontiguousarray(np.asarray(planes, np.float32).reshape(24))
    return _tris18(lambda p, n: load().rtoh_render_octree_planes(root._h, grid._h, kind, None if pl is None else pl.ctypes.data,
                                                                 _f(extraMargin), p, n))


def renderOctreePlanesMs(root: OctreeNode, grid: VoxelGrid, renderer, planes, extraMargin: float):
    """Addition: (milliseconds of one renderOctreePlanes walk, timed inside the library as the reference times its own; triangles)."""
    kind = 1 if isinstance(renderer, VoxelCubeRenderer) else 0
    pl = None if planes is None else np.ascontiguousarray(np.asarray(planes, np.float32).reshape(24))
    n = C.c_int64(0)
    ms = load().rtoh_render_octree_planes_ms(root._h, grid._h, kind, None if pl is None else pl.ctypes.data, _f(extraMargin), C.byref(n))
    return float(ms), int(n.value)


def marchingCubesVolume(scalarField, origin, spacing: float, isoValue: float) -> np.ndarray:
    """453-skeleton/MarchingCubes.cpp:622-689 on the CPU: whole-volume marching cubes of a float field (dimZ, dimY, dimX) whose
    sample (0, 0, 0) lies at `origin`.  (n, 18) float32 as localMC returns them, the reference's placeholder normals included."""
    f = np.ascontiguousarray(np.asarray(scalarField, np.float32))
    dz, dy, dx = f.shape
    o = np.ascontiguousarray(np.asarray(origin, np.float32).reshape(3))
    n = C.c_int64(0)
    lst = load().rtoh_marching_cubes_volume(f.ctypes.data, dx, dy, dz, o.ctypes.data, _f(spacing), _f(isoValue), C.byref(n))
    out = np.zeros((n.value, 18), np.float32)
    load().rtoh_tris_take(lst, out.ctypes.data)
    return out


def isoSurfaceVolume(volume, gridMin, voxelSize: float, params: IsoParams):
    """Addition: the field isosurface rule on the CPU, a plain triple loop over the cells of an int32 volume
    (dimZ, dimY, dimX).  Returns (tris (n, 18) float32, tri_cell (n,) int32, IsoSummary); RtoError where the C ABI refuses."""
    v = np.ascontiguousarray(np.asarray(volume, np.int32))
    dz, dy, dx = v.shape
    g = np.ascontiguousarray(np.asarray(gridMin, np.float32).reshape(3))
    n, rc, summary = C.c_int64(0), C.c_int(0), IsoSummary()
    lst = load().rtoh_iso_surface_volume(v.ctypes.data, dx, dy, dz, g.ctypes.data, _f(voxelSize), C.byref(params), C.byref(summary),
                                         C.byref(rc), C.byref(n))
    out = np.zeros((n.value, 18), np.float32)
    cell = np.zeros(n.value, np.int32)
    load().rtoh_iso_take(lst, out.ctypes.data, cell.ctypes.data)                # one extraction: copied out and freed
    if rc.value != 0:
        raise RtoError(rc.value, "isoSurfaceVolume: invalid parameters")
    return out, cell, summary


def isoSurfaceVolumeMs(volume, gridMin, voxelSize: float, params: IsoParams):
    """Addition: (milliseconds of one isoSurfaceVolume on one core, timed inside the library; triangles)."""
    v = np.ascontiguousarray(np.asarray(volume, np.int32))
    dz, dy, dx = v.shape
    g = np.ascontiguousarray(np.asarray(gridMin, np.float32).reshape(3))
    n = C.c_int64(0)
    ms = load().rtoh_iso_surface_volume_ms(v.ctypes.data, dx, dy, dz, g.ctypes.data, _f(voxelSize), C.byref(params), C.byref(n))
    return float(ms), int(n.value)


def _dc_grid(voxels, gridMin):
    v = np.ascontiguousarray(np.asarray(voxels, np.uint8))
    dz, dy, dx = v.shape
    return v, dx, dy, dz, np.ascontiguousarray(np.asarray(gridMin, np.float32).reshape(3))


def dualContourVolume(voxels, gridMin, voxelSize: float, params: DcParams):
    """Addition: the dual-contouring rule on the CPU, a plain triple loop over the cells of a uint8 grid
    (dimZ, dimY, dimX; 1 is FILLED).  Returns (tris (n, 18) float32, tri_cell (n,) int32, DcSummary); RtoError where the C ABI refuses."""
    v, dx, dy, dz, g = _dc_grid(voxels, gridMin)
    n, rc, summary = C.c_int64(0), C.c_int(0), DcSummary()
    lst = load().rtoh_dual_contour_volume(v.ctypes.data, dx, dy, dz, g.ctypes.data, _f(voxelSize), C.byref(params), C.byref(summary),
                                          C.byref(rc), C.byref(n))
    out = np.zeros((n.value, 18), np.float32)
    cell = np.zeros(n.value, np.int32)
    load().rtoh_iso_take(lst, out.ctypes.data, cell.ctypes.data)                # one extraction: copied out and freed
    if rc.value != 0:
        raise RtoError(rc.value, "dualContourVolume: invalid parameters")
    return out, cell, summary


def dualContourVolumeMs(voxels, gridMin, voxelSize: float, params: DcParams):
    """Addition: (milliseconds of one dualContourVolume on one core, timed inside the library; triangles)."""
    v, dx, dy, dz, g = _dc_grid(voxels, gridMin)
    n = C.c_int64(0)
    ms = load().rtoh_dual_contour_volume_ms(v.ctypes.data, dx, dy, dz, g.ctypes.data, _f(voxelSize), C.byref(params), C.byref(n))
    return float(ms), int(n.value)


def dualVertexVolume(voxels, gridMin, voxelSize: float) -> np.ndarray:
    """Addition: the dual-contouring vertex of every voxel on the CPU, by the arithmetic the kernels run: a DUAL_VERTEX_DTYPE
    array (dimZ, dimY, dimX)."""
    v, dx, dy, dz, g = _dc_grid(voxels, gridMin)
    out = np.zeros((dz, dy, dx), DUAL_VERTEX_DTYPE)
    load().rtoh_dual_vertex_volume(v.ctypes.data, dx, dy, dz, g.ctypes.data, _f(voxelSize), out.ctypes.data)
    return out


def adaptiveDualContouringVertices(voxels, gridMin, voxelSize: float) -> np.ndarray:
    """AdaptiveDualContouringRenderer's per-voxel vertex rule in the reference's own shape (gatherHermiteData(size 1),
    generateDualVertex, QEFSolver): (dimZ, dimY, dimX, 4) float32, w the number of Hermite points."""
    v, dx, dy, dz, g = _dc_grid(voxels, gridMin)
    out = np.zeros((dz, dy, dx, 4), np.float32)
    load().rtoh_adc_render(v.ctypes.data, dx, dy, dz, g.ctypes.data, _f(voxelSize), 0, out.ctypes.data, None)
    return out


def adaptiveDualContouringRender(voxels, gridMin, voxelSize: float) -> np.ndarray:
    """AdaptiveDualContouringRenderer::render's top-level call on the CPU: (n, 18) float32."""
    v, dx, dy, dz, g = _dc_grid(voxels, gridMin)
    n = C.c_int64(0)
    lst = load().rtoh_adc_render(v.ctypes.data, dx, dy, dz, g.ctypes.data, _f(voxelSize), 1, None, C.byref(n))
    out = np.zeros((n.value, 18), np.float32)
    load().rtoh_tris_take(lst, out.ctypes.data)
    return out


def freeOctree(root: OctreeNode | None):
    if root is not None and root._h:
        load().rtoh_octree_free(root._h)
        root._h = None


class Camera:
    """453-skeleton/Camera.h:5-44."""

    def __init__(self, theta: float, phi: float, radius: float):
        self._h = load().rtoh_camera_new(_f(theta), _f(phi), _f(radius))

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.rtoh_camera_free(self._h)
            self._h = None

    def _get(self):
        view = np.zeros(16, np.float32); pos = np.zeros(3, np.float32)
        tgt = np.zeros(3, np.float32); tpr = np.zeros(3, np.float32)
        load().rtoh_camera_get(self._h, view, pos, tgt, tpr)
        return view, pos, tgt, tpr

    def getView(self) -> np.ndarray:
        return self._get()[0]

    def getPos(self) -> np.ndarray:
        return self._get()[1]

    def getTarget(self) -> np.ndarray:
        return self._get()[2]

    def pan(self, dx: float, dy: float):
        load().rtoh_camera_pan(self._h, _f(dx), _f(dy))

    def incrementTheta(self, dt: float):
        load().rtoh_camera_increment(self._h, _f(dt), 0.0, 0.0)

    def incrementPhi(self, dp: float):
        load().rtoh_camera_increment(self._h, 0.0, _f(dp), 0.0)

    def incrementR(self, dr: float):
        load().rtoh_camera_increment(self._h, 0.0, 0.0, _f(dr))

    def setTarget(self, t):
        load().rtoh_camera_set_target(self._h, np.ascontiguousarray(t, dtype=np.float32))

    @property
    def theta(self):
        return self._get()[3][0]

    @property
    def phi(self):
        return self._get()[3][1]

    @property
    def radius(self):
        return self._get()[3][2]


class RayTracerBVH:
    """The C++ drop-in class (host/RayTracerBVH.h), method for method.

    Usage is the reference's (453-skeleton/main.cpp:1127-1131, 1357-1363):
        rt = RayTracerBVH(); rt.ensureComputeInitialized(); rt.setOctree(root, grid)
        rt.renderSceneComputeWithCulling(camera, W, H, aspect, 45.0, updateFrustum)
        img = rt.framebuffer()          # the one addition: read the frame back
    Render calls return None like the reference's void methods; failures go to stderr from C++.
    """

    def __init__(self, device: int = 0):
        self._h = load().rtoh_rt_new(device)
        self._keep = None

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.rtoh_rt_free(self._h)
            self._h = None

    def setDevices(self, n: int, bandRows: int = 16):
        """Before ensureComputeInitialized(): split every frame over n GPUs of this node + ONE RCCL gather (rto_comm_*)."""
        load().rtoh_rt_set_devices(self._h, n, bandRows)

    def ensureComputeInitialized(self):
        load().rtoh_rt_ensure_compute_initialized(self._h)

    def setOctree(self, root: OctreeNode | None, grid: VoxelGrid):
        self._keep = (root, grid)
        load().rtoh_rt_set_octree(self._h, root._h if root is not None else None, grid._h)

    def setOctreeFromGrid(self, grid: VoxelGrid):
        """Addition: build the octree on the GPU straight from the voxel grid (rto_build_octree)."""
        self._keep = (None, grid)
        load().rtoh_rt_set_octree_from_grid(self._h, grid._h)

    def setFrustumCullingEnabled(self, enabled: bool):
        load().rtoh_rt_set_frustum_culling_enabled(self._h, 1 if enabled else 0)

    def renderSceneCompute(self, camera: Camera, width: int, height: int, aspect: float, fovDeg: float):
        load().rtoh_rt_render_scene_compute(self._h, camera._h, width, height, _f(aspect), _f(fovDeg))

    def renderSceneComputeWithCulling(self, camera: Camera, width: int, height: int, aspect: float, fovDeg: float,
                                      updateFrustum: bool):
        load().rtoh_rt_render_scene_compute_with_culling(self._h, camera._h, width, height, _f(aspect), _f(fovDeg),
                                                         1 if updateFrustum else 0)

    # -- additions ---------------------------------------------------------
    def buildLeafTriangles(self):
        """Config 5: per-leaf Marching-Cubes triangles of the grid given to setOctree(), built in HBM."""
        load().rtoh_rt_build_leaf_triangles(self._h)

    def buildLeafTrianglesOnHost(self):
        """The same buffer made by the C++ host builder (localMC per leaf) and uploaded: cross-check of the GPU build."""
        load().rtoh_rt_build_leaf_triangles_on_host(self._h)

    def renderSceneTriangles(self, camera: Camera, width: int, height: int, aspect: float, fovDeg: float, shadow: bool = True):
        load().rtoh_rt_render_scene_triangles(self._h, camera._h, width, height, _f(aspect), _f(fovDeg), 1 if shadow else 0)

    def renderSceneLit(self, camera: Camera, width: int, height: int, aspect: float, fovDeg: float, lightDir=(-1.0, -1.0, -1.0),
                       shadow: bool = True, aoSamples: int = 0, aoRadius: float = 1.0, seed: int = 0):
        """Addition: RayTracerBVH::renderSceneLit -- renderSceneCompute's frame with a shadow ray and aoSamples ambient-occlusion
        rays per hit pixel; read it with framebuffer()."""
        ld = (C.c_float * 3)(*[_f(x) for x in lightDir])
        load().rtoh_rt_render_scene_lit(self._h, camera._h, width, height, _f(aspect), _f(fovDeg), ld, 1 if shadow else 0,
                                        int(aoSamples), _f(aoRadius), int(seed) & 0xFFFFFFFF)

    def renderSurfaceLit(self, camera: Camera, width: int, height: int, aspect: float, fovDeg: float, lightDir=(-1.0, -1.0, -1.0),
                         shadow: bool = True, aoSamples: int = 0, aoRadius: float = 1.0, seed: int = 0):
        """Addition: RayTracerBVH::renderSurfaceLit -- renderSceneTriangles' frame lit the same way; needs
        buildLeafTriangles().  Without triangles resident there is no frame and lastError says why."""
        ld = (C.c_float * 3)(*[_f(x) for x in lightDir])
        load().rtoh_rt_render_surface_lit(self._h, camera._h, width, height, _f(aspect), _f(fovDeg), ld, 1 if shadow else 0,
                                          int(aoSamples), _f(aoRadius), int(seed) & 0xFFFFFFFF)

    def renderField(self, camera: Camera, width: int, height: int, aspect: float, fovDeg: float, view, lut, volume=None) -> int:
        """Addition: RayTracerBVH::renderField -- a frame coloured by a per-voxel int32 volume of the resident grid (DESIGN.md
        section 27).  view: a hip.FieldView; lut: 256 uint32 (hip.ramp_lut); volume: the (dimZ, dimY, dimX) int32 array of
        hip.FIELD_CALLER.  RTO_OK or the refusal's code (lastError); read the frame with framebuffer(), the values with
        fieldValues(), the counts and range with fieldSummary()."""
        lut = np.ascontiguousarray(lut, dtype=np.uint32)
        if lut.shape != (256,):
            raise ValueError("renderField: the LUT has 256 entries")
        vol = None if volume is None else np.ascontiguousarray(volume, dtype=np.int32)
        if vol is not None:
            dims = (C.c_int * 3)()
            load().rtoh_rt_grid(self._h, dims, None)
            if vol.shape != (dims[2], dims[1], dims[0]):
                raise ValueError(f"renderField: the volume must be {(dims[2], dims[1], dims[0])}, not {vol.shape}")
        return int(load().rtoh_rt_render_field(self._h, camera._h, int(width), int(height), _f(aspect), _f(fovDeg), C.addressof(view),
                                               lut.ctypes.data, vol.ctypes.data if vol is not None else None))

    def fieldValues(self) -> np.ndarray | None:
        """Addition: RayTracerBVH::fieldValues -- the last renderField's value under every pixel, (H, W) int32
        (hip.FIELD_PIXEL_MISS / FIELD_PIXEL_NONE where there is none); None when no field view has been rendered."""
        w, h = C.c_int(), C.c_int()
        n = int(load().rtoh_rt_field_values(self._h, None, 0, None))
        if n == 0 or not load().rtoh_rt_framebuffer(self._h, None, 0, C.byref(w), C.byref(h)) or w.value * h.value != n:
            return None
        out = np.empty((h.value, w.value), np.int32)
        load().rtoh_rt_field_values(self._h, out.ctypes.data, out.size, None)
        return out

    def fieldSummary(self):
        """Addition: RayTracerBVH::fieldSummary -- the last renderField's hits, valued, vmin, vmax and the range used, as a
        hip.FIELD_VIEW_SUMMARY_DTYPE record."""
        s = np.zeros(1, FIELD_VIEW_SUMMARY_DTYPE)
        load().rtoh_rt_field_values(self._h, None, 0, s.ctypes.data)
        return s[0]

    def projectField(self, camera: Camera, width: int, height: int, aspect: float, fovDeg: float, projection, lut, volume=None) -> int:
        """Addition: RayTracerBVH::projectField -- a frame whose pixels reduce a per-voxel int32 volume of the resident grid over
        the voxels their rays cross.  projection: a hip.FieldProjection; lut and volume as renderField's.
        RTO_OK or the refusal's code (lastError); read the frame with framebuffer(), the per-pixel outputs with
        projectionValues(), the counts and range with fieldSummary()."""
        lut = np.ascontiguousarray(lut, dtype=np.uint32)
        if lut.shape != (256,):
            raise ValueError("projectField: the LUT has 256 entries")
        vol = None if volume is None else np.ascontiguousarray(volume, dtype=np.int32)
        if vol is not None:
            dims = (C.c_int * 3)()
            load().rtoh_rt_grid(self._h, dims, None)
            if vol.shape != (dims[2], dims[1], dims[0]):
                raise ValueError(f"projectField: the volume must be {(dims[2], dims[1], dims[0])}, not {vol.shape}")
        return int(load().rtoh_rt_project_field(self._h, camera._h, int(width), int(height), _f(aspect), _f(fovDeg),
                                                C.addressof(projection), lut.ctypes.data, vol.ctypes.data if vol is not None else None))

    def projectionValues(self):
        """Addition: RayTracerBVH::projectionValues -- the last projectField's (values, voxels, sums, counts), (H, W) each; None
        when no projection has been rendered."""
        w, h = C.c_int(), C.c_int()
        n = int(load().rtoh_rt_projection_values(self._h, None, None, None, None, 0))
        if n == 0 or not load().rtoh_rt_framebuffer(self._h, None, 0, C.byref(w), C.byref(h)) or w.value * h.value != n:
            return None
        shape = (h.value, w.value)
        values, voxels, counts = np.empty(shape, np.int32), np.empty(shape, np.int32), np.empty(shape, np.int32)
        sums = np.empty(shape, np.int64)
        load().rtoh_rt_projection_values(self._h, values.ctypes.data, voxels.ctypes.data, sums.ctypes.data, counts.ctypes.data, n)
        return values, voxels, sums, counts

    def compositeField(self, camera: Camera, width: int, height: int, aspect: float, fovDeg: float, composite, lut, volume=None,
                       under=None) -> int:
        """Addition: RayTracerBVH::compositeField -- a frame in which a per-voxel int32 volume of the resident grid is seen
        through, LUT colour and opacity composited front to back.  composite: a hip.FieldComposite; lut and
        volume as renderField's; under: None or an (H, W, 4) float32 frame to composite over.  RTO_OK or the refusal's code
        (lastError); read the frame with framebuffer(), the per-pixel outputs with compositeValues(), the counts with
        compositeSummary()."""
        lut = np.ascontiguousarray(lut, dtype=np.uint32)
        if lut.shape != (256,):
            raise ValueError("compositeField: the LUT has 256 entries")
        vol = None if volume is None else np.ascontiguousarray(volume, dtype=np.int32)
        if vol is not None:
            dims = (C.c_int * 3)()
            load().rtoh_rt_grid(self._h, dims, None)
            if vol.shape != (dims[2], dims[1], dims[0]):
                raise ValueError(f"compositeField: the volume must be {(dims[2], dims[1], dims[0])}, not {vol.shape}")
        und = None if under is None else np.ascontiguousarray(under, dtype=np.float32)
        if und is not None and und.shape != (int(height), int(width), 4):
            raise ValueError(f"compositeField: under must be {(int(height), int(width), 4)}, not {und.shape}")
        return int(load().rtoh_rt_composite_field(self._h, camera._h, int(width), int(height), _f(aspect), _f(fovDeg),
                                                  C.addressof(composite), lut.ctypes.data, vol.ctypes.data if vol is not None else None,
                                                  und.ctypes.data if und is not None else None))

    def compositeValues(self):
        """Addition: RayTracerBVH::compositeValues -- the last compositeField's (transmittance, first, stops, counts), (H, W) each;
        None when no composite has been rendered."""
        w, h = C.c_int(), C.c_int()
        n = int(load().rtoh_rt_composite_values(self._h, None, None, None, None, 0, None))
        if n == 0 or not load().rtoh_rt_framebuffer(self._h, None, 0, C.byref(w), C.byref(h)) or w.value * h.value != n:
            return None
        shape = (h.value, w.value)
        trans = np.empty(shape, np.uint32)
        first, stops, counts = np.empty(shape, np.int32), np.empty(shape, np.int32), np.empty(shape, np.int32)
        load().rtoh_rt_composite_values(self._h, trans.ctypes.data, first.ctypes.data, stops.ctypes.data, counts.ctypes.data, n, None)
        return trans, first, stops, counts

    def compositeSummary(self):
        """Addition: RayTracerBVH::compositeSummary -- the last compositeField's hip.COMPOSITE_SUMMARY_DTYPE record."""
        from .hip import COMPOSITE_SUMMARY_DTYPE
        s = np.zeros(1, COMPOSITE_SUMMARY_DTYPE)
        load().rtoh_rt_composite_values(self._h, None, None, None, None, 0, s.ctypes.data)
        return s[0]

    def framebuffer(self) -> np.ndarray | None:
        w, h = C.c_int(), C.c_int()
        if not load().rtoh_rt_framebuffer(self._h, None, 0, C.byref(w), C.byref(h)):
            return None
        out = np.empty((h.value, w.value, 4), np.float32)
        load().rtoh_rt_framebuffer(self._h, out.ctypes.data, out.size, C.byref(w), C.byref(h))
        return out

    def intersectRays(self, origins, dirs, mode: int = 1, tMin: float = 0.0, tMax: float = 1e30) -> np.ndarray:
        """Addition: RayTracerBVH::intersectRays -- rays (origins (n, 3) or one origin, dirs (n, 3)) through the resident octree;
        a structured array of rto_hit records (hip.HIT_DTYPE; node -1 = miss).  mode: 0 first, 1 closest (default), 2 any."""
        d = np.asarray(dirs, np.float32).reshape(-1, 3)
        o = np.broadcast_to(np.asarray(origins, np.float32).reshape(-1, 3), d.shape)
        rays = np.ascontiguousarray(np.concatenate([o, d], 1), dtype=np.float32)
        hits = np.zeros(len(d), HIT_DTYPE)
        load().rtoh_rt_intersect_rays(self._h, rays.ctypes.data, len(d), int(mode), _f(tMin), _f(tMax), hits.ctypes.data)
        return hits

    def pick(self, camera: Camera, px: int, py: int, width: int, height: int, aspect: float, fovDeg: float):
        """Addition: RayTracerBVH::pick -- the leaf renderSceneCompute shows at pixel (px, py): an rto_hit record, or None."""
        out = np.zeros(1, HIT_DTYPE)
        hit = load().rtoh_rt_pick(self._h, camera._h, int(px), int(py), int(width), int(height), _f(aspect), _f(fovDeg), out.ctypes.data)
        return out[0] if hit else None

    def intersectSpans(self, origins, dirs, tMin: float = 0.0, tMax: float = 1e30) -> np.ndarray:
        """Addition: RayTracerBVH::intersectSpans -- the solid path length of rays (origins (n, 3) or one origin, dirs (n, 3))
        through the resident octree; a structured array of rto_span records (hip.SPAN_DTYPE; leaves 0 = miss)."""
        d = np.asarray(dirs, np.float32).reshape(-1, 3)
        o = np.broadcast_to(np.asarray(origins, np.float32).reshape(-1, 3), d.shape)
        rays = np.ascontiguousarray(np.concatenate([o, d], 1), dtype=np.float32)
        spans = np.zeros(len(d), SPAN_DTYPE)
        load().rtoh_rt_intersect_spans(self._h, rays.ctypes.data, len(d), _f(tMin), _f(tMax), spans.ctypes.data)
        return spans

    def pickSpan(self, camera: Camera, px: int, py: int, width: int, height: int, aspect: float, fovDeg: float):
        """Addition: RayTracerBVH::pickSpan -- the span of renderSceneCompute's ray through pixel (px, py): an rto_span record, or None."""
        out = np.zeros(1, SPAN_DTYPE)
        hit = load().rtoh_rt_pick_span(self._h, camera._h, int(px), int(py), int(width), int(height), _f(aspect), _f(fovDeg), out.ctypes.data)
        return out[0] if hit else None

    def intersectTriangles(self, origins, dirs, mode: int = 1, tMin: float = 0.0, tMax: float = 1e30):
        """Addition: RayTracerBVH::intersectTriangles -- rays against the resident leaf triangles.  Returns (hits, points): a
        structured array of rto_tri_hit records (hip.TRI_HIT_DTYPE; tri -1 = miss) and the (n, 3) hit points o + d t (0 for a
        miss).  mode: 0 first, 1 closest (default), 2 any."""
        d = np.asarray(dirs, np.float32).reshape(-1, 3)
        o = np.broadcast_to(np.asarray(origins, np.float32).reshape(-1, 3), d.shape)
        rays = np.ascontiguousarray(np.concatenate([o, d], 1), dtype=np.float32)
        hits = np.zeros(len(d), TRI_HIT_DTYPE)
        points = np.zeros((len(d), 3), np.float32)
        load().rtoh_rt_intersect_triangles(self._h, rays.ctypes.data, len(d), int(mode), _f(tMin), _f(tMax), hits.ctypes.data,
                                           points.ctypes.data)
        return hits, points

    def pickSurface(self, camera: Camera, px: int, py: int, width: int, height: int, aspect: float, fovDeg: float):
        """Addition: RayTracerBVH::pickSurface -- the triangle renderSceneTriangles shows at pixel (px, py): (rto_tri_hit record,
        point (3,)), or None."""
        out = np.zeros(1, TRI_HIT_DTYPE)
        point = np.zeros(3, np.float32)
        hit = load().rtoh_rt_pick_surface(self._h, camera._h, int(px), int(py), int(width), int(height), _f(aspect), _f(fovDeg),
                                          out.ctypes.data, point.ctypes.data)
        return (out[0], point) if hit else None

    def editVoxels(self, brushes) -> int:
        """Addition: RayTracerBVH::editVoxels -- hip.BRUSH_DTYPE brushes (hip.make_brushes), in order, on the grid every GPU holds,
        then the rebuild there.  Returns the number of voxels changed (-1: the edit failed, see lastError)."""
        b = np.asarray(brushes, BRUSH_DTYPE).reshape(-1)
        f = np.ascontiguousarray(np.concatenate([b["centre"], b["extent"]], 1), dtype=np.float32)
        shapes = np.ascontiguousarray(b["shape"], dtype=np.int32)
        ops = np.ascontiguousarray(b["op"], dtype=np.int32)
        return int(load().rtoh_rt_edit_voxels(self._h, f.ctypes.data, shapes.ctypes.data, ops.ctypes.data, len(b)))

    def labelComponents(self, set: int = 1, connectivity: int = 6):
        """Addition: RayTracerBVH::labelComponents -- the resident grid's components (hip.SET_*, hip.CONN_*) as a
        hip.COMPONENT_DTYPE table in ascending order of root; None on an error (lastError)."""
        n = load().rtoh_rt_label_components(self._h, int(set), int(connectivity), None, 0)
        if n < 0:
            return None
        table = np.zeros(n, COMPONENT_DTYPE)
        if n and load().rtoh_rt_label_components(self._h, int(set), int(connectivity), table.ctypes.data, n) != n:
            return None
        return table

    def componentLabels(self):
        """Addition: RayTracerBVH::componentLabels -- the last labelling's volume, int32 (dimZ, dimY, dimX); None when no labels
        are resident (not labelled, or the grid has changed since)."""
        dims = (C.c_int * 3)()
        load().rtoh_rt_grid(self._h, dims, None)
        out = np.empty((dims[2], dims[1], dims[0]), np.int32)
        return out if load().rtoh_rt_component_labels(self._h, out.ctypes.data, out.size) else None

    def removeDebris(self, minVoxels: int, connectivity: int = 6) -> int:
        """Addition: RayTracerBVH::removeDebris -- clears the solid components of fewer than minVoxels voxels; voxels flipped."""
        return int(load().rtoh_rt_remove_debris(self._h, int(minVoxels), int(connectivity)))

    def fillCavities(self) -> int:
        """Addition: RayTracerBVH::fillCavities -- fills the empty space no 6-connected path joins to a face of the grid."""
        return int(load().rtoh_rt_fill_cavities(self._h))

    def keepLargest(self, connectivity: int = 6) -> int:
        """Addition: RayTracerBVH::keepLargest -- clears every solid component but the largest."""
        return int(load().rtoh_rt_keep_largest(self._h, int(connectivity)))

    def flipComponentAt(self, i: int, j: int, k: int, set: int, connectivity: int = 6) -> int:
        """Addition: RayTracerBVH::flipComponentAt -- flips the component of `set` that holds voxel (i, j, k)."""
        return int(load().rtoh_rt_flip_component_at(self._h, int(i), int(j), int(k), int(set), int(connectivity)))

    def distanceField(self, set: int = 1, maxDist: float = float("inf")):
        """Addition: RayTracerBVH::distanceField -- (code, d2 int32 (dimZ, dimY, dimX), summary as a hip.DIST_SUMMARY_DTYPE scalar);
        code is RTO_OK or the refusal's (lastError), and d2 is then None."""
        dims = (C.c_int * 3)()
        load().rtoh_rt_grid(self._h, dims, None)
        d2 = np.empty((dims[2], dims[1], dims[0]), np.int32)
        summary = np.zeros((), DIST_SUMMARY_DTYPE)
        rc = int(load().rtoh_rt_distance_field(self._h, int(set), float(maxDist), d2.ctypes.data, d2.size, summary.ctypes.data))
        return rc, (d2 if rc == 0 else None), summary

    def dilate(self, radius: float) -> int:
        """Addition: RayTracerBVH::dilate -- EMPTY voxels within `radius` of a FILLED one become FILLED; voxels changed, or the
        refusal's code (negative)."""
        return int(load().rtoh_rt_morphology(self._h, 0, float(radius)))

    def erode(self, radius: float) -> int:
        """Addition: RayTracerBVH::erode -- FILLED voxels within `radius` of an EMPTY one become EMPTY."""
        return int(load().rtoh_rt_morphology(self._h, 1, float(radius)))

    def open(self, radius: float) -> int:
        """Addition: RayTracerBVH::open -- erode, then dilate."""
        return int(load().rtoh_rt_morphology(self._h, 2, float(radius)))

    def close(self, radius: float) -> int:
        """Addition: RayTracerBVH::close -- dilate, then erode."""
        return int(load().rtoh_rt_morphology(self._h, 3, float(radius)))

    def thickestPoint(self):
        """Addition: RayTracerBVH::thickestPoint -- (code, None or ((i, j, k), d2, distance in world units)) of the FILLED voxel
        farthest from any EMPTY one."""
        out = (C.c_int64 * 5)()
        dist = C.c_double()
        rc = int(load().rtoh_rt_thickest_point(self._h, out, C.byref(dist)))
        if rc != 0 or not out[0]:
            return rc, None
        return rc, ((int(out[1]), int(out[2]), int(out[3])), int(out[4]), float(dist.value))

    def segmentParts(self, set: int = 1, connectivity: int = 6, ratio: int = 800):
        """Addition: RayTracerBVH::segmentParts -- (code, labels int32 (dimZ, dimY, dimX), summary as a hip.PARTS_SUMMARY_DTYPE
        scalar); code is RTO_OK or the refusal's (lastError), and labels is then None."""
        dims = (C.c_int * 3)()
        load().rtoh_rt_grid(self._h, dims, None)
        labels = np.empty((dims[2], dims[1], dims[0]), np.int32)
        summary = np.zeros((), PARTS_SUMMARY_DTYPE)
        rc = int(load().rtoh_rt_segment_parts(self._h, int(set), int(connectivity), int(ratio), labels.ctypes.data, labels.size, summary.ctypes.data))
        return rc, (labels if rc == 0 else None), summary

    def _partsTable(self, entry, dtype):
        n = C.c_int64()
        rc = int(entry(self._h, None, 0, C.byref(n)))
        if rc != 0:
            return rc, None
        table = np.zeros(n.value, dtype)
        if n.value:
            rc = int(entry(self._h, table.ctypes.data, n.value, C.byref(n)))
        return rc, (table if rc == 0 else None)

    def parts(self):
        """Addition: RayTracerBVH::parts -- (code, the last segmentParts' part table as hip.PART_DTYPE, or None)."""
        return self._partsTable(load().rtoh_rt_parts, PART_DTYPE)

    def necks(self):
        """Addition: RayTracerBVH::necks -- (code, the last segmentParts' neck table as hip.NECK_DTYPE, or None)."""
        return self._partsTable(load().rtoh_rt_necks, NECK_DTYPE)

    def partLabels(self):
        """Addition: RayTracerBVH::partLabels -- (code, the resident part labels int32 (dimZ, dimY, dimX), or None)."""
        dims = (C.c_int * 3)()
        load().rtoh_rt_grid(self._h, dims, None)
        out = np.empty((dims[2], dims[1], dims[0]), np.int32)
        rc = int(load().rtoh_rt_part_labels(self._h, out.ctypes.data, out.size))
        return rc, (out if rc == 0 else None)

    def splitAtNecks(self, set: int = 1, connectivity: int = 6, ratio: int = 800) -> int:
        """Addition: RayTracerBVH::splitAtNecks -- segments afresh and cuts the grid at the necks; voxels flipped, or the refusal's
        code (negative)."""
        return int(load().rtoh_rt_split_at_necks(self._h, int(set), int(connectivity), int(ratio)))

    def thicknessField(self, medium: int = 1, maxRadius: float = 0.0):
        """Addition: RayTracerBVH::thicknessField -- (code, t2 int32 (dimZ, dimY, dimX), summary as a hip.THICK_SUMMARY_DTYPE
        scalar); code is RTO_OK or the refusal's (lastError), and t2 is then None."""
        dims = (C.c_int * 3)()
        load().rtoh_rt_grid(self._h, dims, None)
        t2 = np.empty((dims[2], dims[1], dims[0]), np.int32)
        summary = np.zeros((), THICK_SUMMARY_DTYPE)
        rc = int(load().rtoh_rt_thickness_field(self._h, int(medium), float(maxRadius), t2.ctypes.data, t2.size, summary.ctypes.data))
        return rc, (t2 if rc == 0 else None), summary

    def thinnestPoint(self, medium: int = 1, maxRadius: float = 0.0):
        """Addition: RayTracerBVH::thinnestPoint -- (code, None or ((i, j, k), t2, thin, width in world units)) of the medium voxel
        with the smallest local thickness."""
        out = (C.c_int64 * 6)()
        width = C.c_double()
        rc = int(load().rtoh_rt_thinnest_point(self._h, int(medium), float(maxRadius), out, C.byref(width)))
        if rc != 0 or not out[0]:
            return rc, None
        return rc, ((int(out[1]), int(out[2]), int(out[3])), int(out[4]), int(out[5]), float(width.value))

    def thicknessHistogram(self):
        """Addition: RayTracerBVH::thicknessHistogram -- (code, int64 bins of the last thicknessField, or None)."""
        bins = np.zeros(THICK_MAX_C + 1, np.int64)
        count = C.c_int64()
        rc = int(load().rtoh_rt_thickness_histogram(self._h, bins.ctypes.data, bins.size, C.byref(count)))
        return rc, (bins[:count.value].copy() if rc == 0 else None)

    def measureComponents(self, set: int = 1, connectivity: int = 6):
        """Addition: RayTracerBVH::measureComponents -- labels `set` under `connectivity` and measures every component: (code, table
        as a hip.MEASURE_DTYPE array or None when refused, total as a hip.MEASURE_DTYPE scalar)."""
        total = np.zeros((), MEASURE_DTYPE)
        n = C.c_int64()
        rc = int(load().rtoh_rt_measure_components(self._h, int(set), int(connectivity), None, 0, C.byref(n), total.ctypes.data))
        if rc != 0:
            return rc, None, total
        table = np.zeros(n.value, MEASURE_DTYPE)
        if n.value:
            rc = int(load().rtoh_rt_measure_components(self._h, int(set), int(connectivity), table.ctypes.data, n.value, C.byref(n), total.ctypes.data))
        return rc, (table if rc == 0 else None), total

    def surfaceArea(self, set: int = 1):
        """Addition: RayTracerBVH::surfaceArea -- (code, the exposed faces of the set times voxelSize^2)."""
        area = C.c_double()
        rc = int(load().rtoh_rt_surface_area(self._h, int(set), C.byref(area)))
        return rc, float(area.value)

    def centroid(self, set: int = 1):
        """Addition: RayTracerBVH::centroid -- (code, None or the set's centre of mass (x, y, z) in world units)."""
        out = (C.c_double * 4)()
        rc = int(load().rtoh_rt_centroid(self._h, int(set), out))
        if rc != 0 or not out[0]:
            return rc, None
        return rc, (float(out[1]), float(out[2]), float(out[3]))

    def topology(self, set: int = 1, connectivity: int = 6):
        """Addition: RayTracerBVH::topology -- (code, (pieces, tunnels, cavities))."""
        out = (C.c_int64 * 3)()
        rc = int(load().rtoh_rt_topology(self._h, int(set), int(connectivity), out))
        return rc, (int(out[0]), int(out[1]), int(out[2]))

    def geodesicField(self, seeds, medium: int = 0, connectivity: int = 6, limit: int = 0x7fffffff):
        """Addition: RayTracerBVH::geodesicField -- (code, g int32 (dimZ, dimY, dimX), summary as a hip.GEO_SUMMARY_DTYPE scalar);
        code is RTO_OK or the refusal's (lastError), and g is then None."""
        dims = (C.c_int * 3)()
        load().rtoh_rt_grid(self._h, dims, None)
        s = np.ascontiguousarray(np.asarray(seeds).reshape(-1), np.int64)
        g = np.empty((dims[2], dims[1], dims[0]), np.int32)
        summary = np.zeros((), GEO_SUMMARY_DTYPE)
        rc = int(load().rtoh_rt_geodesic_field(self._h, s.ctypes.data if s.size else None, s.size, int(medium), int(connectivity), int(limit),
                                               g.ctypes.data, g.size, summary.ctypes.data))
        return rc, (g if rc == 0 else None), summary

    def skeletonField(self, set: int = 1, connectivity: int = 26, mode: int = 0, anchors=(), maxPasses: int = 0x7fffffff):
        """Addition: RayTracerBVH::skeletonField -- (code, k int32 (dimZ, dimY, dimX), summary as a hip.SKEL_SUMMARY_DTYPE scalar);
        code is RTO_OK or the refusal's (lastError), and k is then None."""
        dims = (C.c_int * 3)()
        load().rtoh_rt_grid(self._h, dims, None)
        a = np.ascontiguousarray(np.asarray(anchors).reshape(-1), np.int64)
        k = np.empty((dims[2], dims[1], dims[0]), np.int32)
        summary = np.zeros((), SKEL_SUMMARY_DTYPE)
        rc = int(load().rtoh_rt_skeleton_field(self._h, int(set), int(connectivity), int(mode), a.ctypes.data if a.size else None, a.size,
                                               int(maxPasses), k.ctypes.data, k.size, summary.ctypes.data))
        return rc, (k if rc == 0 else None), summary

    def exposureField(self, dirs, weights=None, mode: int = 1, reach: int = 0x7fffffff):
        """Addition: RayTracerBVH::exposureField -- (code, summary as a hip.EXPO_SUMMARY_DTYPE scalar); code is RTO_OK or the
        refusal's (lastError).  The field stays resident: exposure() downloads it."""
        d, w = _expo_args(dirs, weights)
        summary = np.zeros((), EXPO_SUMMARY_DTYPE)
        rc = int(load().rtoh_rt_exposure_field(self._h, None if d is None else d.ctypes.data, None if w is None else w.ctypes.data,
                                               0 if d is None else len(d), int(mode), int(reach), summary.ctypes.data))
        return rc, summary

    def exposure(self):
        """Addition: RayTracerBVH::exposure -- (code, e int32 (dimZ, dimY, dimX) or None when there is no resident field)."""
        dims = (C.c_int * 3)()
        load().rtoh_rt_grid(self._h, dims, None)
        e = np.empty((dims[2], dims[1], dims[0]), np.int32)
        rc = int(load().rtoh_rt_exposure(self._h, e.ctypes.data, e.size))
        return rc, (e if rc == 0 else None)

    def doseField(self, sources, transmit=None, falloff: int = 0, mode: int = 0, reach: int = 0x7fffffff):
        """Addition: RayTracerBVH::doseField -- (code, summary as a hip.DOSE_SUMMARY_DTYPE scalar); code is RTO_OK or the refusal's
        (lastError).  The field stays resident: dose() downloads it, doseCoverage() its per-source counts."""
        s, t = _dose_args(sources, transmit)
        summary = np.zeros((), DOSE_SUMMARY_DTYPE)
        rc = int(load().rtoh_rt_dose_field(self._h, None if s is None else s.ctypes.data, 0 if s is None else len(s), None if t is None else t.ctypes.data,
                                           0 if t is None else len(t), int(falloff), int(mode), int(reach), summary.ctypes.data))
        return rc, summary

    def dose(self):
        """Addition: RayTracerBVH::dose -- (code, e int32 (dimZ, dimY, dimX) or None when there is no resident field)."""
        dims = (C.c_int * 3)()
        load().rtoh_rt_grid(self._h, dims, None)
        e = np.empty((dims[2], dims[1], dims[0]), np.int32)
        rc = int(load().rtoh_rt_dose(self._h, e.ctypes.data, e.size))
        return rc, (e if rc == 0 else None)

    def doseCoverage(self):
        """Addition: RayTracerBVH::doseCoverage -- (code, covered int64 (n) or None when there is no resident field)."""
        out = np.zeros(1024, np.int64)
        count = C.c_int64()
        rc = int(load().rtoh_rt_dose_coverage(self._h, out.ctypes.data, out.size, C.byref(count)))
        return rc, (out[:count.value].copy() if rc == 0 else None)

    def hottestVoxel(self):
        """Addition: RayTracerBVH::hottestVoxel -- (code, (i, j, k) of the resident dose field's peak, the smallest index among
        equals, and its value; None, None when refused)."""
        ijk, value = (C.c_int32 * 3)(), C.c_int32()
        rc = int(load().rtoh_rt_hottest_voxel(self._h, ijk, C.byref(value)))
        return (rc, tuple(ijk), value.value) if rc == 0 else (rc, None, None)

    def thin(self, mode: int = 1, maxPasses: int = 0x7fffffff) -> int:
        """Addition: RayTracerBVH::thin -- replaces the solid by its skeleton; voxels removed, or the refusal's code (negative)."""
        return int(load().rtoh_rt_thin(self._h, int(mode), int(maxPasses)))

    def centreline(self, anchorA: int, anchorB: int):
        """Addition: RayTracerBVH::centreline -- (code, the int64 linear indices left of the free space with both anchors held)."""
        dims = (C.c_int * 3)()
        load().rtoh_rt_grid(self._h, dims, None)
        out = np.empty(max(dims[0] * dims[1] * dims[2], 1), np.int64)
        count = C.c_int64()
        rc = int(load().rtoh_rt_centreline(self._h, int(anchorA), int(anchorB), out.ctypes.data, out.size, C.byref(count)))
        return rc, (out[:count.value].copy() if rc == 0 else None)

    def pathsTo(self, targets, maxLen: int):
        """Addition: RayTracerBVH::pathsTo -- the routes of the last geodesicField: (code, rows (n, maxLen) int64 with -1 behind each
        path, lengths (n,) int64 with -1 for a target not reached)."""
        t = np.ascontiguousarray(np.asarray(targets).reshape(-1), np.int64)
        rows = np.empty((t.size, max(int(maxLen), 0)), np.int64)
        lengths = np.empty(t.size, np.int64)
        rc = int(load().rtoh_rt_paths_to(self._h, t.ctypes.data if t.size else None, t.size, int(maxLen), rows.ctypes.data if rows.size else None,
                                         lengths.ctypes.data))
        return rc, rows, lengths

    def floodFrom(self, seeds, medium: int = 0, connectivity: int = 6, limit: int = 0x7fffffff) -> int:
        """Addition: RayTracerBVH::floodFrom -- flips every voxel of `medium` within `limit` of the seeds along paths inside the
        medium; voxels flipped, or the refusal's code (negative)."""
        s = np.ascontiguousarray(np.asarray(seeds).reshape(-1), np.int64)
        return int(load().rtoh_rt_flood_from(self._h, s.ctypes.data if s.size else None, s.size, int(medium), int(connectivity), int(limit)))

    def farthestPoint(self, seeds, medium: int = 0, connectivity: int = 6):
        """Addition: RayTracerBVH::farthestPoint -- (code, None or ((i, j, k), voxel, g, reached)) of the reached voxel farthest
        from the seeds along paths inside the medium."""
        s = np.ascontiguousarray(np.asarray(seeds).reshape(-1), np.int64)
        out = (C.c_int64 * 7)()
        rc = int(load().rtoh_rt_farthest_point(self._h, s.ctypes.data if s.size else None, s.size, int(medium), int(connectivity), out))
        if rc != 0 or not out[0]:
            return rc, None
        return rc, ((int(out[1]), int(out[2]), int(out[3])), int(out[4]), int(out[5]), int(out[6]))

    def locate(self, points):
        """Addition: RayTracerBVH::locate -- the leaf that holds each of the (n, 3) points: (code, hip.POINT_HIT_DTYPE records).
        code is RTO_OK or the refusal's (lastError)."""
        p = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
        hits = np.zeros(len(p), POINT_HIT_DTYPE)
        rc = load().rtoh_rt_locate(self._h, p.ctypes.data, len(p), hits.ctypes.data)
        return int(rc), hits

    def census(self, brushes):
        """Addition: RayTracerBVH::census -- what each hip.BRUSH_DTYPE brush covers (the op is ignored): (code, hip.REGION_DTYPE
        records)."""
        b = np.asarray(brushes, BRUSH_DTYPE).reshape(-1)
        f = np.ascontiguousarray(np.concatenate([b["centre"], b["extent"]], 1), dtype=np.float32)
        shapes = np.ascontiguousarray(b["shape"], dtype=np.int32)
        out = np.zeros(len(b), REGION_DTYPE)
        rc = load().rtoh_rt_census(self._h, f.ctypes.data, shapes.ctypes.data, len(b), out.ctypes.data)
        return int(rc), out

    def nearestSolid(self, points, maxDist: float = float("inf")):
        """Addition: RayTracerBVH::nearestSolid -- the nearest solid leaf to each of the (n, 3) points within maxDist: (code,
        hip.NEAREST_DTYPE records, distances in world units as float64, inf where there is none)."""
        p = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
        out = np.zeros(len(p), NEAREST_DTYPE)
        dist = np.zeros(len(p), np.float64)
        rc = load().rtoh_rt_nearest_solid(self._h, p.ctypes.data, len(p), _f(maxDist), out.ctypes.data, dist.ctypes.data)
        return int(rc), out, dist

    def loadMesh(self, xyz, tris, voxelSize, recenterPasses=0, triangles=False) -> bool:
        """Addition: RayTracerBVH::loadMesh -- rows (n, 3) and faces (m, 3) of row indices voxelized on every GPU (AUTO grid),
        recentred recenterPasses times, the octree built there.  False on an error (lastError)."""
        v = np.ascontiguousarray(np.asarray(xyz, np.float64).reshape(-1, 3))
        t = np.ascontiguousarray(np.asarray(tris, np.int32).reshape(-1, 3))
        return bool(load().rtoh_rt_load_mesh(self._h, v.ctypes.data, len(v), t.ctypes.data, len(t), _f(voxelSize), int(recenterPasses),
                                             1 if triangles else 0))

    def extractMesh(self, kind: int, camera: "Camera | None" = None, aspect: float = 1.0, extraMargin: float = 50.0, planes=None) -> np.ndarray:
        """Addition: RayTracerBVH::extractMesh -- the list renderOctree returns for this camera (kind 0: MarchingCubesRenderer, 1:
        VoxelCubeRenderer), made on the GPU; camera None: extractMeshPlanes over `planes` (None: nothing
        culled).  (n, 18) float32; empty with lastError set on an error."""
        pl = None if planes is None else np.ascontiguousarray(np.asarray(planes, np.float32).reshape(24))
        n = C.c_int64(0)
        lst = load().rtoh_rt_extract_mesh(self._h, int(kind), camera._h if camera is not None else None, _f(aspect),
                                          None if pl is None else pl.ctypes.data, _f(extraMargin), C.byref(n))
        out = np.zeros((n.value, 18), np.float32)
        load().rtoh_tris_take(lst, out.ctypes.data)                # one extraction: copied out and freed
        return out

    def isoSurface(self, source: int, level: float, outside: float = 0.0, pad: bool = True, volume=None) -> np.ndarray:
        """Addition: RayTracerBVH::isoSurface -- marching cubes of a voxel field at `level`, made on the GPU (DESIGN.md section
        30); volume: the (dimZ, dimY, dimX) int32 array of FIELD_CALLER.  (n, 18) float32; empty with lastError set on an error."""
        vol = None if volume is None else np.ascontiguousarray(np.asarray(volume, np.int32))
        n = C.c_int64(0)
        lst = load().rtoh_rt_iso_surface(self._h, int(source), _f(level), _f(outside), 1 if pad else 0,
                                         None if vol is None else vol.ctypes.data, C.byref(n))
        out = np.zeros((n.value, 18), np.float32)
        load().rtoh_tris_take(lst, out.ctypes.data)
        return out

    def dualContour(self, params: DcParams):
        """Addition: RayTracerBVH::dualContour -- dual contouring of the resident grid, made on the GPU.
        ((n, 18) float32, tri_cell (n,) int32, DcSummary); empty with lastError set on an error."""
        n, summary = C.c_int64(0), DcSummary()
        lst = load().rtoh_rt_dual_contour(self._h, C.byref(params), C.byref(summary), C.byref(n))
        out = np.zeros((n.value, 18), np.float32)
        cell = np.zeros(n.value, np.int32)
        load().rtoh_iso_take(lst, out.ctypes.data, cell.ctypes.data)
        return out, cell, summary

    def dualVertices(self, voxels) -> np.ndarray:
        """Addition: RayTracerBVH::dualVertices -- the vertex of each voxel (linear indices): a DUAL_VERTEX_DTYPE array, or None
        with lastError set on an error."""
        v = np.ascontiguousarray(np.asarray(voxels, np.int64).reshape(-1))
        out = np.zeros(len(v), DUAL_VERTEX_DTYPE)
        ok = load().rtoh_rt_dual_vertices(self._h, v.ctypes.data, len(v), out.ctypes.data)
        return out if ok else None

    def offsetSurface(self, distanceInVoxels: float) -> np.ndarray:
        """Addition: RayTracerBVH::offsetSurface -- the surface at that distance from the solids (the distance field to the
        solids contoured at its square).  (n, 18) float32."""
        n = C.c_int64(0)
        lst = load().rtoh_rt_iso_surface(self._h, -1, _f(distanceInVoxels), 0.0, 1, None, C.byref(n))
        out = np.zeros((n.value, 18), np.float32)
        load().rtoh_tris_take(lst, out.ctypes.data)
        return out

    def grid(self) -> np.ndarray:
        """Addition: RayTracerBVH::grid -- the current voxels, uint8 (dimZ, dimY, dimX), every edit applied."""
        dims = (C.c_int * 3)()
        load().rtoh_rt_grid(self._h, dims, None)
        out = np.empty((dims[2], dims[1], dims[0]), np.uint8)
        load().rtoh_rt_grid(self._h, dims, out.ctypes.data)
        return out

    def finish(self):
        """Wait for the GPU(s): the counterpart of glFinish for timing loops (renders are asynchronous)."""
        load().rtoh_rt_finish(self._h)

    @property
    def numNodes(self) -> int:
        return load().rtoh_rt_num_nodes(self._h)

    @property
    def lastError(self) -> str:
        return load().rtoh_rt_last_error(self._h).decode()

    @property
    def context_handle(self):
        """The rto_context* the C++ object owns (NULL until ensureComputeInitialized() succeeded)."""
        return load().rtoh_rt_context(self._h)


# ---- small math doors used by tests -------------------------------------------------------------
def mat4_inverse(m):
    out = np.zeros(16, np.float32)
    load().rtoh_mat4_inverse(np.ascontiguousarray(m, dtype=np.float32).reshape(16), out)
    return out


def mat4_mul(a, b):
    out = np.zeros(16, np.float32)
    load().rtoh_mat4_mul(np.ascontiguousarray(a, dtype=np.float32).reshape(16),
                         np.ascontiguousarray(b, dtype=np.float32).reshape(16), out)
    return out


def perspective(fovy_rad, aspect, zn, zf):
    out = np.zeros(16, np.float32)
    load().rtoh_perspective(_f(fovy_rad), _f(aspect), _f(zn), _f(zf), out)
    return out


def radians(deg):
    return np.float32(load().rtoh_radians(_f(deg)))


def frustum_test(vp, mins, maxs, margin):
    mins = np.ascontiguousarray(mins, dtype=np.float32).reshape(-1)
    maxs = np.ascontiguousarray(maxs, dtype=np.float32).reshape(-1)
    out = np.zeros(len(mins) // 3, np.int32)
    load().rtoh_frustum_test(np.ascontiguousarray(vp, dtype=np.float32).reshape(16), mins, maxs, len(out), _f(margin),
                             out.ctypes.data)
    return out
