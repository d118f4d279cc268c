// RayTracerBVH.cpp -- host side of the drop-in class; see RayTracerBVH.h.
// Call structure follows 453-skeleton/RayTracerBVH.cpp:393-892; every GL call there maps to one
// rto_* call here (table in INTEGRATION.md).
#include "RayTracerBVH.h"

#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

namespace {

// The C ABI, resolved at run time so this translation unit builds with a plain C++ compiler.
struct HipApi {
    void* handle = nullptr;
    decltype(&rto_create) create = nullptr;
    decltype(&rto_destroy) destroy = nullptr;
    decltype(&rto_last_error) last_error = nullptr;
    decltype(&rto_upload_octree) upload_octree = nullptr;
    decltype(&rto_build_octree) build_octree = nullptr;
    decltype(&rto_octree_info_get) octree_info = nullptr;
    decltype(&rto_update_frustum) update_frustum = nullptr;
    decltype(&rto_render_host) render_host = nullptr;
    decltype(&rto_upload_leaf_triangles) upload_leaf_triangles = nullptr;
    decltype(&rto_build_leaf_triangles) build_leaf_triangles = nullptr;
    decltype(&rto_render_resident) render_resident = nullptr;
    decltype(&rto_download_resident) download_resident = nullptr;
    decltype(&rto_synchronize) synchronize = nullptr;
    decltype(&rto_timing_begin) timing_begin = nullptr;
    decltype(&rto_render_triangles_host) render_triangles_host = nullptr;
    decltype(&rto_comm_create_all) comm_create_all = nullptr;
    decltype(&rto_comm_destroy) comm_destroy = nullptr;
    decltype(&rto_comm_last_error) comm_last_error = nullptr;
    decltype(&rto_comm_render_resident_all) comm_render_resident_all = nullptr;
    decltype(&rto_query_rays_host) query_rays_host = nullptr;
    decltype(&rto_query_pixels_host) query_pixels_host = nullptr;
    decltype(&rto_query_spans_host) query_spans_host = nullptr;
    decltype(&rto_query_span_pixels_host) query_span_pixels_host = nullptr;
    decltype(&rto_query_triangles_host) query_triangles_host = nullptr;
    decltype(&rto_query_triangle_pixels_host) query_triangle_pixels_host = nullptr;
    decltype(&rto_edit_voxels) edit_voxels = nullptr;
    decltype(&rto_download_voxels) download_voxels = nullptr;
    decltype(&rto_download_leaf_triangles) download_leaf_triangles = nullptr;
    decltype(&rto_download_nodes) download_nodes = nullptr;
    decltype(&rto_render_lit_host) render_lit_host = nullptr;
    decltype(&rto_render_lit_triangles_host) render_lit_triangles_host = nullptr;
    decltype(&rto_voxelize_mesh) voxelize_mesh = nullptr;
    decltype(&rto_frustum_planes) frustum_planes = nullptr;
    decltype(&rto_extract_mesh) extract_mesh = nullptr;
    decltype(&rto_download_mesh) download_mesh = nullptr;
    decltype(&rto_extract_isosurface_host) extract_isosurface_host = nullptr;
    decltype(&rto_download_isosurface) download_isosurface = nullptr;
    decltype(&rto_extract_dual_contour) extract_dual_contour = nullptr;
    decltype(&rto_download_dual_contour) download_dual_contour = nullptr;
    decltype(&rto_query_dual_vertices_host) query_dual_vertices_host = nullptr;
    decltype(&rto_query_points_host) query_points_host = nullptr;
    decltype(&rto_query_regions_host) query_regions_host = nullptr;
    decltype(&rto_query_nearest_host) query_nearest_host = nullptr;
    decltype(&rto_scene_bounds_get) scene_bounds_get = nullptr;
    decltype(&rto_label_components) label_components = nullptr;
    decltype(&rto_download_components) download_components = nullptr;
    decltype(&rto_download_labels) download_labels = nullptr;
    decltype(&rto_edit_components) edit_components = nullptr;
    decltype(&rto_distance_field) distance_field = nullptr;
    decltype(&rto_download_distance) download_distance = nullptr;
    decltype(&rto_edit_morphology) edit_morphology = nullptr;
    decltype(&rto_geodesic_field) geodesic_field = nullptr;
    decltype(&rto_download_geodesic) download_geodesic = nullptr;
    decltype(&rto_geodesic_paths) geodesic_paths = nullptr;
    decltype(&rto_edit_geodesic) edit_geodesic = nullptr;
    decltype(&rto_skeleton_field) skeleton_field = nullptr;
    decltype(&rto_download_skeleton) download_skeleton = nullptr;
    decltype(&rto_edit_skeleton) edit_skeleton = nullptr;
    decltype(&rto_exposure_field) exposure_field = nullptr;
    decltype(&rto_download_exposure) download_exposure = nullptr;
    decltype(&rto_dose_field) dose_field = nullptr;
    decltype(&rto_download_dose) download_dose = nullptr;
    decltype(&rto_download_dose_coverage) download_dose_coverage = nullptr;
    decltype(&rto_thickness_field) thickness_field = nullptr;
    decltype(&rto_download_thickness) download_thickness = nullptr;
    decltype(&rto_thickness_histogram) thickness_histogram = nullptr;
    decltype(&rto_measure_components) measure_components = nullptr;
    decltype(&rto_download_measures) download_measures = nullptr;
    decltype(&rto_segment_parts) segment_parts = nullptr;
    decltype(&rto_download_part_labels) download_part_labels = nullptr;
    decltype(&rto_download_parts) download_parts = nullptr;
    decltype(&rto_download_necks) download_necks = nullptr;
    decltype(&rto_edit_parts) edit_parts = nullptr;
    decltype(&rto_render_field_host) render_field_host = nullptr;
    decltype(&rto_project_field_host) project_field_host = nullptr;
    decltype(&rto_composite_field_host) composite_field_host = nullptr;
    std::string error;

    bool load() {
        if (handle) return true;
        std::vector<std::string> candidates;
        if (const char* env = std::getenv("RTO_HIP_LIB")) { if (*env) candidates.emplace_back(env); }      // set but empty: as if unset
        Dl_info info;
        if (dladdr(reinterpret_cast<void*>(&anchor), &info) && info.dli_fname) {   // next to this library
            std::string dir(info.dli_fname);
            const size_t slash = dir.find_last_of('/');
            dir = slash == std::string::npos ? "." : dir.substr(0, slash);
            candidates.push_back(dir + "/librto_hip.so");
        }
        candidates.emplace_back("librto_hip.so");
        for (const std::string& path : candidates) {
            handle = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
            if (handle) break;
            error = dlerror();
        }
        if (!handle) return false;
        bool ok = true;
        auto sym = [&](const char* name) {
            void* p = dlsym(handle, name);
            if (!p) { ok = false; error = std::string("missing symbol ") + name; }
            return p;
        };
        create = reinterpret_cast<decltype(create)>(sym("rto_create"));
        destroy = reinterpret_cast<decltype(destroy)>(sym("rto_destroy"));
        last_error = reinterpret_cast<decltype(last_error)>(sym("rto_last_error"));
        upload_octree = reinterpret_cast<decltype(upload_octree)>(sym("rto_upload_octree"));
        build_octree = reinterpret_cast<decltype(build_octree)>(sym("rto_build_octree"));
        octree_info = reinterpret_cast<decltype(octree_info)>(sym("rto_octree_info_get"));
        update_frustum = reinterpret_cast<decltype(update_frustum)>(sym("rto_update_frustum"));
        render_host = reinterpret_cast<decltype(render_host)>(sym("rto_render_host"));
        upload_leaf_triangles = reinterpret_cast<decltype(upload_leaf_triangles)>(sym("rto_upload_leaf_triangles"));
        build_leaf_triangles = reinterpret_cast<decltype(build_leaf_triangles)>(sym("rto_build_leaf_triangles"));
        render_resident = reinterpret_cast<decltype(render_resident)>(sym("rto_render_resident"));
        download_resident = reinterpret_cast<decltype(download_resident)>(sym("rto_download_resident"));
        synchronize = reinterpret_cast<decltype(synchronize)>(sym("rto_synchronize"));
        timing_begin = reinterpret_cast<decltype(timing_begin)>(sym("rto_timing_begin"));
        render_triangles_host = reinterpret_cast<decltype(render_triangles_host)>(sym("rto_render_triangles_host"));
        comm_create_all = reinterpret_cast<decltype(comm_create_all)>(sym("rto_comm_create_all"));
        comm_destroy = reinterpret_cast<decltype(comm_destroy)>(sym("rto_comm_destroy"));
        comm_last_error = reinterpret_cast<decltype(comm_last_error)>(sym("rto_comm_last_error"));
        comm_render_resident_all = reinterpret_cast<decltype(comm_render_resident_all)>(sym("rto_comm_render_resident_all"));
        query_rays_host = reinterpret_cast<decltype(query_rays_host)>(sym("rto_query_rays_host"));
        query_pixels_host = reinterpret_cast<decltype(query_pixels_host)>(sym("rto_query_pixels_host"));
        query_spans_host = reinterpret_cast<decltype(query_spans_host)>(sym("rto_query_spans_host"));
        query_span_pixels_host = reinterpret_cast<decltype(query_span_pixels_host)>(sym("rto_query_span_pixels_host"));
        query_triangles_host = reinterpret_cast<decltype(query_triangles_host)>(sym("rto_query_triangles_host"));
        query_triangle_pixels_host = reinterpret_cast<decltype(query_triangle_pixels_host)>(sym("rto_query_triangle_pixels_host"));
        edit_voxels = reinterpret_cast<decltype(edit_voxels)>(sym("rto_edit_voxels"));
        download_voxels = reinterpret_cast<decltype(download_voxels)>(sym("rto_download_voxels"));
        download_leaf_triangles = reinterpret_cast<decltype(download_leaf_triangles)>(sym("rto_download_leaf_triangles"));
        download_nodes = reinterpret_cast<decltype(download_nodes)>(sym("rto_download_nodes"));
        render_lit_host = reinterpret_cast<decltype(render_lit_host)>(sym("rto_render_lit_host"));
        render_lit_triangles_host = reinterpret_cast<decltype(render_lit_triangles_host)>(sym("rto_render_lit_triangles_host"));
        voxelize_mesh = reinterpret_cast<decltype(voxelize_mesh)>(sym("rto_voxelize_mesh"));
        frustum_planes = reinterpret_cast<decltype(frustum_planes)>(sym("rto_frustum_planes"));
        extract_mesh = reinterpret_cast<decltype(extract_mesh)>(sym("rto_extract_mesh"));
        download_mesh = reinterpret_cast<decltype(download_mesh)>(sym("rto_download_mesh"));
        extract_isosurface_host = reinterpret_cast<decltype(extract_isosurface_host)>(sym("rto_extract_isosurface_host"));
        download_isosurface = reinterpret_cast<decltype(download_isosurface)>(sym("rto_download_isosurface"));
        extract_dual_contour = reinterpret_cast<decltype(extract_dual_contour)>(sym("rto_extract_dual_contour"));
        download_dual_contour = reinterpret_cast<decltype(download_dual_contour)>(sym("rto_download_dual_contour"));
        query_dual_vertices_host = reinterpret_cast<decltype(query_dual_vertices_host)>(sym("rto_query_dual_vertices_host"));
        query_points_host = reinterpret_cast<decltype(query_points_host)>(sym("rto_query_points_host"));
        query_regions_host = reinterpret_cast<decltype(query_regions_host)>(sym("rto_query_regions_host"));
        query_nearest_host = reinterpret_cast<decltype(query_nearest_host)>(sym("rto_query_nearest_host"));
        scene_bounds_get = reinterpret_cast<decltype(scene_bounds_get)>(sym("rto_scene_bounds_get"));
        label_components = reinterpret_cast<decltype(label_components)>(sym("rto_label_components"));
        download_components = reinterpret_cast<decltype(download_components)>(sym("rto_download_components"));
        download_labels = reinterpret_cast<decltype(download_labels)>(sym("rto_download_labels"));
        edit_components = reinterpret_cast<decltype(edit_components)>(sym("rto_edit_components"));
        distance_field = reinterpret_cast<decltype(distance_field)>(sym("rto_distance_field"));
        download_distance = reinterpret_cast<decltype(download_distance)>(sym("rto_download_distance"));
        edit_morphology = reinterpret_cast<decltype(edit_morphology)>(sym("rto_edit_morphology"));
        geodesic_field = reinterpret_cast<decltype(geodesic_field)>(sym("rto_geodesic_field"));
        download_geodesic = reinterpret_cast<decltype(download_geodesic)>(sym("rto_download_geodesic"));
        geodesic_paths = reinterpret_cast<decltype(geodesic_paths)>(sym("rto_geodesic_paths"));
        edit_geodesic = reinterpret_cast<decltype(edit_geodesic)>(sym("rto_edit_geodesic"));
        skeleton_field = reinterpret_cast<decltype(skeleton_field)>(sym("rto_skeleton_field"));
        download_skeleton = reinterpret_cast<decltype(download_skeleton)>(sym("rto_download_skeleton"));
        edit_skeleton = reinterpret_cast<decltype(edit_skeleton)>(sym("rto_edit_skeleton"));
        exposure_field = reinterpret_cast<decltype(exposure_field)>(sym("rto_exposure_field"));
        download_exposure = reinterpret_cast<decltype(download_exposure)>(sym("rto_download_exposure"));
        dose_field = reinterpret_cast<decltype(dose_field)>(sym("rto_dose_field"));
        download_dose = reinterpret_cast<decltype(download_dose)>(sym("rto_download_dose"));
        download_dose_coverage = reinterpret_cast<decltype(download_dose_coverage)>(sym("rto_download_dose_coverage"));
        thickness_field = reinterpret_cast<decltype(thickness_field)>(sym("rto_thickness_field"));
        download_thickness = reinterpret_cast<decltype(download_thickness)>(sym("rto_download_thickness"));
        thickness_histogram = reinterpret_cast<decltype(thickness_histogram)>(sym("rto_thickness_histogram"));
        measure_components = reinterpret_cast<decltype(measure_components)>(sym("rto_measure_components"));
        download_measures = reinterpret_cast<decltype(download_measures)>(sym("rto_download_measures"));
        segment_parts = reinterpret_cast<decltype(segment_parts)>(sym("rto_segment_parts"));
        download_part_labels = reinterpret_cast<decltype(download_part_labels)>(sym("rto_download_part_labels"));
        download_parts = reinterpret_cast<decltype(download_parts)>(sym("rto_download_parts"));
        download_necks = reinterpret_cast<decltype(download_necks)>(sym("rto_download_necks"));
        edit_parts = reinterpret_cast<decltype(edit_parts)>(sym("rto_edit_parts"));
        render_field_host = reinterpret_cast<decltype(render_field_host)>(sym("rto_render_field_host"));
        project_field_host = reinterpret_cast<decltype(project_field_host)>(sym("rto_project_field_host"));
        composite_field_host = reinterpret_cast<decltype(composite_field_host)>(sym("rto_composite_field_host"));
        if (!ok) { dlclose(handle); handle = nullptr; }
        return ok;
    }
    static void anchor() {}
};

HipApi& api() {
    static HipApi a;
    return a;
}

}  // namespace

RayTracerBVH::RayTracerBVH()
    : m_octreeRoot(nullptr), m_numNodes(0), m_computeInited(false), m_computeOk(false),
      m_frustumCullingEnabled(true), m_device(0), m_ctx(nullptr), m_frameW(0), m_frameH(0) {}

RayTracerBVH::~RayTracerBVH() {
    for (rto_comm* m : m_comms) if (m) api().comm_destroy(m);
    for (rto_context* c : m_ctxs) if (c) api().destroy(c);
}

// Runs `call(ctx)` (an rto_* call returning RTO_OK or an error code) on every GPU's context.
template <class F> bool RayTracerBVH::forEachContext(F&& call, const char* what) {
    for (rto_context* c : m_ctxs) {
        if (call(c) != RTO_OK) {
            m_lastError = api().last_error(c);
            std::cerr << "[RayTracerBVH] " << what << " failed: " << m_lastError << std::endl;
            return false;
        }
    }
    return true;
}

// One frame into the (first GPU's) resident framebuffer: a plain render, or the split over all GPUs + one gather.
bool RayTracerBVH::renderFrame(const rto_frame& f, int mode) {
    if (m_comms.empty()) {
        if (api().render_resident(m_ctx, &f, mode) == RTO_OK) return true;
        m_lastError = api().last_error(m_ctx);
        return false;
    }
    if (api().comm_render_resident_all(m_comms.data(), (int)m_comms.size(), &f, mode) == RTO_OK) return true;
    m_lastError = api().comm_last_error(m_comms[0]);
    return false;
}

std::vector<GPUNodes> RayTracerBVH::flatten(const OctreeNode* root) {
    // Breadth-first; a child receives the next free index at the moment its parent is dequeued, so the 8
    // children of an internal node are consecutive and the root is 0 (RayTracerBVH.cpp:443-490).
    std::vector<GPUNodes> flat;
    if (!root) return flat;
    std::vector<const OctreeNode*> order;
    order.push_back(root);
    for (size_t head = 0; head < order.size(); head++) {
        const OctreeNode* nd = order[head];
        GPUNodes g;
        g.x = nd->x; g.y = nd->y; g.z = nd->z; g.size = nd->size;
        g.isLeaf = nd->isLeaf ? 1 : 0;
        g.isSolid = nd->isSolid ? 1 : 0;
        g.isUniform = nd->isUniform ? 1 : 0;
        for (int& c : g.child) c = -1;
        if (!nd->isLeaf)
            for (int i = 0; i < 8; i++)
                if (const OctreeNode* c = nd->children[i]) {
                    g.child[i] = static_cast<int>(order.size());
                    order.push_back(c);
                }
        flat.push_back(g);
    }
    return flat;
}

void RayTracerBVH::setOctree(OctreeNode* root, const VoxelGrid& grid) {
    m_octreeRoot = root;
    m_grid = grid;                      // the reference copies the grid too (RayTracerBVH.cpp:433)
    m_gridStale = false;
    m_flatNodes.clear();
    m_numNodes = 0;
    if (!root) return;                  // :439
    m_flatNodes = flatten(root);
    m_numNodes = static_cast<int>(m_flatNodes.size());
    if (!m_ctx) return;                 // uploaded by ensureComputeInitialized() once the device exists
    const float gridMin[3] = { m_grid.minX, m_grid.minY, m_grid.minZ };
    if (!forEachContext([&](rto_context* c) {
            return api().upload_octree(c, reinterpret_cast<const rto_node*>(m_flatNodes.data()), m_numNodes, gridMin, m_grid.voxelSize);
        }, "octree upload"))
        m_computeOk = false;
}

void RayTracerBVH::setOctreeFromGrid(const VoxelGrid& grid) {
    m_octreeRoot = nullptr;
    m_grid = grid;
    m_gridStale = false;
    m_flatNodes.clear();
    m_numNodes = 0;
    if (!m_computeInited) ensureComputeInitialized();
    if (!m_computeOk || grid.dimX <= 0 || grid.dimY <= 0 || grid.dimZ <= 0) return;
    const float gridMin[3] = { grid.minX, grid.minY, grid.minZ };
    static_assert(sizeof(VoxelState) == 1, "VoxelGrid.data is one byte per voxel");
    if (!forEachContext([&](rto_context* c) {
            return api().build_octree(c, reinterpret_cast<const uint8_t*>(grid.data.data()), grid.dimX, grid.dimY, grid.dimZ, gridMin, grid.voxelSize);
        }, "GPU octree build"))
        return;
    rto_octree_info info;
    if (api().octree_info(m_ctx, &info) == RTO_OK) m_numNodes = static_cast<int>(info.num_nodes);
}

void RayTracerBVH::ensureComputeInitialized() {
    if (m_computeInited) return;
    m_computeInited = true;
    if (!api().load()) {
        m_lastError = "cannot load librto_hip.so: " + api().error;
        std::cerr << "[RayTracerBVH] " << m_lastError << std::endl;
        return;
    }
    for (int i = 0; i < m_numDevices; i++) {
        rto_context* c = nullptr;
        if (api().create(m_device + i, &c) != RTO_OK) {
            m_lastError = api().last_error(nullptr);
            std::cerr << "[RayTracerBVH] " << m_lastError << std::endl;
            for (rto_context* d : m_ctxs) api().destroy(d);
            m_ctxs.clear();
            m_ctx = nullptr;
            return;
        }
        m_ctxs.push_back(c);
        api().timing_begin(c, -1);                     // nobody reads kernel timings through this class: no event pair per launch
    }
    m_ctx = m_ctxs[0];
    if (m_numDevices > 1) {
        m_comms.assign((size_t)m_numDevices, nullptr);
        if (api().comm_create_all(m_ctxs.data(), m_numDevices, m_bandRows, m_comms.data()) != RTO_OK) {
            m_lastError = api().last_error(m_ctx);
            std::cerr << "[RayTracerBVH] " << m_lastError << std::endl;
            m_comms.clear();
            return;                                    // m_computeOk stays false: no silent single-GPU fallback
        }
    }
    m_computeOk = true;
    if (m_numNodes > 0 && !m_flatNodes.empty()) {   // setOctree() came first
        const float gridMin[3] = { m_grid.minX, m_grid.minY, m_grid.minZ };
        if (!forEachContext([&](rto_context* c) {
                return api().upload_octree(c, reinterpret_cast<const rto_node*>(m_flatNodes.data()), m_numNodes, gridMin, m_grid.voxelSize);
            }, "octree upload"))
            m_computeOk = false;
    }
}

// The rto_frame of a camera and a frame size: what every render, pick and lit call hands to the C ABI.
static rto_frame frame_of(const Camera& camera, int width, int height, float aspect, float fovDeg) {
    rto_frame f;
    const auto view = camera.getView();            // rtmath::mat4 or glm::mat4: both column-major, m[col][row]
    std::memcpy(f.view, &view[0][0], sizeof f.view);
    const auto pos = camera.getPos();
    f.cam_pos[0] = pos.x; f.cam_pos[1] = pos.y; f.cam_pos[2] = pos.z;
    f.aspect = aspect; f.fov_deg = fovDeg; f.width = width; f.height = height;
    return f;
}

bool RayTracerBVH::render(const Camera& camera, int width, int height, float aspect, float fovDeg) {
    const rto_frame f = frame_of(camera, width, height, aspect, fovDeg);
    if (width <= 0 || height <= 0) return false;
    // like the reference's texture, the frame stays on the GPU (asynchronous); framebuffer() fetches it on demand
    m_frameW = m_frameH = 0; m_frameStale = false;
    if (!renderFrame(f, RTO_RESIDENT_OCTREE)) {
        std::cerr << "[RayTracerBVH] render failed: " << m_lastError << std::endl;
        m_frame.clear();
        return false;
    }
    m_frameW = width; m_frameH = height; m_frameStale = true;
    return true;
}

void RayTracerBVH::buildLeafTriangles() {
    if (!m_computeInited || !m_computeOk) {
        std::cerr << "[RayTracerBVH] Compute pipeline not initialized or failed.\n";
        return;
    }
    if (m_numNodes <= 0) return;
    // the triangles MarchingCubesRenderer::render would emit per leaf, built in HBM from the grid given to setOctree()
    // (after setOctreeFromGrid the voxels are already resident: NULL)
    static_assert(sizeof(VoxelState) == 1, "VoxelState is a byte upstream (S/OctreeVoxel.h:10-13)");
    const uint8_t* vox = m_flatNodes.empty() ? nullptr : reinterpret_cast<const uint8_t*>(m_grid.data.data());
    forEachContext([&](rto_context* c) { return api().build_leaf_triangles(c, vox, m_grid.dimX, m_grid.dimY, m_grid.dimZ); }, "leaf-triangle build");
}

#ifndef RTO_REFERENCE_HEADERS
// The same buffer made by this repo's host builder (localMC per leaf) and uploaded: the cross-check of the GPU build.
void RayTracerBVH::buildLeafTrianglesOnHost() {
    if (!m_computeInited || !m_computeOk) {
        std::cerr << "[RayTracerBVH] Compute pipeline not initialized or failed.\n";
        return;
    }
    if (m_numNodes <= 0) return;
    // the resident array: setOctree()'s, or (after setOctreeFromGrid / editVoxels) the one the GPU built
    std::vector<GPUNodes> downloaded;
    if (m_flatNodes.empty()) {
        int64_t n = 0;
        if (api().download_nodes(m_ctx, nullptr, 0, &n) != RTO_OK) { m_lastError = api().last_error(m_ctx); return; }
        downloaded.resize((size_t)n);
        if (api().download_nodes(m_ctx, reinterpret_cast<rto_node*>(downloaded.data()), n, &n) != RTO_OK) { m_lastError = api().last_error(m_ctx); return; }
    }
    const std::vector<GPUNodes>& nodes = m_flatNodes.empty() ? downloaded : m_flatNodes;
    std::vector<float> tris;
    std::vector<int32_t> off;
    ::buildLeafTriangles(grid(), GPUNodesView{ reinterpret_cast<const int32_t*>(nodes.data()), (int64_t)nodes.size() }, tris, off);
    forEachContext([&](rto_context* c) { return api().upload_leaf_triangles(c, tris.data(), (int64_t)(tris.size() / 12), off.data()); }, "triangle upload");
}
#endif

void RayTracerBVH::renderSceneTriangles(const Camera& camera, int width, int height, float aspect, float fovDeg, bool shadow) {
    if (!m_computeInited || !m_computeOk) {
        std::cerr << "[RayTracerBVH] Compute pipeline not initialized or failed.\n";
        return;
    }
    if (m_numNodes <= 0 || width <= 0 || height <= 0) return;
    const rto_frame f = frame_of(camera, width, height, aspect, fovDeg);
    m_frameW = m_frameH = 0; m_frameStale = false;
    if (!renderFrame(f, shadow ? RTO_RESIDENT_TRIANGLES_SHADOW : RTO_RESIDENT_TRIANGLES)) {
        std::cerr << "[RayTracerBVH] render failed: " << m_lastError << std::endl;
        m_frame.clear();
        return;
    }
    m_frameW = width; m_frameH = height; m_frameStale = true;
}

void RayTracerBVH::renderSceneLit(const Camera& camera, int width, int height, float aspect, float fovDeg, const Lighting& lighting) {
    renderLit(camera, width, height, aspect, fovDeg, lighting, false);
}

void RayTracerBVH::renderSurfaceLit(const Camera& camera, int width, int height, float aspect, float fovDeg, const Lighting& lighting) {
    renderLit(camera, width, height, aspect, fovDeg, lighting, true);
}

void RayTracerBVH::renderLit(const Camera& camera, int width, int height, float aspect, float fovDeg, const Lighting& lighting, bool surface) {
    if (!m_computeInited || !m_computeOk) {
        std::cerr << "[RayTracerBVH] Compute pipeline not initialized or failed.\n";
        return;
    }
    if (m_numNodes <= 0 || width <= 0 || height <= 0) return;
    const rto_frame f = frame_of(camera, width, height, aspect, fovDeg);
    rto_lighting L;
    L.light_dir[0] = lighting.lightDir.x; L.light_dir[1] = lighting.lightDir.y; L.light_dir[2] = lighting.lightDir.z;
    L.shadow = lighting.shadow ? 1 : 0;
    L.ao_samples = lighting.aoSamples;
    L.ao_radius = lighting.aoRadius;
    L.seed = lighting.seed;
    L.reserved = 0;
    m_frameW = m_frameH = 0; m_frameStale = false;
    m_frame.resize(static_cast<size_t>(width) * height * 4);
    const int rc = surface ? api().render_lit_triangles_host(m_ctx, &f, &L, m_frame.data(), nullptr)
                           : api().render_lit_host(m_ctx, &f, &L, m_frame.data(), nullptr);
    if (rc != RTO_OK) {
        m_lastError = api().last_error(m_ctx);
        std::cerr << "[RayTracerBVH] lit " << (surface ? "surface " : "") << "render failed: " << m_lastError << std::endl;
        m_frame.clear();
        return;
    }
    m_frameW = width; m_frameH = height;
}

// A field view of the first GPU's resident grid (rto_render_field_host): the frame goes to framebuffer(), the per-pixel values and
// the summary to fieldValues() / fieldSummary().  A grid that came as a pointer tree is built on the GPU first, as the fields'
// makers do; a refusal leaves no frame and no values.
int RayTracerBVH::renderField(const Camera& camera, int width, int height, float aspect, float fovDeg, const rto_field_view& view,
                              const uint32_t* lut, const int32_t* volume) {
    m_fieldValues.clear();
    m_fieldSummary = rto_field_view_summary{ 0, 0, 0, 0, 0, 0 };
    if (!computeUsable("renderField")) return RTO_E_INVALID;
    if (m_numNodes > 0 && !makeGridResident("field view")) return RTO_E_HIP;
    const rto_frame f = frame_of(camera, width, height, aspect, fovDeg);
    m_frameW = m_frameH = 0; m_frameStale = false;
    m_frame.clear();
    if (width > 0 && height > 0) {
        m_frame.resize(static_cast<size_t>(width) * height * 4);
        m_fieldValues.resize(static_cast<size_t>(width) * height);
    }
    const int rc = api().render_field_host(m_ctx, &f, &view, lut, volume, m_frame.empty() ? nullptr : m_frame.data(),
                                           m_fieldValues.empty() ? nullptr : m_fieldValues.data(), &m_fieldSummary, nullptr);
    if (rc != RTO_OK) {
        m_frame.clear();
        m_fieldValues.clear();
        m_fieldSummary = rto_field_view_summary{ 0, 0, 0, 0, 0, 0 };
        return regionFailed(rc, "renderField");
    }
    m_frameW = width; m_frameH = height;
    return RTO_OK;
}

// A projection of the first GPU's resident grid (rto_project_field_host): the frame goes to framebuffer(), the per-pixel outputs
// to projectionValues(), the summary to fieldSummary().  A refusal leaves no frame and no values.
int RayTracerBVH::projectField(const Camera& camera, int width, int height, float aspect, float fovDeg,
                               const rto_field_projection& projection, const uint32_t* lut, const int32_t* volume) {
    m_projection = ProjectionValues();
    m_fieldSummary = rto_field_view_summary{ 0, 0, 0, 0, 0, 0 };
    if (!computeUsable("projectField")) return RTO_E_INVALID;
    if (m_numNodes > 0 && !makeGridResident("field projection")) return RTO_E_HIP;
    const rto_frame f = frame_of(camera, width, height, aspect, fovDeg);
    m_frameW = m_frameH = 0; m_frameStale = false;
    m_frame.clear();
    if (width > 0 && height > 0) {
        const size_t n = static_cast<size_t>(width) * height;
        m_frame.resize(n * 4);
        m_projection.values.resize(n); m_projection.voxels.resize(n); m_projection.counts.resize(n); m_projection.sums.resize(n);
    }
    ProjectionValues& p = m_projection;
    const bool have = !m_frame.empty();
    const int rc = api().project_field_host(m_ctx, &f, &projection, lut, volume, have ? m_frame.data() : nullptr,
                                            have ? p.values.data() : nullptr, have ? p.voxels.data() : nullptr,
                                            have ? p.sums.data() : nullptr, have ? p.counts.data() : nullptr, &m_fieldSummary, nullptr);
    if (rc != RTO_OK) {
        m_frame.clear();
        m_projection = ProjectionValues();
        m_fieldSummary = rto_field_view_summary{ 0, 0, 0, 0, 0, 0 };
        return regionFailed(rc, "projectField");
    }
    m_frameW = width; m_frameH = height;
    return RTO_OK;
}

// A composite of the first GPU's resident grid (rto_composite_field_host): the frame goes to framebuffer(), the per-pixel outputs
// to compositeValues(), the summary to compositeSummary().  A refusal leaves no frame and no values.
int RayTracerBVH::compositeField(const Camera& camera, int width, int height, float aspect, float fovDeg,
                                 const rto_field_composite& composite, const uint32_t* lut, const int32_t* volume, const float* under) {
    m_composite = CompositeValues();
    m_compositeSummary = rto_composite_summary{ 0, 0, 0, 0 };
    if (!computeUsable("compositeField")) return RTO_E_INVALID;
    if (m_numNodes > 0 && !makeGridResident("field composite")) return RTO_E_HIP;
    const rto_frame f = frame_of(camera, width, height, aspect, fovDeg);
    m_frameW = m_frameH = 0; m_frameStale = false;
    m_frame.clear();
    if (width > 0 && height > 0) {
        const size_t n = static_cast<size_t>(width) * height;
        m_frame.resize(n * 4);
        m_composite.transmittance.resize(n); m_composite.first.resize(n); m_composite.stops.resize(n); m_composite.counts.resize(n);
    }
    CompositeValues& p = m_composite;
    const bool have = !m_frame.empty();
    const int rc = api().composite_field_host(m_ctx, &f, &composite, lut, volume, under, have ? m_frame.data() : nullptr,
                                              have ? p.transmittance.data() : nullptr, have ? p.first.data() : nullptr,
                                              have ? p.stops.data() : nullptr, have ? p.counts.data() : nullptr, &m_compositeSummary);
    if (rc != RTO_OK) {
        m_frame.clear();
        m_composite = CompositeValues();
        m_compositeSummary = rto_composite_summary{ 0, 0, 0, 0 };
        return regionFailed(rc, "compositeField");
    }
    m_frameW = width; m_frameH = height;
    return RTO_OK;
}

static RayHit to_ray_hit(const rto_hit& h) {
    RayHit r;
    r.t = h.t; r.node = h.node; r.face = h.face; r.size = h.size; r.x = h.x; r.y = h.y; r.z = h.z;
    return r;
}

void RayTracerBVH::intersectRays(const std::vector<Ray>& rays, std::vector<RayHit>& hits, int mode, float tMin, float tMax) {
    hits.assign(rays.size(), RayHit());
    if (!m_computeInited || !m_computeOk) {
        std::cerr << "[RayTracerBVH] Compute pipeline not initialized or failed.\n";
        return;
    }
    if (rays.empty() || m_numNodes <= 0) return;
    std::vector<rto_ray> in(rays.size());
    for (size_t i = 0; i < rays.size(); i++) {
        const Ray& r = rays[i];
        in[i] = rto_ray{ r.origin.x, r.origin.y, r.origin.z, tMin, r.direction.x, r.direction.y, r.direction.z, tMax };
    }
    std::vector<rto_hit> out(rays.size());
    if (api().query_rays_host(m_ctx, mode, in.data(), (int64_t)in.size(), out.data()) != RTO_OK) {
        m_lastError = api().last_error(m_ctx);
        std::cerr << "[RayTracerBVH] ray query failed: " << m_lastError << std::endl;
        return;
    }
    for (size_t i = 0; i < out.size(); i++) hits[i] = to_ray_hit(out[i]);
}

bool RayTracerBVH::pick(const Camera& camera, int px, int py, int width, int height, float aspect, float fovDeg, RayHit& out) {
    out = RayHit();
    if (!m_computeInited || !m_computeOk) {
        std::cerr << "[RayTracerBVH] Compute pipeline not initialized or failed.\n";
        return false;
    }
    if (m_numNodes <= 0 || width <= 0 || height <= 0) return false;
    const rto_frame f = frame_of(camera, width, height, aspect, fovDeg);
    const int32_t xy[2] = { px, py };
    rto_hit h;
    if (api().query_pixels_host(m_ctx, RTO_QUERY_FIRST, &f, xy, 1, &h) != RTO_OK) {
        m_lastError = api().last_error(m_ctx);
        std::cerr << "[RayTracerBVH] pick failed: " << m_lastError << std::endl;
        return false;
    }
    out = to_ray_hit(h);
    return out.hit();
}

static RaySpan to_ray_span(const rto_span& s) {
    RaySpan r;
    r.length = s.length; r.tEnter = s.t_enter; r.tExit = s.t_exit; r.leaves = s.leaves; r.node = s.node; r.face = s.face;
    return r;
}

void RayTracerBVH::intersectSpans(const std::vector<Ray>& rays, std::vector<RaySpan>& spans, float tMin, float tMax) {
    spans.assign(rays.size(), RaySpan());
    if (!m_computeInited || !m_computeOk) {
        std::cerr << "[RayTracerBVH] Compute pipeline not initialized or failed.\n";
        return;
    }
    if (rays.empty() || m_numNodes <= 0) return;
    std::vector<rto_ray> in(rays.size());
    for (size_t i = 0; i < rays.size(); i++) {
        const Ray& r = rays[i];
        in[i] = rto_ray{ r.origin.x, r.origin.y, r.origin.z, tMin, r.direction.x, r.direction.y, r.direction.z, tMax };
    }
    std::vector<rto_span> out(rays.size());
    if (api().query_spans_host(m_ctx, in.data(), (int64_t)in.size(), out.data()) != RTO_OK) {
        m_lastError = api().last_error(m_ctx);
        std::cerr << "[RayTracerBVH] span query failed: " << m_lastError << std::endl;
        return;
    }
    for (size_t i = 0; i < out.size(); i++) spans[i] = to_ray_span(out[i]);
}

bool RayTracerBVH::pickSpan(const Camera& camera, int px, int py, int width, int height, float aspect, float fovDeg, RaySpan& out) {
    out = RaySpan();
    if (!m_computeInited || !m_computeOk) {
        std::cerr << "[RayTracerBVH] Compute pipeline not initialized or failed.\n";
        return false;
    }
    if (m_numNodes <= 0 || width <= 0 || height <= 0) return false;
    const rto_frame f = frame_of(camera, width, height, aspect, fovDeg);
    const int32_t xy[2] = { px, py };
    rto_span s;
    if (api().query_span_pixels_host(m_ctx, &f, xy, 1, &s) != RTO_OK) {
        m_lastError = api().last_error(m_ctx);
        std::cerr << "[RayTracerBVH] pickSpan failed: " << m_lastError << std::endl;
        return false;
    }
    out = to_ray_span(s);
    return out.hit();
}

std::vector<MCTriangle> RayTracerBVH::extractMeshPlanes(int kind, const float* planes, float extraMargin) {
    std::vector<MCTriangle> out;
    m_lastError.clear();                       // an empty list with lastError() empty is an empty mesh, not a failure
    if (!computeUsable("extractMesh")) {
        std::cerr << "[RayTracerBVH] Compute pipeline not initialized or failed.\n";
        return out;
    }
    if (m_numNodes <= 0) {
        m_lastError = "extractMesh: no octree set";
        return out;
    }
    rto_mesh_cull cull;
    if (planes) { std::memcpy(cull.planes, planes, sizeof cull.planes); cull.margin = extraMargin; }
    int64_t n = 0;
    if (api().extract_mesh(m_ctx, kind, planes ? &cull : nullptr, &n) != RTO_OK) {
        m_lastError = api().last_error(m_ctx);
        std::cerr << "[RayTracerBVH] extractMesh failed: " << m_lastError << std::endl;
        return out;
    }
    std::vector<float> rec((size_t)n * 12);
    if (n > 0 && api().download_mesh(m_ctx, rec.data(), n, nullptr, &n) != RTO_OK) {
        m_lastError = api().last_error(m_ctx);
        std::cerr << "[RayTracerBVH] extractMesh failed: " << m_lastError << std::endl;
        return out;
    }
    out.resize((size_t)n);
    for (size_t i = 0; i < out.size(); i++) {
        const float* r = rec.data() + 12 * i;
        for (int v = 0; v < 3; v++) out[i].v[v] = rto_host::vec3(r[3 * v], r[3 * v + 1], r[3 * v + 2]);
        out[i].normal[0] = out[i].normal[1] = out[i].normal[2] = rto_host::vec3(r[9], r[10], r[11]);
    }
    return out;
}

std::vector<MCTriangle> RayTracerBVH::isoSurface(int source, float level, float outside, bool pad, const int32_t* volume,
                                                 std::vector<int32_t>* triCell, rto_iso_summary* summary) {
    std::vector<MCTriangle> out;
    if (triCell) triCell->clear();
    m_lastError.clear();                       // an empty list with lastError() empty is an empty surface, not a failure
    if (!computeUsable("isoSurface")) {
        std::cerr << "[RayTracerBVH] Compute pipeline not initialized or failed.\n";
        return out;
    }
    if (m_numNodes > 0 && !makeGridResident("isosurface")) return out;
    rto_iso_params p;
    std::memset(&p, 0, sizeof p);
    p.source = source;
    p.valid_lo = 0; p.valid_hi = 0x7ffffffe;
    p.level = level; p.outside = outside;
    p.pad = pad ? 1 : 0;
    std::vector<float> rec;
    int64_t n = 0;
    if (api().extract_isosurface_host(m_ctx, &p, volume, summary) != RTO_OK || api().download_isosurface(m_ctx, nullptr, 0, nullptr, &n) != RTO_OK) {
        m_lastError = api().last_error(m_ctx);
        std::cerr << "[RayTracerBVH] isoSurface failed: " << m_lastError << std::endl;
        return out;
    }
    rec.resize((size_t)n * 12);
    if (triCell) triCell->resize((size_t)n);
    if (n > 0 && api().download_isosurface(m_ctx, rec.data(), n, triCell ? triCell->data() : nullptr, &n) != RTO_OK) {
        m_lastError = api().last_error(m_ctx);
        std::cerr << "[RayTracerBVH] isoSurface failed: " << m_lastError << std::endl;
        if (triCell) triCell->clear();
        return out;
    }
    out.resize((size_t)n);
    for (size_t i = 0; i < out.size(); i++) {
        const float* r = rec.data() + 12 * i;
        for (int v = 0; v < 3; v++) out[i].v[v] = rto_host::vec3(r[3 * v], r[3 * v + 1], r[3 * v + 2]);
        out[i].normal[0] = out[i].normal[1] = out[i].normal[2] = rto_host::vec3(r[9], r[10], r[11]);
    }
    return out;
}

std::vector<MCTriangle> RayTracerBVH::dualContour(const rto_dc_params& params, std::vector<int32_t>* triCell, rto_dc_summary* summary) {
    std::vector<MCTriangle> out;
    if (triCell) triCell->clear();
    m_lastError.clear();                       // an empty list with lastError() empty is an empty surface, not a failure
    if (!computeUsable("dualContour")) {
        std::cerr << "[RayTracerBVH] Compute pipeline not initialized or failed.\n";
        return out;
    }
    if (m_numNodes > 0 && !makeGridResident("dual contouring")) return out;
    std::vector<float> rec;
    int64_t n = 0;
    if (api().extract_dual_contour(m_ctx, &params, summary) != RTO_OK || api().download_dual_contour(m_ctx, nullptr, 0, nullptr, &n) != RTO_OK) {
        m_lastError = api().last_error(m_ctx);
        std::cerr << "[RayTracerBVH] dualContour failed: " << m_lastError << std::endl;
        return out;
    }
    rec.resize((size_t)n * 12);
    if (triCell) triCell->resize((size_t)n);
    if (n > 0 && api().download_dual_contour(m_ctx, rec.data(), n, triCell ? triCell->data() : nullptr, &n) != RTO_OK) {
        m_lastError = api().last_error(m_ctx);
        std::cerr << "[RayTracerBVH] dualContour failed: " << m_lastError << std::endl;
        if (triCell) triCell->clear();
        return out;
    }
    out.resize((size_t)n);
    for (size_t i = 0; i < out.size(); i++) {
        const float* r = rec.data() + 12 * i;
        for (int v = 0; v < 3; v++) out[i].v[v] = rto_host::vec3(r[3 * v], r[3 * v + 1], r[3 * v + 2]);
        out[i].normal[0] = out[i].normal[1] = out[i].normal[2] = rto_host::vec3(r[9], r[10], r[11]);
    }
    return out;
}

std::vector<rto_dual_vertex> RayTracerBVH::dualVertices(const int64_t* voxels, int64_t n) {
    std::vector<rto_dual_vertex> out;
    m_lastError.clear();
    if (!computeUsable("dualVertices")) {
        std::cerr << "[RayTracerBVH] Compute pipeline not initialized or failed.\n";
        return out;
    }
    if (m_numNodes > 0 && !makeGridResident("dual contouring")) return out;
    out.resize(n > 0 ? (size_t)n : 0);
    if (api().query_dual_vertices_host(m_ctx, voxels, n, out.data()) != RTO_OK) {
        m_lastError = api().last_error(m_ctx);
        std::cerr << "[RayTracerBVH] dualVertices failed: " << m_lastError << std::endl;
        out.clear();
    }
    return out;
}

std::vector<MCTriangle> RayTracerBVH::offsetSurface(float distanceInVoxels) {
    if (distanceField(RTO_SET_SOLID, INFINITY, nullptr) != RTO_OK) return {};
    return isoSurface(RTO_FIELD_DISTANCE, distanceInVoxels * distanceInVoxels, 1.0e9f, true);
}

std::vector<MCTriangle> RayTracerBVH::extractMesh(int kind, const Camera& camera, float aspect, float extraMargin) {
    if (!computeUsable("extractMesh")) {
        std::cerr << "[RayTracerBVH] Compute pipeline not initialized or failed.\n";
        return {};
    }
    const rto_frame f = frame_of(camera, 1, 1, aspect, 45.0f);       // renderOctree's own frustum: fov 45 (main.cpp:125)
    float planes[24];
    api().frustum_planes(f.view, 45.0f, aspect, planes);
    return extractMeshPlanes(kind, planes, extraMargin);
}

// The renders' ray direction through pixel (px, py) (S/RT:338-355 in the oracle's operation order: what fill_params and
// generate_ray_tab compute on the device), so that pickSurface's point is o + d t on the very ray the frame traced.
static rto_host::vec3 pixel_direction(const Camera& camera, int px, int py, int width, int height, float aspect, float fovDeg) {
    const auto view = camera.getView();
#ifdef RTO_REFERENCE_HEADERS
    const auto m = glm::inverse(view);
    const float tanHalfFov = std::tan(glm::radians(fovDeg) * 0.5f);
#else
    const auto m = rtmath::inverse(view);
    const float tanHalfFov = std::tan(rtmath::radians(fovDeg) * 0.5f);
#endif
    float nx = ((float)px + 0.5f) / (float)width * 2.0f - 1.0f;
    float ny = 1.0f - ((float)py + 0.5f) / (float)height * 2.0f;
    nx *= aspect;
    nx *= tanHalfFov;
    ny *= tanHalfFov;
    const float d4 = (nx * nx + ny * ny) + ((-1.0f) * (-1.0f) + 0.0f * 0.0f);
    const float inv4 = 1.0f / std::sqrt(d4);
    const float vx = nx * inv4, vy = ny * inv4, vz = (-1.0f) * inv4, vw = 0.0f * inv4;
    const float wx = (m[0][0] * vx + m[1][0] * vy) + (m[2][0] * vz + m[3][0] * vw);
    const float wy = (m[0][1] * vx + m[1][1] * vy) + (m[2][1] * vz + m[3][1] * vw);
    const float wz = (m[0][2] * vx + m[1][2] * vy) + (m[2][2] * vz + m[3][2] * vw);
    const float tx = wx * wx, ty = wy * wy, tz = wz * wz;
    const float s = 1.0f / std::sqrt(tx + ty + tz);
    return rto_host::vec3(wx * s, wy * s, wz * s);
}

static TriangleHit to_triangle_hit(const rto_tri_hit& h, const rto_host::vec3& o, const rto_host::vec3& d) {
    TriangleHit r;
    if (h.tri < 0) return r;
    r.t = h.t; r.tri = h.tri; r.node = h.node; r.u = h.u; r.v = h.v;
    r.point = rto_host::vec3(o.x + d.x * h.t, o.y + d.y * h.t, o.z + d.z * h.t);
    r.normal = rto_host::vec3(h.nx, h.ny, h.nz);
    return r;
}

void RayTracerBVH::intersectTriangles(const std::vector<Ray>& rays, std::vector<TriangleHit>& hits, int mode, float tMin, float tMax) {
    hits.assign(rays.size(), TriangleHit());
    if (!m_computeInited || !m_computeOk) {
        std::cerr << "[RayTracerBVH] Compute pipeline not initialized or failed.\n";
        return;
    }
    if (rays.empty() || m_numNodes <= 0) return;
    std::vector<rto_ray> in(rays.size());
    for (size_t i = 0; i < rays.size(); i++) {
        const Ray& r = rays[i];
        in[i] = rto_ray{ r.origin.x, r.origin.y, r.origin.z, tMin, r.direction.x, r.direction.y, r.direction.z, tMax };
    }
    std::vector<rto_tri_hit> out(rays.size());
    if (api().query_triangles_host(m_ctx, mode, in.data(), (int64_t)in.size(), out.data()) != RTO_OK) {
        m_lastError = api().last_error(m_ctx);
        std::cerr << "[RayTracerBVH] triangle query failed: " << m_lastError << std::endl;
        return;
    }
    for (size_t i = 0; i < out.size(); i++) hits[i] = to_triangle_hit(out[i], rays[i].origin, rays[i].direction);
}

bool RayTracerBVH::pickSurface(const Camera& camera, int px, int py, int width, int height, float aspect, float fovDeg, TriangleHit& out) {
    out = TriangleHit();
    if (!m_computeInited || !m_computeOk) {
        std::cerr << "[RayTracerBVH] Compute pipeline not initialized or failed.\n";
        return false;
    }
    if (m_numNodes <= 0 || width <= 0 || height <= 0 || px < 0 || px >= width || py < 0 || py >= height) return false;
    const rto_frame f = frame_of(camera, width, height, aspect, fovDeg);
    const int32_t xy[2] = { px, py };
    rto_tri_hit h;
    if (api().query_triangle_pixels_host(m_ctx, RTO_QUERY_FIRST, &f, xy, 1, &h) != RTO_OK) {
        m_lastError = api().last_error(m_ctx);
        std::cerr << "[RayTracerBVH] pickSurface failed: " << m_lastError << std::endl;
        return false;
    }
    if (h.tri < 0) return false;
    out = to_triangle_hit(h, camera.getPos(), pixel_direction(camera, px, py, width, height, aspect, fovDeg));
    return true;
}

const std::vector<float>& RayTracerBVH::framebuffer() const {
    if (m_frameStale && m_ctx) {
        m_frame.resize(static_cast<size_t>(m_frameW) * m_frameH * 4);
        if (api().download_resident(m_ctx, m_frame.data()) != RTO_OK) {
            m_lastError = api().last_error(m_ctx);
            std::cerr << "[RayTracerBVH] frame read-back failed: " << m_lastError << std::endl;
            m_frame.clear();
        }
        m_frameStale = false;
    }
    return m_frame;
}

void RayTracerBVH::finish() const {
    for (rto_context* c : m_ctxs) (void)api().synchronize(c);
}

void RayTracerBVH::renderSceneCompute(const Camera& camera, int width, int height, float aspect, float fovDeg) {
    if (!m_computeInited || !m_computeOk) {
        std::cerr << "[RayTracerBVH] Compute pipeline not initialized or failed.\n";
        return;
    }
    if (m_numNodes <= 0) return;
    render(camera, width, height, aspect, fovDeg);
}

void RayTracerBVH::renderSceneComputeWithCulling(const Camera& camera, int width, int height, float aspect,
                                                 float fovDeg, bool updateFrustum) {
    if (!m_computeInited || !m_computeOk) {
        std::cerr << "[RayTracerBVH] Compute pipeline not initialized or failed.\n";
        return;
    }
    if (m_numNodes <= 0) {
        std::printf("No nodes to render.\n");
        return;
    }
    if (updateFrustum) {
        // the reference recomputes visibility on the CPU and re-uploads the compacted array
        // (RayTracerBVH.cpp:725-813); here the same test and compaction run on the GPU.
        const auto view = camera.getView();
        if (!forEachContext([&](rto_context* c) { return api().update_frustum(c, &view[0][0], fovDeg, aspect, 1); }, "frustum update")) return;
    }
    render(camera, width, height, aspect, fovDeg);
}

// ---- region queries: the C ABI's records, one per point or brush; a refusal leaves the defaults and returns its code
int RayTracerBVH::regionFailed(int rc, const char* what) {
    m_lastError = api().last_error(m_ctx);
    std::cerr << "[RayTracerBVH] " << what << " failed: " << m_lastError << std::endl;
    return rc;
}

// Is the compute pipeline usable?  If not, lastError() says so in `who`'s name.
bool RayTracerBVH::computeUsable(const char* who) {
    if (m_computeInited && m_computeOk) return true;
    m_lastError = std::string(who) + ": compute pipeline not initialized or failed";
    return false;
}

// A per-voxel field of the first GPU's resident grid: make() makes it resident; when the caller gave a vector, it is sized for the
// grid and filled by `download`, and left empty on any failure.  The code is RTO_OK or the refusal's.
template <class Make>
int RayTracerBVH::fieldInto(const char* who, const char* what, std::vector<int32_t>* out, Make&& make, int (*download)(rto_context*, int32_t*, int64_t)) {
    if (out) out->clear();
    if (!computeUsable(who)) return RTO_E_INVALID;
    if (m_numNodes > 0 && !makeGridResident(what)) return RTO_E_HIP;
    int rc = make();
    if (rc == RTO_OK && out) {
        out->resize((size_t)m_grid.dimX * m_grid.dimY * m_grid.dimZ);
        rc = download(m_ctx, out->data(), (int64_t)out->size());
        if (rc != RTO_OK) out->clear();
    }
    if (rc != RTO_OK) return regionFailed(rc, who);
    return RTO_OK;
}

int RayTracerBVH::locate(const std::vector<rto_host::vec3>& points, std::vector<PointLocation>& out) {
    out.assign(points.size(), PointLocation());
    if (!computeUsable("locate")) return RTO_E_INVALID;
    if (points.empty()) return RTO_OK;
    std::vector<float> in(3 * points.size());
    for (size_t i = 0; i < points.size(); i++) { in[3 * i] = points[i].x; in[3 * i + 1] = points[i].y; in[3 * i + 2] = points[i].z; }
    std::vector<rto_point_hit> hits(points.size());
    const int rc = api().query_points_host(m_ctx, in.data(), (int64_t)points.size(), hits.data());
    if (rc != RTO_OK) return regionFailed(rc, "locate");
    for (size_t i = 0; i < hits.size(); i++) {
        const rto_point_hit& h = hits[i];
        PointLocation& o = out[i];
        o.node = h.node; o.solid = h.solid != 0; o.x = h.x; o.y = h.y; o.z = h.z; o.size = h.size; o.depth = h.depth;
    }
    return RTO_OK;
}

int RayTracerBVH::census(const std::vector<VoxelBrush>& regions, std::vector<RegionCensus>& out) {
    out.assign(regions.size(), RegionCensus());
    if (!computeUsable("census")) return RTO_E_INVALID;
    if (regions.empty()) return RTO_OK;
    std::vector<rto_brush> in(regions.size());
    for (size_t i = 0; i < regions.size(); i++) {
        const VoxelBrush& v = regions[i];
        in[i] = rto_brush{ { v.centre.x, v.centre.y, v.centre.z }, { v.extent.x, v.extent.y, v.extent.z }, v.shape, v.op };
    }
    std::vector<rto_region> res(regions.size());
    const int rc = api().query_regions_host(m_ctx, in.data(), (int64_t)in.size(), res.data());
    if (rc != RTO_OK) return regionFailed(rc, "census");
    for (size_t i = 0; i < res.size(); i++) {
        const rto_region& r = res[i];
        RegionCensus& o = out[i];
        o.filled = r.filled; o.covered = r.covered; o.solidLeaves = r.solid_leaves; o.firstNode = r.first_node;
    }
    return RTO_OK;
}

int RayTracerBVH::nearestSolid(const std::vector<rto_host::vec3>& points, std::vector<NearestSolid>& out, float maxDist) {
    out.assign(points.size(), NearestSolid());
    if (!computeUsable("nearestSolid")) return RTO_E_INVALID;
    if (points.empty()) return RTO_OK;
    std::vector<rto_near_point> in(points.size());
    for (size_t i = 0; i < points.size(); i++) in[i] = rto_near_point{ points[i].x, points[i].y, points[i].z, maxDist };
    std::vector<rto_nearest> res(points.size());
    const int rc = api().query_nearest_host(m_ctx, in.data(), (int64_t)in.size(), res.data());
    if (rc != RTO_OK) return regionFailed(rc, "nearestSolid");
    rto_scene_bounds sb;
    const int rcb = api().scene_bounds_get(m_ctx, &sb);
    if (rcb != RTO_OK) return regionFailed(rcb, "nearestSolid");
    for (size_t i = 0; i < res.size(); i++) {
        const rto_nearest& r = res[i];
        NearestSolid& o = out[i];
        o.dist2 = r.dist2; o.node = r.node; o.size = r.size;
        for (int a = 0; a < 3; a++) o.cq[a] = r.cq[a];
        if (r.dist2 >= 0) o.distance = std::sqrt((double)r.dist2) / 64.0 * (double)sb.voxel_size;
    }
    return RTO_OK;
}

// Carve / fill the resident grid on every GPU (rto_edit_voxels) and rebuild the octree there; triangles that were resident are
// rebuilt too.  After setOctree() no grid is resident yet: the first edit builds the octree from m_grid (the same array, DESIGN.md
// section 1, N4) and edits that.  m_grid is then stale; grid() fetches it when asked, never per edit.
void RayTracerBVH::editVoxels(const std::vector<VoxelBrush>& brushes) {
    if (!m_computeInited || !m_computeOk) {
        std::cerr << "[RayTracerBVH] Compute pipeline not initialized or failed.\n";
        return;
    }
    m_lastEditChanged = -1;
    if (m_numNodes <= 0) return;
    std::vector<rto_brush> b(brushes.size());
    for (size_t i = 0; i < brushes.size(); i++) {
        const VoxelBrush& v = brushes[i];
        b[i] = rto_brush{ { v.centre.x, v.centre.y, v.centre.z }, { v.extent.x, v.extent.y, v.extent.z }, v.shape, v.op };
    }
    const bool fromHost = !m_flatNodes.empty();
    const float gridMin[3] = { m_grid.minX, m_grid.minY, m_grid.minZ };
    int64_t changed = 0;
    if (!forEachContext([&](rto_context* c) {
            if (fromHost) {
                int64_t numTris = 0;
                const bool hadTris = api().download_leaf_triangles(c, nullptr, 0, nullptr, &numTris) == RTO_OK;
                int rc = api().build_octree(c, reinterpret_cast<const uint8_t*>(m_grid.data.data()), m_grid.dimX, m_grid.dimY, m_grid.dimZ,
                                            gridMin, m_grid.voxelSize);
                if (rc == RTO_OK && hadTris) rc = api().build_leaf_triangles(c, nullptr, 0, 0, 0);
                if (rc != RTO_OK) return rc;
            }
            return api().edit_voxels(c, b.data(), (int)b.size(), c == m_ctx ? &changed : nullptr);
        }, "voxel edit"))
        return;
    m_lastEditChanged = changed;
    if (fromHost) { m_flatNodes.clear(); m_octreeRoot = nullptr; }   // the caller's pointer tree no longer describes the scene
    if (changed > 0 || fromHost) {
        rto_octree_info info;
        if (api().octree_info(m_ctx, &info) == RTO_OK) m_numNodes = static_cast<int>(info.num_nodes);
    }
    if (changed > 0) m_gridStale = true;
}

// After setOctree() the GPUs hold the caller's node array and no grid: build the octree from m_grid there (the same array, DESIGN.md
// section 1, N4), keeping leaf triangles resident where they were, as the first editVoxels does.
bool RayTracerBVH::makeGridResident(const char* what) {
    if (m_flatNodes.empty()) return true;
    const float gridMin[3] = { m_grid.minX, m_grid.minY, m_grid.minZ };
    if (!forEachContext([&](rto_context* c) {
            int64_t numTris = 0;
            const bool hadTris = api().download_leaf_triangles(c, nullptr, 0, nullptr, &numTris) == RTO_OK;
            int rc = api().build_octree(c, reinterpret_cast<const uint8_t*>(m_grid.data.data()), m_grid.dimX, m_grid.dimY, m_grid.dimZ,
                                        gridMin, m_grid.voxelSize);
            if (rc == RTO_OK && hadTris) rc = api().build_leaf_triangles(c, nullptr, 0, 0, 0);
            return rc;
        }, what))
        return false;
    m_flatNodes.clear(); m_octreeRoot = nullptr;      // the caller's pointer tree no longer describes what the GPUs hold
    rto_octree_info info;
    if (api().octree_info(m_ctx, &info) == RTO_OK) m_numNodes = static_cast<int>(info.num_nodes);
    return true;
}

std::vector<rto_component> RayTracerBVH::labelComponents(int set, int connectivity) {
    std::vector<rto_component> table;
    m_lastComponents = -1;
    if (!m_computeInited || !m_computeOk) {
        std::cerr << "[RayTracerBVH] Compute pipeline not initialized or failed.\n";
        return table;
    }
    if (m_numNodes <= 0 || !makeGridResident("component labelling")) return table;
    int64_t count = 0;
    int rc = api().label_components(m_ctx, set, connectivity, &count);
    if (rc == RTO_OK && count > 0) {
        table.resize((size_t)count);
        rc = api().download_components(m_ctx, table.data(), count, &count);
    }
    if (rc != RTO_OK) {
        m_lastError = api().last_error(m_ctx);
        std::cerr << "[RayTracerBVH] component labelling failed: " << m_lastError << std::endl;
        table.clear();
        return table;
    }
    m_lastComponents = count;
    return table;
}

std::vector<int32_t> RayTracerBVH::componentLabels() {
    std::vector<int32_t> labels;
    if (!m_ctx || m_numNodes <= 0) return labels;
    labels.resize((size_t)m_grid.dimX * m_grid.dimY * m_grid.dimZ);
    if (api().download_labels(m_ctx, labels.data(), (int64_t)labels.size()) != RTO_OK) {
        m_lastError = api().last_error(m_ctx);
        labels.clear();
    }
    return labels;
}

int64_t RayTracerBVH::editComponents(int set, int connectivity, int select, int64_t arg) {
    if (!m_computeInited || !m_computeOk) {
        std::cerr << "[RayTracerBVH] Compute pipeline not initialized or failed.\n";
        return -1;
    }
    m_lastEditChanged = -1;
    if (m_numNodes <= 0 || !makeGridResident("component edit")) return -1;
    int64_t changed = 0;
    if (!forEachContext([&](rto_context* c) { return api().edit_components(c, set, connectivity, select, arg, c == m_ctx ? &changed : nullptr); },
                        "component edit"))
        return -1;
    m_lastEditChanged = changed;
    if (changed > 0) {
        rto_octree_info info;
        if (api().octree_info(m_ctx, &info) == RTO_OK) m_numNodes = static_cast<int>(info.num_nodes);
        m_gridStale = true;
    }
    return changed;
}

int64_t RayTracerBVH::removeDebris(int64_t minVoxels, int connectivity) {
    return editComponents(RTO_SET_SOLID, connectivity, RTO_SELECT_SMALLER_THAN, minVoxels);
}
int64_t RayTracerBVH::fillCavities() { return editComponents(RTO_SET_EMPTY, RTO_CONN_FACE, RTO_SELECT_ENCLOSED, 0); }
int64_t RayTracerBVH::keepLargest(int connectivity) { return editComponents(RTO_SET_SOLID, connectivity, RTO_SELECT_ALL_BUT_LARGEST, 0); }
int64_t RayTracerBVH::flipComponentAt(int i, int j, int k, int set, int connectivity) {
    if (i < 0 || i >= m_grid.dimX || j < 0 || j >= m_grid.dimY || k < 0 || k >= m_grid.dimZ) {
        m_lastError = "flipComponentAt: the voxel lies outside the grid";
        m_lastEditChanged = -1;
        return -1;
    }
    return editComponents(set, connectivity, RTO_SELECT_CONTAINING, (int64_t)i + (int64_t)m_grid.dimX * ((int64_t)j + (int64_t)m_grid.dimY * k));
}

// The distance field of the first GPU's resident grid (rto_distance_field); the code is RTO_OK or the refusal's.
int RayTracerBVH::distanceField(int set, float maxDist, std::vector<int32_t>* d2, rto_dist_summary* summary) {
    return fieldInto("distanceField", "distance field", d2, [&] { return api().distance_field(m_ctx, set, maxDist, summary); },
                     api().download_distance);
}

// rto_edit_morphology on every GPU: the number of voxels changed, or the refusal's code (negative).
int64_t RayTracerBVH::editMorphology(int op, float radius) {
    m_lastEditChanged = -1;
    if (!computeUsable("morphology")) return RTO_E_INVALID;
    if (m_numNodes > 0 && !makeGridResident("morphology")) return RTO_E_HIP;
    int64_t changed = 0;
    for (rto_context* c : m_ctxs) {
        const int rc = api().edit_morphology(c, op, radius, c == m_ctx ? &changed : nullptr);
        if (rc != RTO_OK) {
            m_lastError = api().last_error(c);
            std::cerr << "[RayTracerBVH] morphology failed: " << m_lastError << std::endl;
            return rc;
        }
    }
    m_lastEditChanged = changed;
    if (changed > 0) {
        rto_octree_info info;
        if (api().octree_info(m_ctx, &info) == RTO_OK) m_numNodes = static_cast<int>(info.num_nodes);
        m_gridStale = true;
    }
    return changed;
}

int64_t RayTracerBVH::dilate(float radius) { return editMorphology(RTO_MORPH_DILATE, radius); }
int64_t RayTracerBVH::erode(float radius) { return editMorphology(RTO_MORPH_ERODE, radius); }
int64_t RayTracerBVH::open(float radius) { return editMorphology(RTO_MORPH_OPEN, radius); }
int64_t RayTracerBVH::close(float radius) { return editMorphology(RTO_MORPH_CLOSE, radius); }

int RayTracerBVH::thickestPoint(ThickestPoint& out) {
    out = ThickestPoint();
    rto_dist_summary s;
    const int rc = distanceField(RTO_SET_EMPTY, INFINITY, nullptr, &s);
    if (rc != RTO_OK) return rc;
    if (s.finite == 0 || s.max_d2 <= 0) return RTO_OK;                 // nothing EMPTY to measure from, or nothing FILLED
    out.found = true;
    out.i = (int)(s.argmax % m_grid.dimX); out.j = (int)((s.argmax / m_grid.dimX) % m_grid.dimY); out.k = (int)(s.argmax / ((int64_t)m_grid.dimX * m_grid.dimY));
    out.d2 = s.max_d2;
    out.distance = std::sqrt((double)s.max_d2) * (double)m_grid.voxelSize;
    return RTO_OK;
}

// The geodesic field of the first GPU's resident grid (rto_geodesic_field); the code is RTO_OK or the refusal's.
int RayTracerBVH::geodesicField(const std::vector<int64_t>& seeds, int medium, int connectivity, int64_t limit, std::vector<int32_t>* g,
                                rto_geo_summary* summary) {
    return fieldInto("geodesicField", "geodesic field", g,
                     [&] { return api().geodesic_field(m_ctx, medium, connectivity, seeds.data(), (int64_t)seeds.size(), limit, summary); },
                     api().download_geodesic);
}

// The paths of the last geodesicField to `targets` (rto_geodesic_paths): rows of maxLen voxels, -1 behind each path; the full lengths.
int RayTracerBVH::pathsTo(const std::vector<int64_t>& targets, int64_t maxLen, std::vector<int64_t>& voxels, std::vector<int64_t>& lengths) {
    voxels.clear();
    lengths.clear();
    if (maxLen < 0 || targets.empty()) { m_lastError = "pathsTo: no targets, or a negative maxLen"; return RTO_E_INVALID; }
    if (!computeUsable("pathsTo")) return RTO_E_INVALID;
    voxels.assign(targets.size() * (size_t)maxLen, -1);
    lengths.assign(targets.size(), -1);
    const int rc = api().geodesic_paths(m_ctx, targets.data(), (int64_t)targets.size(), maxLen, maxLen > 0 ? voxels.data() : nullptr, lengths.data());
    if (rc != RTO_OK) { voxels.clear(); lengths.clear(); regionFailed(rc, "pathsTo"); }
    return rc;
}

// rto_edit_geodesic on every GPU: the number of voxels flipped, or the refusal's code (negative).
int64_t RayTracerBVH::floodFrom(const std::vector<int64_t>& seeds, int medium, int connectivity, int64_t limit) {
    m_lastEditChanged = -1;
    if (!computeUsable("floodFrom")) return RTO_E_INVALID;
    if (m_numNodes > 0 && !makeGridResident("flood")) return RTO_E_HIP;
    int64_t changed = 0;
    for (rto_context* c : m_ctxs) {
        const int rc = api().edit_geodesic(c, medium, connectivity, seeds.data(), (int64_t)seeds.size(), limit, c == m_ctx ? &changed : nullptr);
        if (rc != RTO_OK) {
            m_lastError = api().last_error(c);
            std::cerr << "[RayTracerBVH] flood failed: " << m_lastError << std::endl;
            return rc;
        }
    }
    m_lastEditChanged = changed;
    if (changed > 0) {
        rto_octree_info info;
        if (api().octree_info(m_ctx, &info) == RTO_OK) m_numNodes = static_cast<int>(info.num_nodes);
        m_gridStale = true;
    }
    return changed;
}

int RayTracerBVH::farthestPoint(const std::vector<int64_t>& seeds, int medium, int connectivity, FarthestPoint& out) {
    out = FarthestPoint();
    rto_geo_summary s;
    const int rc = geodesicField(seeds, medium, connectivity, 0x7fffffffll, nullptr, &s);
    if (rc != RTO_OK) return rc;
    if (s.reached == 0) return RTO_OK;                                  // no seed lies in the medium
    out.found = true;
    out.i = (int)(s.argmax % m_grid.dimX); out.j = (int)((s.argmax / m_grid.dimX) % m_grid.dimY); out.k = (int)(s.argmax / ((int64_t)m_grid.dimX * m_grid.dimY));
    out.voxel = s.argmax;
    out.g = s.max_g;
    out.reached = s.reached;
    return RTO_OK;
}

// The skeleton field of the first GPU's resident grid (rto_skeleton_field); the code is RTO_OK or the refusal's.
int RayTracerBVH::skeletonField(int set, int connectivity, int mode, const std::vector<int64_t>& anchors, int64_t maxPasses, std::vector<int32_t>* k,
                                rto_skel_summary* summary) {
    return fieldInto("skeletonField", "skeleton field", k,
                     [&] {
                         return api().skeleton_field(m_ctx, set, connectivity, mode, anchors.empty() ? nullptr : anchors.data(), (int64_t)anchors.size(),
                                                     maxPasses, summary);
                     },
                     api().download_skeleton);
}

// rto_edit_skeleton of the solid under RTO_CONN_FULL on every GPU: the number of voxels removed, or the refusal's code (negative).
int64_t RayTracerBVH::thin(int mode, int64_t maxPasses) {
    m_lastEditChanged = -1;
    if (!computeUsable("thin")) return RTO_E_INVALID;
    if (m_numNodes > 0 && !makeGridResident("thin")) return RTO_E_HIP;
    int64_t changed = 0;
    for (rto_context* c : m_ctxs) {
        const int rc = api().edit_skeleton(c, RTO_SET_SOLID, RTO_CONN_FULL, mode, nullptr, 0, maxPasses, c == m_ctx ? &changed : nullptr);
        if (rc != RTO_OK) {
            m_lastError = api().last_error(c);
            std::cerr << "[RayTracerBVH] thin failed: " << m_lastError << std::endl;
            return rc;
        }
    }
    m_lastEditChanged = changed;
    if (changed > 0) {
        rto_octree_info info;
        if (api().octree_info(m_ctx, &info) == RTO_OK) m_numNodes = static_cast<int>(info.num_nodes);
        m_gridStale = true;
    }
    return changed;
}

// What the thinning of the free space leaves when the two anchors are held (the grid stays as it is).
int RayTracerBVH::centreline(int64_t anchorA, int64_t anchorB, std::vector<int64_t>& voxels) {
    voxels.clear();
    std::vector<int32_t> k;
    const int rc = skeletonField(RTO_SET_EMPTY, RTO_CONN_FULL, RTO_SKEL_TOPOLOGY, { anchorA, anchorB }, RTO_SKEL_NO_LIMIT, &k);
    if (rc != RTO_OK) return rc;
    for (size_t v = 0; v < k.size(); v++)
        if (k[v] == 0) voxels.push_back((int64_t)v);
    return RTO_OK;
}

// The exposure field of the first GPU's resident grid (rto_exposure_field); the code is RTO_OK or the refusal's.
int RayTracerBVH::exposureField(const std::vector<int32_t>& dirs, const std::vector<int32_t>& weights, int mode, int reach, rto_expo_summary* summary) {
    if (!computeUsable("exposureField")) return RTO_E_INVALID;
    if (dirs.size() % 3 != 0 || (!weights.empty() && weights.size() != dirs.size() / 3)) {
        m_lastError = "exposureField: three components a direction, and one weight a direction or none";
        return RTO_E_INVALID;
    }
    if (m_numNodes > 0 && !makeGridResident("exposure field")) return RTO_E_HIP;
    const int rc = api().exposure_field(m_ctx, dirs.empty() ? nullptr : dirs.data(), weights.empty() ? nullptr : weights.data(), (int)(dirs.size() / 3),
                                        mode, reach, summary);
    if (rc != RTO_OK) return regionFailed(rc, "exposureField");
    return RTO_OK;
}

// The resident exposure field, downloaded.
int RayTracerBVH::exposure(std::vector<int32_t>& e) {
    e.clear();
    if (!computeUsable("exposure")) return RTO_E_INVALID;
    e.resize((size_t)m_grid.dimX * m_grid.dimY * m_grid.dimZ);
    const int rc = api().download_exposure(m_ctx, e.data(), (int64_t)e.size());
    if (rc != RTO_OK) { e.clear(); return regionFailed(rc, "exposure"); }
    return RTO_OK;
}

// The dose field of the first GPU's resident grid (rto_dose_field); the code is RTO_OK or the refusal's.
int RayTracerBVH::doseField(const std::vector<int32_t>& sources, const std::vector<uint32_t>& transmit, int falloff, int mode, int reach,
                            rto_dose_summary* summary) {
    if (!computeUsable("doseField")) return RTO_E_INVALID;
    if (sources.size() % 4 != 0) {
        m_lastError = "doseField: four int32 a source: i, j, k and the weight";
        return RTO_E_INVALID;
    }
    if (m_numNodes > 0 && !makeGridResident("dose field")) return RTO_E_HIP;
    const int rc = api().dose_field(m_ctx, sources.empty() ? nullptr : sources.data(), (int)(sources.size() / 4), transmit.empty() ? nullptr : transmit.data(),
                                    (int)transmit.size(), falloff, mode, reach, summary);
    if (rc != RTO_OK) return regionFailed(rc, "doseField");
    m_doseSources = (int)(sources.size() / 4);
    return RTO_OK;
}

// The resident dose field, downloaded.
int RayTracerBVH::dose(std::vector<int32_t>& e) {
    e.clear();
    if (!computeUsable("dose")) return RTO_E_INVALID;
    e.resize((size_t)m_grid.dimX * m_grid.dimY * m_grid.dimZ);
    const int rc = api().download_dose(m_ctx, e.data(), (int64_t)e.size());
    if (rc != RTO_OK) { e.clear(); return regionFailed(rc, "dose"); }
    return RTO_OK;
}

// The resident dose field's coverage table, downloaded: one count per source of the last doseField.
int RayTracerBVH::doseCoverage(std::vector<int64_t>& covered) {
    covered.clear();
    if (!computeUsable("doseCoverage")) return RTO_E_INVALID;
    covered.resize((size_t)RTO_DOSE_MAX_SOURCES);
    const int rc = api().download_dose_coverage(m_ctx, covered.data(), (int64_t)covered.size());
    if (rc != RTO_OK) { covered.clear(); return regionFailed(rc, "doseCoverage"); }
    covered.resize((size_t)m_doseSources);
    return RTO_OK;
}

// The voxel of the resident dose field with the largest value, the smallest linear index among equals.
int RayTracerBVH::hottestVoxel(int32_t ijk[3], int32_t* value) {
    std::vector<int32_t> e;
    const int rc = dose(e);
    if (rc != RTO_OK) return rc;
    const auto top = std::max_element(e.begin(), e.end());              // the first of equals
    if (top == e.end() || *top < 0) {
        m_lastError = "hottestVoxel: the dose field evaluates no voxel";
        return RTO_E_INVALID;
    }
    const int64_t v = top - e.begin();
    ijk[0] = (int32_t)(v % m_grid.dimX); ijk[1] = (int32_t)(v / m_grid.dimX % m_grid.dimY); ijk[2] = (int32_t)(v / m_grid.dimX / m_grid.dimY);
    if (value) *value = *top;
    return RTO_OK;
}

// The part segmentation of the first GPU's resident grid (rto_segment_parts); the code is RTO_OK or the refusal's.
int RayTracerBVH::segmentParts(int set, int connectivity, int ratio, std::vector<int32_t>* labels, rto_parts_summary* summary) {
    return fieldInto("segmentParts", "part segmentation", labels, [&] { return api().segment_parts(m_ctx, set, connectivity, ratio, summary); },
                     api().download_part_labels);
}

// A resident table of the last segmentParts, downloaded: the count first, then the records.
template <class Record>
static int downloadPartsTable(rto_context* ctx, int (*download)(rto_context*, Record*, int64_t, int64_t*), std::vector<Record>& table) {
    int64_t count = 0;
    int rc = download(ctx, nullptr, 0, &count);
    if (rc == RTO_OK && count > 0) {
        table.resize((size_t)count);
        rc = download(ctx, table.data(), count, &count);
    }
    if (rc != RTO_OK) table.clear();
    return rc;
}

int RayTracerBVH::parts(std::vector<rto_part>& table) {
    table.clear();
    if (!computeUsable("parts")) return RTO_E_INVALID;
    const int rc = downloadPartsTable(m_ctx, api().download_parts, table);
    return rc == RTO_OK ? RTO_OK : regionFailed(rc, "parts");
}

int RayTracerBVH::necks(std::vector<rto_neck>& table) {
    table.clear();
    if (!computeUsable("necks")) return RTO_E_INVALID;
    const int rc = downloadPartsTable(m_ctx, api().download_necks, table);
    return rc == RTO_OK ? RTO_OK : regionFailed(rc, "necks");
}

int RayTracerBVH::partLabels(std::vector<int32_t>& labels) {
    labels.clear();
    if (!computeUsable("partLabels")) return RTO_E_INVALID;
    labels.resize((size_t)m_grid.dimX * m_grid.dimY * m_grid.dimZ);
    const int rc = api().download_part_labels(m_ctx, labels.data(), (int64_t)labels.size());
    if (rc != RTO_OK) { labels.clear(); return regionFailed(rc, "partLabels"); }
    return RTO_OK;
}

// rto_edit_parts on every GPU: the number of voxels flipped, or the refusal's code (negative).
int64_t RayTracerBVH::splitAtNecks(int set, int connectivity, int ratio) {
    m_lastEditChanged = -1;
    if (!computeUsable("splitAtNecks")) return RTO_E_INVALID;
    if (m_numNodes > 0 && !makeGridResident("splitAtNecks")) return RTO_E_HIP;
    int64_t changed = 0;
    for (rto_context* c : m_ctxs) {
        const int rc = api().edit_parts(c, set, connectivity, ratio, c == m_ctx ? &changed : nullptr);
        if (rc != RTO_OK) {
            m_lastError = api().last_error(c);
            std::cerr << "[RayTracerBVH] splitAtNecks failed: " << m_lastError << std::endl;
            return rc;
        }
    }
    m_lastEditChanged = changed;
    if (changed > 0) {
        rto_octree_info info;
        if (api().octree_info(m_ctx, &info) == RTO_OK) m_numNodes = static_cast<int>(info.num_nodes);
        m_gridStale = true;
    }
    return changed;
}

// The local thickness field of the first GPU's resident grid (rto_thickness_field); the code is RTO_OK or the refusal's.
int RayTracerBVH::thicknessField(int medium, float maxRadius, std::vector<int32_t>* t2, rto_thick_summary* summary) {
    return fieldInto("thicknessField", "thickness field", t2, [&] { return api().thickness_field(m_ctx, medium, maxRadius, summary); },
                     api().download_thickness);
}

int RayTracerBVH::thinnestPoint(int medium, float maxRadius, ThinnestPoint& out) {
    out = ThinnestPoint();
    rto_thick_summary s;
    const int rc = thicknessField(medium, maxRadius, nullptr, &s);
    if (rc != RTO_OK) return rc;
    if (s.medium == 0) return RTO_OK;                                   // no voxel of the medium to measure
    out.found = true;
    out.i = (int)(s.argmin % m_grid.dimX); out.j = (int)((s.argmin / m_grid.dimX) % m_grid.dimY); out.k = (int)(s.argmin / ((int64_t)m_grid.dimX * m_grid.dimY));
    out.t2 = s.min_t2;
    out.thin = s.thin;
    out.width = 2.0 * std::sqrt((double)s.min_t2) * (double)m_grid.voxelSize;
    return RTO_OK;
}

// The histogram of the last thicknessField (rto_thickness_histogram): c + 1 bins; empty with the refusal's code when none is resident.
int RayTracerBVH::thicknessHistogram(std::vector<int64_t>& bins) {
    bins.clear();
    if (!computeUsable("thicknessHistogram")) return RTO_E_INVALID;
    int64_t count = 0;
    int rc = api().thickness_histogram(m_ctx, nullptr, 0, &count);
    if (rc == RTO_OK) {
        bins.assign((size_t)count, 0);
        rc = api().thickness_histogram(m_ctx, bins.data(), count, nullptr);
    }
    if (rc != RTO_OK) { bins.clear(); return regionFailed(rc, "thicknessHistogram"); }
    return RTO_OK;
}

// The measures of the first GPU's resident grid (rto_measure_components): labels `set` under `connectivity` afresh, then measures
// that labelling; the code is RTO_OK or the refusal's.
int RayTracerBVH::measureComponents(int set, int connectivity, std::vector<rto_measure>* table, rto_measure* total) {
    if (table) table->clear();
    if (!computeUsable("measureComponents")) return RTO_E_INVALID;
    if (m_numNodes > 0 && !makeGridResident("component measures")) return RTO_E_HIP;
    int64_t count = 0;
    int rc = api().label_components(m_ctx, set, connectivity, &count);
    if (rc == RTO_OK) rc = api().measure_components(m_ctx, total);
    if (rc == RTO_OK && table && count > 0) {
        table->resize((size_t)count);
        rc = api().download_measures(m_ctx, table->data(), count, nullptr);
        if (rc != RTO_OK) table->clear();
    }
    if (rc != RTO_OK) return regionFailed(rc, "measureComponents");
    return RTO_OK;
}

int RayTracerBVH::surfaceArea(int set, double& area) {
    area = 0.0;
    rto_measure t;
    const int rc = measureComponents(set, RTO_CONN_FACE, nullptr, &t);
    if (rc != RTO_OK) return rc;
    int64_t faces = 0;
    for (int d = 0; d < 6; d++) faces += t.faces[d];
    area = (double)faces * (double)m_grid.voxelSize * (double)m_grid.voxelSize;
    return RTO_OK;
}

int RayTracerBVH::centroid(int set, Centroid& out) {
    out = Centroid();
    rto_measure t;
    const int rc = measureComponents(set, RTO_CONN_FACE, nullptr, &t);
    if (rc != RTO_OK) return rc;
    if (t.voxels == 0) return RTO_OK;                                   // no voxel of the set to weigh
    const double mins[3] = { (double)m_grid.minX, (double)m_grid.minY, (double)m_grid.minZ };
    out.found = true;
    out.voxels = t.voxels;
    for (int a = 0; a < 3; a++) out.p[a] = mins[a] + ((double)t.sum[a] / (double)t.voxels + 0.5) * (double)m_grid.voxelSize;
    return RTO_OK;
}

// Cavities first (the complement's components under the dual connectivity that touch no grid face), then the set's pieces, then
// tunnels = pieces + cavities - euler.  The set's labels and measures stay resident.
int RayTracerBVH::topology(int set, int connectivity, Topology& out) {
    out = Topology();
    if (!computeUsable("topology")) return RTO_E_INVALID;
    if (m_numNodes > 0 && !makeGridResident("topology")) return RTO_E_HIP;
    // an unknown set or connectivity goes through as it is: the library refuses it with its message
    const int other = set == RTO_SET_SOLID ? RTO_SET_EMPTY : (set == RTO_SET_EMPTY ? RTO_SET_SOLID : set);
    const int dual = connectivity == RTO_CONN_FACE ? RTO_CONN_FULL : (connectivity == RTO_CONN_FULL ? RTO_CONN_FACE : connectivity);
    int64_t count = 0;
    std::vector<rto_component> outside;
    int rc = api().label_components(m_ctx, other, dual, &count);
    if (rc == RTO_OK && count > 0) {
        outside.resize((size_t)count);
        rc = api().download_components(m_ctx, outside.data(), count, &count);
    }
    if (rc != RTO_OK) return regionFailed(rc, "topology");
    int64_t cavities = 0;
    for (const rto_component& c : outside) cavities += c.touches == 0 ? 1 : 0;
    rto_measure t;
    rc = api().label_components(m_ctx, set, connectivity, &count);
    if (rc == RTO_OK) rc = api().measure_components(m_ctx, &t);
    if (rc != RTO_OK) return regionFailed(rc, "topology");
    out.pieces = count;
    out.cavities = cavities;
    out.tunnels = count + cavities - t.euler;
    return RTO_OK;
}

bool RayTracerBVH::loadMesh(const double* xyz, int64_t nVerts, const int32_t* tris, int64_t nTris, float voxelSize, int recenterPasses,
                            bool triangles) {
    if (!m_computeInited) ensureComputeInitialized();
    if (!m_computeOk) {
        std::cerr << "[RayTracerBVH] Compute pipeline not initialized or failed.\n";
        return false;
    }
    rto_voxelize_params p;
    std::memset(&p, 0, sizeof p);
    p.mode = RTO_VOXELIZE_AUTO;
    p.voxel_size = voxelSize;
    p.recenter_passes = recenterPasses;
    p.triangles = triangles ? 1 : 0;
    rto_voxelize_result r;
    if (!forEachContext([&](rto_context* c) { return api().voxelize_mesh(c, xyz, nVerts, tris, nTris, &p, c == m_ctx ? &r : nullptr); },
                        "mesh voxelization"))
        return false;
    m_octreeRoot = nullptr;
    m_flatNodes.clear();
    m_grid.dimX = r.dims[0]; m_grid.dimY = r.dims[1]; m_grid.dimZ = r.dims[2];
    m_grid.minX = r.grid_min[0]; m_grid.minY = r.grid_min[1]; m_grid.minZ = r.grid_min[2];
    m_grid.voxelSize = r.voxel_size;
    m_grid.data.assign((size_t)r.dims[0] * r.dims[1] * r.dims[2], VoxelState::EMPTY);
    m_gridStale = true;                 // grid() fetches the voxels when asked
    rto_octree_info info;
    if (api().octree_info(m_ctx, &info) == RTO_OK) m_numNodes = static_cast<int>(info.num_nodes);
    return true;
}

const VoxelGrid& RayTracerBVH::grid() const {
    if (m_gridStale && m_ctx) {
        int dims[3] = { 0, 0, 0 };
        static_assert(sizeof(VoxelState) == 1, "VoxelGrid.data is one byte per voxel");
        if (api().download_voxels(m_ctx, reinterpret_cast<uint8_t*>(m_grid.data.data()), (int64_t)m_grid.data.size(), dims) == RTO_OK)
            m_gridStale = false;
        else {
            m_lastError = api().last_error(m_ctx);
            std::cerr << "[RayTracerBVH] grid download failed: " << m_lastError << std::endl;
        }
    }
    return m_grid;
}
