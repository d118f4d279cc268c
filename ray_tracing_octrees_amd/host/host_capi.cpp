// host_capi.cpp -- extern "C" doors onto the C++ host layer so Python (tests, bench.py) can drive the
// same classes a C++ application would: VoxelGrid / createOctreeFromVoxelGrid / Camera / Frustum /
// CacheUtils / RayTracerBVH.  Pure plumbing; no algorithm lives here.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>

#include "BuildingLoader.h"
#include "CacheUtils.h"
#include "Components.h"
#include "Distance.h"
#include "DualContouring.h"
#include "Geodesic.h"
#include "Skeleton.h"
#include "Dose.h"
#include "Exposure.h"
#include "Thickness.h"
#include "Parts.h"
#include "Measure.h"
#include "MarchingCubes.h"
#include "Composite.h"
#include "Projection.h"
#include "Camera.h"
#include "Frustum.h"
#include "OctreeVoxel.h"
#include "RayTracerBVH.h"
#include "Renderer.h"

extern "C" {

// ---------------------------------------------------------------- VoxelGrid
VoxelGrid* rtoh_grid_new(int dx, int dy, int dz, float minx, float miny, float minz, float voxelSize, const uint8_t* data) {
    VoxelGrid* g = new VoxelGrid();
    g->dimX = dx; g->dimY = dy; g->dimZ = dz;
    g->minX = minx; g->minY = miny; g->minZ = minz;
    g->voxelSize = voxelSize;
    const size_t n = (size_t)dx * dy * dz;
    g->data.resize(n);
    if (data) for (size_t i = 0; i < n; i++) g->data[i] = data[i] ? VoxelState::FILLED : VoxelState::EMPTY;
    return g;
}
VoxelGrid* rtoh_grid_test_sphere(int dim) { return new VoxelGrid(makeTestSphereGrid(dim)); }
VoxelGrid* rtoh_grid_load(const char* path) {
    VoxelGrid* g = new VoxelGrid();
    if (!loadVoxelGrid(path, *g)) { delete g; return nullptr; }
    return g;
}
VoxelGrid* rtoh_grid_load_partial(const char* path, int startLayer, int numLayers) {
    VoxelGrid* g = new VoxelGrid();
    if (!loadVoxelGridPartial(path, *g, startLayer, numLayers)) { delete g; return nullptr; }
    return g;
}
int rtoh_grid_save(const VoxelGrid* g, const char* path) { return saveVoxelGrid(path, *g) ? 1 : 0; }
void rtoh_grid_free(VoxelGrid* g) { delete g; }
void rtoh_grid_info(const VoxelGrid* g, int dims[3], float mn[3], float* voxelSize) {
    dims[0] = g->dimX; dims[1] = g->dimY; dims[2] = g->dimZ;
    mn[0] = g->minX; mn[1] = g->minY; mn[2] = g->minZ;
    *voxelSize = g->voxelSize;
}
void rtoh_grid_data(const VoxelGrid* g, uint8_t* out) {
    for (size_t i = 0; i < g->data.size(); i++) out[i] = (uint8_t)g->data[i];
}
int64_t rtoh_grid_count(const VoxelGrid* g) { return (int64_t)g->data.size(); }
int rtoh_grid_recenter(VoxelGrid* g) { return recenterFilledVoxels(*g) ? 1 : 0; }
// loadCSVDataIntoVoxelGrid (host/BuildingLoader.h): voxelized on GPU 0
VoxelGrid* rtoh_grid_load_csv(const char* verts, const char* faces, float voxelSize) {
    return new VoxelGrid(loadCSVDataIntoVoxelGrid(verts, faces, voxelSize));
}
int rtoh_get_voxel_safe(const VoxelGrid* g, int x, int y, int z) { return (int)getVoxelSafe(*g, x, y, z); }

// ---------------------------------------------------------------- octree
OctreeNode* rtoh_octree_build(const VoxelGrid* g) { return createOctreeFromVoxelGrid(*g); }
void rtoh_octree_free(OctreeNode* root) { freeOctree(root); }
int64_t rtoh_octree_map_size() { return (int64_t)g_octreeMap.size(); }
// flatten into caller memory; returns the node count (call with out == NULL to size the buffer)
int64_t rtoh_octree_flatten(const OctreeNode* root, GPUNodes* out, int64_t capacity) {
    const std::vector<GPUNodes> flat = RayTracerBVH::flatten(root);
    if (out && capacity >= (int64_t)flat.size()) std::memcpy(out, flat.data(), flat.size() * sizeof(GPUNodes));
    return (int64_t)flat.size();
}
int rtoh_octree_neighbors(const VoxelGrid* g, int x, int y, int z, int size, int* outXYZS /* 6*4 */) {
    (void)g; (void)size;
    auto it = g_octreeMap.find(buildKey(x, y, z));
    if (it == g_octreeMap.end()) return -1;
    const std::vector<OctreeNode*> nb = getNeighbors(it->second, g_octreeMap);
    for (size_t i = 0; i < nb.size() && i < 6; i++) {
        outXYZS[i * 4 + 0] = nb[i]->x; outXYZS[i * 4 + 1] = nb[i]->y; outXYZS[i * 4 + 2] = nb[i]->z; outXYZS[i * 4 + 3] = nb[i]->size;
    }
    return (int)nb.size();
}

// localMC / MarchingCubesRenderer: 18 floats per triangle (v0,v1,v2, n0,n1,n2); call with out == NULL to size
static int64_t copy_tris(const std::vector<MCTriangle>& tris, float* out, int64_t capacityTris) {
    if (out && capacityTris >= (int64_t)tris.size())
        for (size_t i = 0; i < tris.size(); i++)
            for (int v = 0; v < 3; v++)
                for (int a = 0; a < 3; a++) {
                    out[i * 18 + v * 3 + a] = tris[i].v[v][a];
                    out[i * 18 + 9 + v * 3 + a] = tris[i].normal[v][a];
                }
    return (int64_t)tris.size();
}
int64_t rtoh_local_mc(const VoxelGrid* g, int x0, int y0, int z0, int size, float* out, int64_t capacityTris) {
    return copy_tris(localMC(*g, x0, y0, z0, size), out, capacityTris);
}
int64_t rtoh_mc_renderer(const OctreeNode* root, const VoxelGrid* g, float* out, int64_t capacityTris) {
    MarchingCubesRenderer r;
    return copy_tris(r.render(root, *g, root ? root->x : 0, root ? root->y : 0, root ? root->z : 0, root ? root->size : 0), out, capacityTris);
}

// VoxelCubeRenderer over the whole tree, and renderOctree's walk (kind 0: MarchingCubesRenderer, 1: VoxelCubeRenderer) over
// caller-supplied planes (NULL: nothing culled) or a camera's own frustum; 18 floats per triangle as above
int64_t rtoh_cube_renderer(const OctreeNode* root, const VoxelGrid* g, float* out, int64_t capacityTris) {
    VoxelCubeRenderer r;
    return copy_tris(r.render(root, *g, root ? root->x : 0, root ? root->y : 0, root ? root->z : 0, root ? root->size : 0), out, capacityTris);
}
int64_t rtoh_render_octree_planes(const OctreeNode* root, const VoxelGrid* g, int kind, const float* planes, float margin, float* out,
                                  int64_t capacityTris) {
    MarchingCubesRenderer mc;
    VoxelCubeRenderer vc;
    Renderer& r = kind == 0 ? static_cast<Renderer&>(mc) : static_cast<Renderer&>(vc);
    return copy_tris(renderOctreePlanes(root, *g, r, planes, margin), out, capacityTris);
}
// the same walk timed where it runs, as the reference times its own (main.cpp prints renderOctree's milliseconds): returns the
// milliseconds of one walk, the list's length in *numTris; nothing is copied
double rtoh_render_octree_planes_ms(const OctreeNode* root, const VoxelGrid* g, int kind, const float* planes, float margin, int64_t* numTris) {
    MarchingCubesRenderer mc;
    VoxelCubeRenderer vc;
    Renderer& r = kind == 0 ? static_cast<Renderer&>(mc) : static_cast<Renderer&>(vc);
    const auto t0 = std::chrono::steady_clock::now();
    const std::vector<MCTriangle> tris = renderOctreePlanes(root, *g, r, planes, margin);
    const auto t1 = std::chrono::steady_clock::now();
    if (numTris) *numTris = (int64_t)tris.size();
    return std::chrono::duration<double, std::milli>(t1 - t0).count();
}
int64_t rtoh_render_octree(const OctreeNode* root, const VoxelGrid* g, int kind, const Camera* cam, float aspect, float margin, float* out,
                           int64_t capacityTris) {
    MarchingCubesRenderer mc;
    VoxelCubeRenderer vc;
    Renderer& r = kind == 0 ? static_cast<Renderer&>(mc) : static_cast<Renderer&>(vc);
    return copy_tris(renderOctree(root, *g, r, *cam, aspect, margin), out, capacityTris);
}

// leaf-triangle buffer for the triangle ray path: returns the triangle count; call with tris == NULL to size
int64_t rtoh_build_leaf_triangles(const VoxelGrid* g, const GPUNodes* nodes, int64_t n, float* tris, int64_t capacityTris, int32_t* triOffset) {
    std::vector<float> t;
    std::vector<int32_t> off;
    buildLeafTriangles(*g, GPUNodesView{ reinterpret_cast<const int32_t*>(nodes), n }, t, off);
    const int64_t count = (int64_t)(t.size() / 12);
    if (tris && capacityTris >= count && triOffset) {
        std::memcpy(tris, t.data(), t.size() * sizeof(float));
        std::memcpy(triOffset, off.data(), off.size() * sizeof(int32_t));
    }
    return count;
}

// ---------------------------------------------------------------- Camera
Camera* rtoh_camera_new(float theta, float phi, float radius) { return new Camera(theta, phi, radius); }
void rtoh_camera_free(Camera* c) { delete c; }
void rtoh_camera_pan(Camera* c, float dx, float dy) { c->pan(dx, dy); }
void rtoh_camera_increment(Camera* c, float dTheta, float dPhi, float dR) {
    c->incrementTheta(dTheta); c->incrementPhi(dPhi); c->incrementR(dR);
}
void rtoh_camera_set_target(Camera* c, const float t[3]) { c->setTarget(rtmath::vec3(t[0], t[1], t[2])); }
void rtoh_camera_get(const Camera* c, float view[16], float pos[3], float target[3], float tpr[3]) {
    const rtmath::mat4 v = c->getView();
    std::memcpy(view, v.data(), 64);
    const rtmath::vec3 p = c->getPos();
    pos[0] = p.x; pos[1] = p.y; pos[2] = p.z;
    target[0] = c->target.x; target[1] = c->target.y; target[2] = c->target.z;
    tpr[0] = c->theta; tpr[1] = c->phi; tpr[2] = c->radius;
}

// ---------------------------------------------------------------- math / frustum
void rtoh_mat4_inverse(const float m[16], float out[16]) { std::memcpy(out, rtmath::inverse(rtmath::mat4::from(m)).data(), 64); }
void rtoh_mat4_mul(const float a[16], const float b[16], float out[16]) {
    std::memcpy(out, (rtmath::mat4::from(a) * rtmath::mat4::from(b)).data(), 64);
}
void rtoh_perspective(float fovyRad, float aspect, float zn, float zf, float out[16]) {
    std::memcpy(out, rtmath::perspective(fovyRad, aspect, zn, zf).data(), 64);
}
float rtoh_radians(float deg) { return rtmath::radians(deg); }
void rtoh_frustum_test(const float vp[16], const float* mins, const float* maxs, int64_t n, float margin, int32_t* out) {
    const Frustum fr(rtmath::mat4::from(vp));
    for (int64_t i = 0; i < n; i++)
        out[i] = fr.testAABB(rtmath::vec3(mins[3 * i], mins[3 * i + 1], mins[3 * i + 2]),
                             rtmath::vec3(maxs[3 * i], maxs[3 * i + 1], maxs[3 * i + 2]), margin);
}

// ---------------------------------------------------------------- RayTracerBVH
RayTracerBVH* rtoh_rt_new(int device) {
    RayTracerBVH* rt = new RayTracerBVH();
    rt->setDevice(device);
    return rt;
}
void rtoh_rt_free(RayTracerBVH* rt) { delete rt; }
void rtoh_rt_set_devices(RayTracerBVH* rt, int n, int bandRows) { rt->setDevices(n, bandRows); }
void rtoh_rt_ensure_compute_initialized(RayTracerBVH* rt) { rt->ensureComputeInitialized(); }
void rtoh_rt_set_octree(RayTracerBVH* rt, OctreeNode* root, const VoxelGrid* g) { rt->setOctree(root, *g); }
void rtoh_rt_set_octree_from_grid(RayTracerBVH* rt, const VoxelGrid* g) { rt->setOctreeFromGrid(*g); }
void rtoh_rt_set_frustum_culling_enabled(RayTracerBVH* rt, int enabled) { rt->setFrustumCullingEnabled(enabled != 0); }
void rtoh_rt_render_scene_compute(RayTracerBVH* rt, const Camera* cam, int w, int h, float aspect, float fovDeg) {
    rt->renderSceneCompute(*cam, w, h, aspect, fovDeg);
}
void rtoh_rt_render_scene_compute_with_culling(RayTracerBVH* rt, const Camera* cam, int w, int h, float aspect,
                                               float fovDeg, int updateFrustum) {
    rt->renderSceneComputeWithCulling(*cam, w, h, aspect, fovDeg, updateFrustum != 0);
}
void rtoh_rt_build_leaf_triangles(RayTracerBVH* rt) { rt->buildLeafTriangles(); }
void rtoh_rt_build_leaf_triangles_on_host(RayTracerBVH* rt) { rt->buildLeafTrianglesOnHost(); }
void rtoh_rt_render_scene_triangles(RayTracerBVH* rt, const Camera* cam, int w, int h, float aspect, float fovDeg, int shadow) {
    rt->renderSceneTriangles(*cam, w, h, aspect, fovDeg, shadow != 0);
}
void rtoh_rt_render_scene_lit(RayTracerBVH* rt, const Camera* cam, int w, int h, float aspect, float fovDeg, const float lightDir[3],
                              int shadow, int aoSamples, float aoRadius, uint32_t seed) {
    Lighting L;
    L.lightDir = rto_host::vec3(lightDir[0], lightDir[1], lightDir[2]);
    L.shadow = shadow != 0;
    L.aoSamples = aoSamples;
    L.aoRadius = aoRadius;
    L.seed = seed;
    rt->renderSceneLit(*cam, w, h, aspect, fovDeg, L);
}
void rtoh_rt_render_surface_lit(RayTracerBVH* rt, const Camera* cam, int w, int h, float aspect, float fovDeg, const float lightDir[3],
                                int shadow, int aoSamples, float aoRadius, uint32_t seed) {
    Lighting L;
    L.lightDir = rto_host::vec3(lightDir[0], lightDir[1], lightDir[2]);
    L.shadow = shadow != 0;
    L.aoSamples = aoSamples;
    L.aoRadius = aoRadius;
    L.seed = seed;
    rt->renderSurfaceLit(*cam, w, h, aspect, fovDeg, L);
}
int rtoh_rt_render_field(RayTracerBVH* rt, const Camera* cam, int w, int h, float aspect, float fovDeg, const rto_field_view* view,
                         const uint32_t* lut, const int32_t* volume) {
    return rt->renderField(*cam, w, h, aspect, fovDeg, *view, lut, volume);
}
// values: up to `capacity` int32 of the last renderField, row-major; returns how many there are.  summary may be NULL.
int64_t rtoh_rt_field_values(const RayTracerBVH* rt, int32_t* values, int64_t capacity, rto_field_view_summary* summary) {
    const std::vector<int32_t>& v = rt->fieldValues();
    if (values) std::copy(v.begin(), v.begin() + (size_t)std::min<int64_t>((int64_t)v.size(), capacity), values);
    if (summary) *summary = rt->fieldSummary();
    return (int64_t)v.size();
}
int rtoh_rt_project_field(RayTracerBVH* rt, const Camera* cam, int w, int h, float aspect, float fovDeg, const rto_field_projection* proj,
                          const uint32_t* lut, const int32_t* volume) {
    return rt->projectField(*cam, w, h, aspect, fovDeg, *proj, lut, volume);
}
// Up to `capacity` entries each of the last projectField's values, voxels, sums and counts, row-major; returns how many there are.
int64_t rtoh_rt_projection_values(const RayTracerBVH* rt, int32_t* values, int32_t* voxels, int64_t* sums, int32_t* counts, int64_t capacity) {
    const RayTracerBVH::ProjectionValues& p = rt->projectionValues();
    const size_t n = (size_t)std::min<int64_t>((int64_t)p.values.size(), capacity);
    if (values) std::copy(p.values.begin(), p.values.begin() + n, values);
    if (voxels) std::copy(p.voxels.begin(), p.voxels.begin() + n, voxels);
    if (sums) std::copy(p.sums.begin(), p.sums.begin() + n, sums);
    if (counts) std::copy(p.counts.begin(), p.counts.begin() + n, counts);
    return (int64_t)p.values.size();
}
// The CPU form of a projection (host/Projection.h): one ray's visited voxels (x, y, z per voxel, up to `capacity` of them; returns
// how many there are) and the reduction of a volume over such a walk (result: value, voxel, sum, count).
int64_t rtoh_projection_walk(const float gridMin[3], float voxelSize, const int32_t dim[3], const float o[3], const float d[3],
                             const int32_t lo[3], const int32_t hi[3], int32_t* cells, int64_t capacity) {
    const std::vector<rto_host::ProjectionVoxel> w = rto_host::projectionWalk(gridMin, voxelSize, dim, o, d, lo, hi);
    for (size_t i = 0; i < w.size() && (int64_t)i < capacity; i++) { cells[3 * i] = w[i].x; cells[3 * i + 1] = w[i].y; cells[3 * i + 2] = w[i].z; }
    return (int64_t)w.size();
}
void rtoh_projection_reduce(const int32_t* volume, const int32_t dim[3], const int32_t* cells, int64_t n, int op, int32_t validLo,
                            int32_t validHi, int64_t result[4]) {
    static_assert(sizeof(rto_host::ProjectionVoxel) == 12, "x, y, z");
    const rto_host::ProjectionResult r = rto_host::projectionReduce(volume, dim, reinterpret_cast<const rto_host::ProjectionVoxel*>(cells), n,
                                                                    op, validLo, validHi);
    result[0] = r.value; result[1] = r.voxel; result[2] = r.sum; result[3] = r.count;
}
int rtoh_rt_composite_field(RayTracerBVH* rt, const Camera* cam, int w, int h, float aspect, float fovDeg, const rto_field_composite* comp,
                            const uint32_t* lut, const int32_t* volume, const float* under) {
    return rt->compositeField(*cam, w, h, aspect, fovDeg, *comp, lut, volume, under);
}
// Up to `capacity` entries each of the last compositeField's transmittance, first, stops and counts, row-major; returns how many
// there are.  summary may be NULL.
int64_t rtoh_rt_composite_values(const RayTracerBVH* rt, uint32_t* transmittance, int32_t* first, int32_t* stops, int32_t* counts,
                                 int64_t capacity, rto_composite_summary* summary) {
    const RayTracerBVH::CompositeValues& p = rt->compositeValues();
    const size_t n = (size_t)std::min<int64_t>((int64_t)p.counts.size(), capacity);
    if (transmittance) std::copy(p.transmittance.begin(), p.transmittance.begin() + n, transmittance);
    if (first) std::copy(p.first.begin(), p.first.begin() + n, first);
    if (stops) std::copy(p.stops.begin(), p.stops.begin() + n, stops);
    if (counts) std::copy(p.counts.begin(), p.counts.begin() + n, counts);
    if (summary) *summary = rt->compositeSummary();
    return (int64_t)p.counts.size();
}
// The CPU form of a composite (host/Composite.h).  One ray: a walk of rtoh_projection_walk composited under comp; grid: the
// resident bytes (read with comp->occlude), under: the pixel below or NULL; result: T, R, G, B, first, stop, count, end; rgba: the
// pixel's colour (n == 0 is a miss).
void rtoh_composite_ray(const int32_t* volume, const uint8_t* grid, const int32_t dim[3], const int32_t* cells, int64_t n,
                        const rto_field_composite* comp, const uint32_t* lut, const float* under, int64_t result[8], float rgba[4]) {
    const rto_host::CompositeResult r = rto_host::compositeRay(volume, grid, dim, reinterpret_cast<const rto_host::ProjectionVoxel*>(cells), n,
                                                               *comp, lut);
    result[0] = r.T; result[1] = r.R; result[2] = r.G; result[3] = r.B; result[4] = r.first; result[5] = r.stop; result[6] = r.count;
    result[7] = r.end;
    rto_host::compositeColour(r, n > 0, *comp, under, rgba);
}
int rtoh_composite_index(int32_t v, int32_t lo, int32_t hi, int scale) { return rto_host::compositeIndex(v, lo, hi, scale); }
void rtoh_composite_thresholds(int scale, int32_t lo, int32_t hi, uint32_t thr[256]) { rto_host::compositeThresholds(scale, lo, hi, thr); }
int64_t rtoh_rt_num_nodes(const RayTracerBVH* rt) { return (int64_t)rt->numNodes(); }
int rtoh_rt_framebuffer(const RayTracerBVH* rt, float* out, int64_t capacityFloats, int* w, int* h) {
    *w = rt->frameWidth(); *h = rt->frameHeight();
    const std::vector<float>& fb = rt->framebuffer();
    if (fb.empty()) return 0;
    if (out && capacityFloats >= (int64_t)fb.size()) std::memcpy(out, fb.data(), fb.size() * sizeof(float));
    return 1;
}
// rays: n x (ox, oy, oz, dx, dy, dz); hits: n rto_hit records
void rtoh_rt_intersect_rays(RayTracerBVH* rt, const float* rays, int64_t n, int mode, float tMin, float tMax, rto_hit* hits) {
    std::vector<Ray> in((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        in[(size_t)i].origin = rto_host::vec3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]);
        in[(size_t)i].direction = rto_host::vec3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
    }
    std::vector<RayHit> out;
    rt->intersectRays(in, out, mode, tMin, tMax);
    for (int64_t i = 0; i < n; i++) {
        const RayHit& h = out[(size_t)i];
        hits[i] = rto_hit{ h.t, h.node, h.face, h.size, h.x, h.y, h.z, 0 };
    }
}
int rtoh_rt_pick(RayTracerBVH* rt, const Camera* cam, int px, int py, int w, int h, float aspect, float fovDeg, rto_hit* out) {
    RayHit r;
    const bool hit = rt->pick(*cam, px, py, w, h, aspect, fovDeg, r);
    *out = rto_hit{ r.t, r.node, r.face, r.size, r.x, r.y, r.z, 0 };
    return hit ? 1 : 0;
}
static rto_span to_rto_span(const RaySpan& s) {
    return rto_span{ s.length, s.tEnter, s.tExit, s.leaves, s.node, s.face, { 0, 0 } };
}
// rays: n x (ox, oy, oz, dx, dy, dz); spans: n rto_span records
void rtoh_rt_intersect_spans(RayTracerBVH* rt, const float* rays, int64_t n, float tMin, float tMax, rto_span* spans) {
    std::vector<Ray> in((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        in[(size_t)i].origin = rto_host::vec3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]);
        in[(size_t)i].direction = rto_host::vec3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
    }
    std::vector<RaySpan> out;
    rt->intersectSpans(in, out, tMin, tMax);
    for (int64_t i = 0; i < n; i++) spans[i] = to_rto_span(out[(size_t)i]);
}
int rtoh_rt_pick_span(RayTracerBVH* rt, const Camera* cam, int px, int py, int w, int h, float aspect, float fovDeg, rto_span* out) {
    RaySpan r;
    const bool hit = rt->pickSpan(*cam, px, py, w, h, aspect, fovDeg, r);
    *out = to_rto_span(r);
    return hit ? 1 : 0;
}
static rto_tri_hit to_rto_tri_hit(const TriangleHit& h) {
    return rto_tri_hit{ h.t, h.tri, h.node, h.u, h.v, h.normal.x, h.normal.y, h.normal.z };
}
// rays: n x (ox, oy, oz, dx, dy, dz); hits: n rto_tri_hit records; points: n x 3 floats (o + d t; NULL: not wanted)
void rtoh_rt_intersect_triangles(RayTracerBVH* rt, const float* rays, int64_t n, int mode, float tMin, float tMax, rto_tri_hit* hits,
                                 float* points) {
    std::vector<Ray> in((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        in[(size_t)i].origin = rto_host::vec3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]);
        in[(size_t)i].direction = rto_host::vec3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
    }
    std::vector<TriangleHit> out;
    rt->intersectTriangles(in, out, mode, tMin, tMax);
    for (int64_t i = 0; i < n; i++) {
        const TriangleHit& h = out[(size_t)i];
        hits[i] = to_rto_tri_hit(h);
        if (points) { points[3 * i] = h.point.x; points[3 * i + 1] = h.point.y; points[3 * i + 2] = h.point.z; }
    }
}
int rtoh_rt_pick_surface(RayTracerBVH* rt, const Camera* cam, int px, int py, int w, int h, float aspect, float fovDeg, rto_tri_hit* out,
                         float* point) {
    TriangleHit r;
    const bool hit = rt->pickSurface(*cam, px, py, w, h, aspect, fovDeg, r);
    *out = to_rto_tri_hit(r);
    if (point) { point[0] = r.point.x; point[1] = r.point.y; point[2] = r.point.z; }
    return hit ? 1 : 0;
}
// brushes: n x (cx, cy, cz, ex, ey, ez) floats, shapes / ops: n ints each; the number of voxels changed (-1: the edit failed)
int64_t rtoh_rt_edit_voxels(RayTracerBVH* rt, const float* brushes, const int* shapes, const int* ops, int n) {
    std::vector<VoxelBrush> b((size_t)n);
    for (int i = 0; i < n; i++) {
        const float* f = brushes + 6 * i;
        b[(size_t)i] = VoxelBrush{ rto_host::vec3(f[0], f[1], f[2]), rto_host::vec3(f[3], f[4], f[5]), shapes[i], ops[i] };
    }
    rt->editVoxels(b);
    return rt->lastEditChanged();
}
// Connected components.  rtoh_components_cpu: the CPU form of the rule (Components.h) on a grid: labels (dims product int32) and
// table (capacity records) may be NULL; the count, -1 for a refusal.  rtoh_components_select_cpu edits the grid in place.
int64_t rtoh_components_cpu(const VoxelGrid* g, int set, int connectivity, int32_t* labels, rto_component* table, int64_t capacity) {
    std::vector<int32_t> l;
    std::vector<rto_component> t;
    const int64_t n = labelComponentsCPU(*g, set, connectivity, l, t);
    if (n < 0) return n;
    if (labels) std::copy(l.begin(), l.end(), labels);
    if (table) std::copy(t.begin(), t.begin() + (size_t)std::min<int64_t>(n, capacity), table);
    return n;
}
int64_t rtoh_components_select_cpu(VoxelGrid* g, int set, int connectivity, int select, int64_t arg) {
    return applyComponentSelectionCPU(*g, set, connectivity, select, arg);
}
// RayTracerBVH::labelComponents: the count (-1: it failed), table filled up to capacity; rtoh_rt_component_labels: 1 when copied
int64_t rtoh_rt_label_components(RayTracerBVH* rt, int set, int connectivity, rto_component* table, int64_t capacity) {
    const std::vector<rto_component> t = rt->labelComponents(set, connectivity);
    if (rt->lastComponentCount() < 0) return -1;
    if (table) std::copy(t.begin(), t.begin() + (size_t)std::min<int64_t>((int64_t)t.size(), capacity), table);
    return (int64_t)t.size();
}
int rtoh_rt_component_labels(RayTracerBVH* rt, int32_t* out, int64_t capacity) {
    const std::vector<int32_t> l = rt->componentLabels();
    if (l.empty() || (int64_t)l.size() > capacity) return 0;
    std::copy(l.begin(), l.end(), out);
    return 1;
}
int64_t rtoh_rt_remove_debris(RayTracerBVH* rt, int64_t minVoxels, int connectivity) { return rt->removeDebris(minVoxels, connectivity); }
int64_t rtoh_rt_fill_cavities(RayTracerBVH* rt) { return rt->fillCavities(); }
int64_t rtoh_rt_keep_largest(RayTracerBVH* rt, int connectivity) { return rt->keepLargest(connectivity); }
int64_t rtoh_rt_flip_component_at(RayTracerBVH* rt, int i, int j, int k, int set, int connectivity) {
    return rt->flipComponentAt(i, j, k, set, connectivity);
}
// Distance fields.  rtoh_distance_cpu: the CPU form of the rule (Distance.h) on a grid for mq quanta (-1: no cap): d2 (dims product
// int32) and summary may be NULL; 1, or 0 for a refusal.  rtoh_morphology_cpu edits the grid in place (-1: refused).
int rtoh_distance_quantize(float dist, float voxelSize, int64_t* mq) { return quantizeDistanceCPU(dist, voxelSize, *mq) ? 1 : 0; }
int rtoh_distance_cpu(const VoxelGrid* g, int set, int64_t mq, int32_t* d2, rto_dist_summary* summary) {
    std::vector<int32_t> f;
    if (!distanceFieldCPU(*g, set, mq, f, summary)) return 0;
    if (d2) std::copy(f.begin(), f.end(), d2);
    return 1;
}
int64_t rtoh_morphology_cpu(VoxelGrid* g, int op, int64_t rq) { return applyMorphologyCPU(*g, op, rq); }
// RayTracerBVH::distanceField: the class's code; d2 (capacity int32) and summary may be NULL.  rtoh_rt_morphology: changed, or the
// refusal's code.  rtoh_rt_thickest_point: the class's code; out = found, i, j, k, d2 as int64 and the distance.
int rtoh_rt_distance_field(RayTracerBVH* rt, int set, float maxDist, int32_t* d2, int64_t capacity, rto_dist_summary* summary) {
    std::vector<int32_t> f;
    const int rc = rt->distanceField(set, maxDist, d2 ? &f : nullptr, summary);
    if (rc != RTO_OK) return rc;
    if (d2) std::copy(f.begin(), f.begin() + (size_t)std::min<int64_t>((int64_t)f.size(), capacity), d2);
    return RTO_OK;
}
int64_t rtoh_rt_morphology(RayTracerBVH* rt, int op, float radius) {
    switch (op) {
        case RTO_MORPH_DILATE: return rt->dilate(radius);
        case RTO_MORPH_ERODE: return rt->erode(radius);
        case RTO_MORPH_OPEN: return rt->open(radius);
        case RTO_MORPH_CLOSE: return rt->close(radius);
        default: return RTO_E_INVALID;
    }
}
int rtoh_rt_thickest_point(RayTracerBVH* rt, int64_t out[5], double* distance) {
    RayTracerBVH::ThickestPoint t;
    const int rc = rt->thickestPoint(t);
    out[0] = t.found ? 1 : 0; out[1] = t.i; out[2] = t.j; out[3] = t.k; out[4] = t.d2;
    *distance = t.distance;
    return rc;
}
// Local thickness fields.  rtoh_thickness_cpu: the CPU form of the rule (Thickness.h) on a grid for mq quanta: t2 (dims product
// int32), bins (capacity int64, *count = c + 1) and summary may be NULL; the code of rto_thickness_field.
int rtoh_thickness_cpu(const VoxelGrid* g, int medium, int64_t mq, int32_t* t2, int64_t* bins, int64_t capacity, int64_t* count,
                       rto_thick_summary* summary) {
    std::vector<int32_t> f;
    std::vector<int64_t> b;
    const int rc = thicknessFieldCPU(*g, medium, mq, f, b, summary);
    if (rc != RTO_OK) return rc;
    if (t2) std::copy(f.begin(), f.end(), t2);
    if (bins) std::copy(b.begin(), b.begin() + (size_t)std::min<int64_t>((int64_t)b.size(), capacity), bins);
    if (count) *count = (int64_t)b.size();
    return RTO_OK;
}
// RayTracerBVH::thicknessField / thinnestPoint / thicknessHistogram: the class's codes; out = found, i, j, k, t2, thin as int64 and
// the width; bins: capacity int64, *count = the bins there are.
int rtoh_rt_thickness_field(RayTracerBVH* rt, int medium, float maxRadius, int32_t* t2, int64_t capacity, rto_thick_summary* summary) {
    std::vector<int32_t> f;
    const int rc = rt->thicknessField(medium, maxRadius, t2 ? &f : nullptr, summary);
    if (rc != RTO_OK) return rc;
    if (t2) std::copy(f.begin(), f.begin() + (size_t)std::min<int64_t>((int64_t)f.size(), capacity), t2);
    return RTO_OK;
}
int rtoh_rt_thinnest_point(RayTracerBVH* rt, int medium, float maxRadius, int64_t out[6], double* width) {
    RayTracerBVH::ThinnestPoint t;
    const int rc = rt->thinnestPoint(medium, maxRadius, t);
    out[0] = t.found ? 1 : 0; out[1] = t.i; out[2] = t.j; out[3] = t.k; out[4] = t.t2; out[5] = t.thin;
    *width = t.width;
    return rc;
}
int rtoh_rt_thickness_histogram(RayTracerBVH* rt, int64_t* bins, int64_t capacity, int64_t* count) {
    std::vector<int64_t> b;
    const int rc = rt->thicknessHistogram(b);
    if (rc != RTO_OK) return rc;
    if (bins) std::copy(b.begin(), b.begin() + (size_t)std::min<int64_t>((int64_t)b.size(), capacity), bins);
    if (count) *count = (int64_t)b.size();
    return RTO_OK;
}
// Part segmentation.  rtoh_parts_cpu runs the CPU form of the rule (Parts.h) on a grid ONCE and keeps the answer: the handle (NULL
// for a refusal) gives the counts (rtoh_parts_counts: parts, necks) and then the copies (rtoh_parts_copy: labels of dims product
// int32, parts and necks of the counted sizes, the summary; any may be NULL); rtoh_parts_free ends it.  rtoh_parts_split_cpu edits
// the grid in place (the number flipped, -1: refused).
struct RtohParts {
    std::vector<int32_t> labels;
    std::vector<rto_part> parts;
    std::vector<rto_neck> necks;
    rto_parts_summary summary;
};
RtohParts* rtoh_parts_cpu(const VoxelGrid* g, int set, int connectivity, int ratio) {
    RtohParts* r = new RtohParts();
    if (segmentPartsCPU(*g, set, connectivity, ratio, r->labels, r->parts, r->necks, &r->summary) < 0) { delete r; return nullptr; }
    return r;
}
void rtoh_parts_counts(const RtohParts* r, int64_t counts[2]) { counts[0] = (int64_t)r->parts.size(); counts[1] = (int64_t)r->necks.size(); }
void rtoh_parts_copy(const RtohParts* r, int32_t* labels, rto_part* parts, rto_neck* necks, rto_parts_summary* summary) {
    if (labels) std::copy(r->labels.begin(), r->labels.end(), labels);
    if (parts) std::copy(r->parts.begin(), r->parts.end(), parts);
    if (necks) std::copy(r->necks.begin(), r->necks.end(), necks);
    if (summary) *summary = r->summary;
}
void rtoh_parts_free(RtohParts* r) { delete r; }
int64_t rtoh_parts_split_cpu(VoxelGrid* g, int set, int connectivity, int ratio) { return splitAtNecksCPU(*g, set, connectivity, ratio); }
// RayTracerBVH::segmentParts / parts / necks / partLabels / splitAtNecks: the class's codes; the tables are filled up to capacity and
// *count = the records there are.
int rtoh_rt_segment_parts(RayTracerBVH* rt, int set, int connectivity, int ratio, int32_t* labels, int64_t capacity, rto_parts_summary* summary) {
    std::vector<int32_t> l;
    const int rc = rt->segmentParts(set, connectivity, ratio, labels ? &l : nullptr, summary);
    if (rc != RTO_OK) return rc;
    if (labels) std::copy(l.begin(), l.begin() + (size_t)std::min<int64_t>((int64_t)l.size(), capacity), labels);
    return RTO_OK;
}
int rtoh_rt_parts(RayTracerBVH* rt, rto_part* out, int64_t capacity, int64_t* count) {
    std::vector<rto_part> t;
    const int rc = rt->parts(t);
    if (rc != RTO_OK) return rc;
    if (out) std::copy(t.begin(), t.begin() + (size_t)std::min<int64_t>((int64_t)t.size(), capacity), out);
    if (count) *count = (int64_t)t.size();
    return RTO_OK;
}
int rtoh_rt_necks(RayTracerBVH* rt, rto_neck* out, int64_t capacity, int64_t* count) {
    std::vector<rto_neck> t;
    const int rc = rt->necks(t);
    if (rc != RTO_OK) return rc;
    if (out) std::copy(t.begin(), t.begin() + (size_t)std::min<int64_t>((int64_t)t.size(), capacity), out);
    if (count) *count = (int64_t)t.size();
    return RTO_OK;
}
int rtoh_rt_part_labels(RayTracerBVH* rt, int32_t* out, int64_t capacity) {
    std::vector<int32_t> l;
    const int rc = rt->partLabels(l);
    if (rc != RTO_OK) return rc;
    if ((int64_t)l.size() > capacity) return RTO_E_INVALID;
    std::copy(l.begin(), l.end(), out);
    return RTO_OK;
}
int64_t rtoh_rt_split_at_necks(RayTracerBVH* rt, int set, int connectivity, int ratio) { return rt->splitAtNecks(set, connectivity, ratio); }
// Component measures.  rtoh_measure_cpu: the CPU form of the rule (Measure.h) on a label volume of dims[3]: out (capacity records)
// and total may be NULL; the code of rto_measure_components.
int rtoh_measure_cpu(const int* dims, const int32_t* labels, int64_t count, int connectivity, rto_measure* out, int64_t capacity,
                     rto_measure* total) {
    std::vector<rto_measure> t;
    const int rc = measureComponentsCPU(dims[0], dims[1], dims[2], labels, count, connectivity, t, total);
    if (rc != RTO_OK) return rc;
    if (out) std::copy(t.begin(), t.begin() + (size_t)std::min<int64_t>((int64_t)t.size(), capacity), out);
    return RTO_OK;
}
// RayTracerBVH::measureComponents / surfaceArea / centroid / topology: the class's codes; *count = the records there are, out
// filled up to capacity; centroid: out = found, x, y, z as doubles; topology: out = pieces, tunnels, cavities.
int rtoh_rt_measure_components(RayTracerBVH* rt, int set, int connectivity, rto_measure* out, int64_t capacity, int64_t* count,
                               rto_measure* total) {
    std::vector<rto_measure> t;
    const int rc = rt->measureComponents(set, connectivity, &t, total);
    if (rc != RTO_OK) return rc;
    if (out) std::copy(t.begin(), t.begin() + (size_t)std::min<int64_t>((int64_t)t.size(), capacity), out);
    if (count) *count = (int64_t)t.size();
    return RTO_OK;
}
int rtoh_rt_surface_area(RayTracerBVH* rt, int set, double* area) { return rt->surfaceArea(set, *area); }
int rtoh_rt_centroid(RayTracerBVH* rt, int set, double out[4]) {
    RayTracerBVH::Centroid c;
    const int rc = rt->centroid(set, c);
    out[0] = c.found ? 1.0 : 0.0; out[1] = c.p[0]; out[2] = c.p[1]; out[3] = c.p[2];
    return rc;
}
int rtoh_rt_topology(RayTracerBVH* rt, int set, int connectivity, int64_t out[3]) {
    RayTracerBVH::Topology t;
    const int rc = rt->topology(set, connectivity, t);
    out[0] = t.pieces; out[1] = t.tunnels; out[2] = t.cavities;
    return rc;
}
// Skeletons.  rtoh_skeleton_cpu: the CPU form of the rule (Skeleton.h) on a grid: k (dims product int32) and summary may be NULL; the
// code of rto_skeleton_field.  rtoh_skeleton_thin_cpu edits the grid in place (the number flipped, or the refusal's code);
// rtoh_skeleton_simple is the simple-point test of one 27-bit block.
int rtoh_skeleton_cpu(const VoxelGrid* g, int set, int connectivity, int mode, const int64_t* anchors, int64_t n, int64_t maxPasses, int32_t* out,
                      rto_skel_summary* summary) {
    std::vector<int32_t> k;
    const int rc = skeletonFieldCPU(*g, set, connectivity, mode, anchors, n, maxPasses, k, summary);
    if (rc != RTO_OK) return rc;
    if (out) std::copy(k.begin(), k.end(), out);
    return RTO_OK;
}
int64_t rtoh_skeleton_thin_cpu(VoxelGrid* g, int set, int connectivity, int mode, const int64_t* anchors, int64_t n, int64_t maxPasses) {
    return thinCPU(*g, set, connectivity, mode, anchors, n, maxPasses);
}
int rtoh_skeleton_simple(uint32_t mask, int connectivity) { return skeletonSimpleCPU(mask, connectivity) ? 1 : 0; }
// RayTracerBVH::skeletonField / thin / centreline: the class's codes; centreline: *count = the voxels there are, out filled up to
// capacity.
int rtoh_rt_skeleton_field(RayTracerBVH* rt, int set, int connectivity, int mode, const int64_t* anchors, int64_t n, int64_t maxPasses, int32_t* k,
                           int64_t capacity, rto_skel_summary* summary) {
    std::vector<int32_t> f;
    const int rc = rt->skeletonField(set, connectivity, mode, std::vector<int64_t>(anchors, anchors + (n > 0 ? n : 0)), maxPasses, k ? &f : nullptr, summary);
    if (rc != RTO_OK) return rc;
    if (k) std::copy(f.begin(), f.begin() + (size_t)std::min<int64_t>((int64_t)f.size(), capacity), k);
    return RTO_OK;
}
int64_t rtoh_rt_thin(RayTracerBVH* rt, int mode, int64_t maxPasses) { return rt->thin(mode, maxPasses); }
int rtoh_rt_centreline(RayTracerBVH* rt, int64_t a, int64_t b, int64_t* out, int64_t capacity, int64_t* count) {
    std::vector<int64_t> v;
    const int rc = rt->centreline(a, b, v);
    if (rc != RTO_OK) return rc;
    if (out) std::copy(v.begin(), v.begin() + (size_t)std::min<int64_t>((int64_t)v.size(), capacity), out);
    if (count) *count = (int64_t)v.size();
    return RTO_OK;
}
// Exposure fields.  rtoh_exposure_cpu: the CPU form of the rule (Exposure.h) on a grid: e (dims product int32), summary and steps
// may be NULL; the code of rto_exposure_field.  rtoh_rt_exposure_field / rtoh_rt_exposure: RayTracerBVH::exposureField / exposure,
// the class's codes; e is filled up to capacity.
int rtoh_exposure_cpu(const VoxelGrid* g, const int32_t* dirs, const int32_t* weights, int n, int mode, int reach, int32_t* out,
                      rto_expo_summary* summary, int64_t* steps) {
    std::vector<int32_t> e;
    const int rc = exposureFieldCPU(*g, dirs, weights, n, mode, reach, e, summary, steps);
    if (rc != RTO_OK) return rc;
    if (out) std::copy(e.begin(), e.end(), out);
    return RTO_OK;
}
int rtoh_rt_exposure_field(RayTracerBVH* rt, const int32_t* dirs, const int32_t* weights, int n, int mode, int reach, rto_expo_summary* summary) {
    const size_t count = dirs && n > 0 ? (size_t)n : 0;
    return rt->exposureField(std::vector<int32_t>(dirs, dirs + 3 * count), weights ? std::vector<int32_t>(weights, weights + count) : std::vector<int32_t>(),
                             mode, reach, summary);
}
int rtoh_rt_exposure(RayTracerBVH* rt, int32_t* e, int64_t capacity) {
    std::vector<int32_t> f;
    const int rc = rt->exposure(f);
    if (rc != RTO_OK) return rc;
    if (e) std::copy(f.begin(), f.begin() + (size_t)std::min<int64_t>((int64_t)f.size(), capacity), e);
    return RTO_OK;
}
// Dose fields.  rtoh_dose_cpu: the CPU form of the rule (Dose.h) on a grid: e (dims product int32), covered (n int64), summary, steps
// and bad_source may be NULL; the code of rto_dose_field.  rtoh_rt_dose_field / rtoh_rt_dose / rtoh_rt_dose_coverage:
// RayTracerBVH::doseField / dose / doseCoverage, the class's codes; e and covered are filled up to capacity, *count = the sources.
int rtoh_dose_cpu(const VoxelGrid* g, const int32_t* sources, int n, const uint32_t* transmit, int m, int falloff, int mode, int reach, int32_t* out,
                  int64_t* covered, rto_dose_summary* summary, int64_t* steps, int* bad_source) {
    std::vector<int32_t> e;
    std::vector<int64_t> cover;
    const int rc = doseFieldCPU(*g, sources, n, transmit, m, falloff, mode, reach, e, &cover, summary, steps, bad_source);
    if (rc != RTO_OK) return rc;
    if (out) std::copy(e.begin(), e.end(), out);
    if (covered) std::copy(cover.begin(), cover.end(), covered);
    return RTO_OK;
}
int rtoh_rt_dose_field(RayTracerBVH* rt, const int32_t* sources, int n, const uint32_t* transmit, int m, int falloff, int mode, int reach,
                       rto_dose_summary* summary) {
    const size_t count = sources && n > 0 ? (size_t)n : 0;
    if (transmit && m < 1) return RTO_E_INVALID;                        // an empty vector would stand for NULL: line of sight
    return rt->doseField(std::vector<int32_t>(sources, sources + 4 * count),
                         transmit && m > 0 ? std::vector<uint32_t>(transmit, transmit + m) : std::vector<uint32_t>(), falloff, mode, reach, summary);
}
int rtoh_rt_dose(RayTracerBVH* rt, int32_t* e, int64_t capacity) {
    std::vector<int32_t> f;
    const int rc = rt->dose(f);
    if (rc != RTO_OK) return rc;
    if (e) std::copy(f.begin(), f.begin() + (size_t)std::min<int64_t>((int64_t)f.size(), capacity), e);
    return RTO_OK;
}
int rtoh_rt_dose_coverage(RayTracerBVH* rt, int64_t* covered, int64_t capacity, int64_t* count) {
    std::vector<int64_t> t;
    const int rc = rt->doseCoverage(t);
    if (rc != RTO_OK) return rc;
    if (covered) std::copy(t.begin(), t.begin() + (size_t)std::min<int64_t>((int64_t)t.size(), capacity), covered);
    if (count) *count = (int64_t)t.size();
    return RTO_OK;
}
int rtoh_rt_hottest_voxel(RayTracerBVH* rt, int32_t ijk[3], int32_t* value) { return rt->hottestVoxel(ijk, value); }
// Geodesic fields.  rtoh_geodesic_cpu: the CPU form of the rule (Geodesic.h) on a grid: g (dims product int32) and summary may be
// NULL; the code of rto_geodesic_field.  rtoh_geodesic_paths_cpu walks a field of that grid; rtoh_geodesic_flood_cpu edits the grid
// in place (the number flipped, or the refusal's code).
int rtoh_geodesic_cpu(const VoxelGrid* g, int medium, int connectivity, const int64_t* seeds, int64_t n, int64_t limit, int32_t* out,
                      rto_geo_summary* summary) {
    std::vector<int32_t> f;
    const int rc = geodesicFieldCPU(*g, medium, connectivity, seeds, n, limit, f, summary);
    if (rc != RTO_OK) return rc;
    if (out) std::copy(f.begin(), f.end(), out);
    return RTO_OK;
}
int rtoh_geodesic_paths_cpu(const VoxelGrid* g, int connectivity, const int32_t* field, const int64_t* targets, int64_t n, int64_t maxLen,
                            int64_t* outVoxels, int64_t* outLen) {
    if (!field) return RTO_E_INVALID;
    const std::vector<int32_t> f(field, field + (size_t)g->dimX * g->dimY * g->dimZ);
    return geodesicPathsCPU(*g, connectivity, f, targets, n, maxLen, outVoxels, outLen);
}
int64_t rtoh_geodesic_flood_cpu(VoxelGrid* g, int medium, int connectivity, const int64_t* seeds, int64_t n, int64_t limit) {
    return floodGeodesicCPU(*g, medium, connectivity, seeds, n, limit);
}
// RayTracerBVH::geodesicField / pathsTo / floodFrom / farthestPoint: the class's codes; out = found, i, j, k, voxel, g, reached.
int rtoh_rt_geodesic_field(RayTracerBVH* rt, const int64_t* seeds, int64_t n, int medium, int connectivity, int64_t limit, int32_t* g,
                           int64_t capacity, rto_geo_summary* summary) {
    std::vector<int32_t> f;
    const int rc = rt->geodesicField(std::vector<int64_t>(seeds, seeds + (n > 0 ? n : 0)), medium, connectivity, limit, g ? &f : nullptr, summary);
    if (rc != RTO_OK) return rc;
    if (g) std::copy(f.begin(), f.begin() + (size_t)std::min<int64_t>((int64_t)f.size(), capacity), g);
    return RTO_OK;
}
int rtoh_rt_paths_to(RayTracerBVH* rt, const int64_t* targets, int64_t n, int64_t maxLen, int64_t* outVoxels, int64_t* outLen) {
    std::vector<int64_t> voxels, lengths;
    const int rc = rt->pathsTo(std::vector<int64_t>(targets, targets + (n > 0 ? n : 0)), maxLen, voxels, lengths);
    if (rc != RTO_OK) return rc;
    if (outVoxels) std::copy(voxels.begin(), voxels.end(), outVoxels);
    std::copy(lengths.begin(), lengths.end(), outLen);
    return RTO_OK;
}
int64_t rtoh_rt_flood_from(RayTracerBVH* rt, const int64_t* seeds, int64_t n, int medium, int connectivity, int64_t limit) {
    return rt->floodFrom(std::vector<int64_t>(seeds, seeds + (n > 0 ? n : 0)), medium, connectivity, limit);
}
int rtoh_rt_farthest_point(RayTracerBVH* rt, const int64_t* seeds, int64_t n, int medium, int connectivity, int64_t out[7]) {
    RayTracerBVH::FarthestPoint t;
    const int rc = rt->farthestPoint(std::vector<int64_t>(seeds, seeds + (n > 0 ? n : 0)), medium, connectivity, t);
    out[0] = t.found ? 1 : 0; out[1] = t.i; out[2] = t.j; out[3] = t.k; out[4] = t.voxel; out[5] = t.g; out[6] = t.reached;
    return rc;
}
// RayTracerBVH::locate / census / nearestSolid: the C ABI's records back out; each returns the class's code (RTO_OK or the refusal's)
int rtoh_rt_locate(RayTracerBVH* rt, const float* points, int64_t n, rto_point_hit* hits) {
    std::vector<rto_host::vec3> in((size_t)n);
    for (int64_t i = 0; i < n; i++) in[(size_t)i] = rto_host::vec3(points[3 * i], points[3 * i + 1], points[3 * i + 2]);
    std::vector<PointLocation> out;
    const int rc = rt->locate(in, out);
    for (int64_t i = 0; i < n; i++) {
        const PointLocation& o = out[(size_t)i];
        hits[i] = rto_point_hit{ o.node, o.solid ? 1 : 0, o.x, o.y, o.z, o.size, o.depth, 0 };
    }
    return rc;
}
// brushes: n x (cx, cy, cz, ex, ey, ez) floats, shapes: n ints (as rtoh_rt_edit_voxels; the op is ignored)
int rtoh_rt_census(RayTracerBVH* rt, const float* brushes, const int* shapes, int64_t n, rto_region* regions) {
    std::vector<VoxelBrush> b((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const float* f = brushes + 6 * i;
        b[(size_t)i] = VoxelBrush{ rto_host::vec3(f[0], f[1], f[2]), rto_host::vec3(f[3], f[4], f[5]), shapes[i], VoxelBrush::Carve };
    }
    std::vector<RegionCensus> out;
    const int rc = rt->census(b, out);
    for (int64_t i = 0; i < n; i++) {
        const RegionCensus& o = out[(size_t)i];
        regions[i] = rto_region{ o.filled, o.covered, o.solidLeaves, o.firstNode, { 0, 0 } };
    }
    return rc;
}
// distances: n doubles, world units (+inf where dist2 is -1)
int rtoh_rt_nearest_solid(RayTracerBVH* rt, const float* points, int64_t n, float maxDist, rto_nearest* res, double* distances) {
    std::vector<rto_host::vec3> in((size_t)n);
    for (int64_t i = 0; i < n; i++) in[(size_t)i] = rto_host::vec3(points[3 * i], points[3 * i + 1], points[3 * i + 2]);
    std::vector<NearestSolid> out;
    const int rc = rt->nearestSolid(in, out, maxDist);
    for (int64_t i = 0; i < n; i++) {
        const NearestSolid& o = out[(size_t)i];
        res[i] = rto_nearest{ o.dist2, o.node, o.size, { o.cq[0], o.cq[1], o.cq[2] }, 0 };
        distances[i] = o.distance;
    }
    return rc;
}
// the class's current grid (RayTracerBVH::grid()), as rtoh_grid_data: dims only when out is NULL
void rtoh_rt_grid(const RayTracerBVH* rt, int dims[3], uint8_t* out) {
    const VoxelGrid& g = rt->grid();
    dims[0] = g.dimX; dims[1] = g.dimY; dims[2] = g.dimZ;
    if (out) for (size_t i = 0; i < g.data.size(); i++) out[i] = (uint8_t)g.data[i];
}
int rtoh_rt_load_mesh(RayTracerBVH* rt, const double* xyz, int64_t nVerts, const int32_t* tris, int64_t nTris, float voxelSize,
                      int recenterPasses, int triangles) {
    return rt->loadMesh(xyz, nVerts, tris, nTris, voxelSize, recenterPasses, triangles != 0) ? 1 : 0;
}
// RayTracerBVH::extractMesh (cam != NULL) / extractMeshPlanes, once: returns the list and its length; rtoh_tris_take copies it out
// (18 floats per triangle; out may be NULL) and frees it
void* rtoh_rt_extract_mesh(RayTracerBVH* rt, int kind, const Camera* cam, float aspect, const float* planes, float margin, int64_t* numTris) {
    auto* list = new std::vector<MCTriangle>(cam ? rt->extractMesh(kind, *cam, aspect, margin) : rt->extractMeshPlanes(kind, planes, margin));
    *numTris = (int64_t)list->size();
    return list;
}
void rtoh_tris_take(void* list, float* out) {
    auto* tris = static_cast<std::vector<MCTriangle>*>(list);
    if (!tris) return;
    copy_tris(*tris, out, (int64_t)tris->size());
    delete tris;
}
// marchingCubesVolume (host/MarchingCubes.h), once: the list and its length; rtoh_tris_take copies it out and frees it
void* rtoh_marching_cubes_volume(const float* field, int dimX, int dimY, int dimZ, const float origin[3], float spacing, float iso, int64_t* numTris) {
    auto* list = new std::vector<MCTriangle>(marchingCubesVolume(field, dimX, dimY, dimZ, rto_host::vec3(origin[0], origin[1], origin[2]), spacing, iso));
    *numTris = (int64_t)list->size();
    return list;
}
// isoSurfaceVolume, once: a handle to the list and its tri_cell, their length in *numTris, RTO_OK or the refusal's code in *rc;
// rtoh_iso_take copies both out (18 floats and one int32 per triangle; either may be NULL) and frees the handle
struct IsoList {
    std::vector<MCTriangle> tris;
    std::vector<int32_t> cells;
};
void* rtoh_iso_surface_volume(const int32_t* volume, int dimX, int dimY, int dimZ, const float gridMin[3], float voxelSize,
                              const rto_iso_params* params, rto_iso_summary* summary, int* rc, int64_t* numTris) {
    auto* list = new IsoList();
    list->tris = isoSurfaceVolume(volume, dimX, dimY, dimZ, rto_host::vec3(gridMin[0], gridMin[1], gridMin[2]), voxelSize, *params, &list->cells,
                                  summary, rc);
    *numTris = (int64_t)list->tris.size();
    return list;
}
void rtoh_iso_take(void* handle, float* tris, int32_t* cells) {
    auto* list = static_cast<IsoList*>(handle);
    if (!list) return;
    copy_tris(list->tris, tris, (int64_t)list->tris.size());
    if (cells && !list->cells.empty()) std::memcpy(cells, list->cells.data(), list->cells.size() * sizeof(int32_t));
    delete list;
}
// the same, timed where it runs: the milliseconds of one extraction on one core; nothing is copied
double rtoh_iso_surface_volume_ms(const int32_t* volume, int dimX, int dimY, int dimZ, const float gridMin[3], float voxelSize,
                                  const rto_iso_params* params, int64_t* numTris) {
    const auto t0 = std::chrono::steady_clock::now();
    const std::vector<MCTriangle> tris = isoSurfaceVolume(volume, dimX, dimY, dimZ, rto_host::vec3(gridMin[0], gridMin[1], gridMin[2]), voxelSize, *params);
    const auto t1 = std::chrono::steady_clock::now();
    if (numTris) *numTris = (int64_t)tris.size();
    return std::chrono::duration<double, std::milli>(t1 - t0).count();
}
// RayTracerBVH::isoSurface / offsetSurface (source < 0: offsetSurface(level)), once, as rtoh_rt_extract_mesh
void* rtoh_rt_iso_surface(RayTracerBVH* rt, int source, float level, float outside, int pad, const int32_t* volume, int64_t* numTris) {
    auto* list = new std::vector<MCTriangle>(source < 0 ? rt->offsetSurface(level) : rt->isoSurface(source, level, outside, pad != 0, volume));
    *numTris = (int64_t)list->size();
    return list;
}
// dualContourVolume (host/DualContouring.h), once, as rtoh_iso_surface_volume: rtoh_iso_take copies the list out and frees the handle
void* rtoh_dual_contour_volume(const uint8_t* voxels, int dimX, int dimY, int dimZ, const float gridMin[3], float voxelSize,
                               const rto_dc_params* params, rto_dc_summary* summary, int* rc, int64_t* numTris) {
    auto* list = new IsoList();
    list->tris = dualContourVolume(voxels, dimX, dimY, dimZ, rto_host::vec3(gridMin[0], gridMin[1], gridMin[2]), voxelSize, *params, &list->cells,
                                   summary, rc);
    *numTris = (int64_t)list->tris.size();
    return list;
}
// the same, timed where it runs: the milliseconds of one extraction on one core; nothing is copied
double rtoh_dual_contour_volume_ms(const uint8_t* voxels, int dimX, int dimY, int dimZ, const float gridMin[3], float voxelSize,
                                   const rto_dc_params* params, int64_t* numTris) {
    const auto t0 = std::chrono::steady_clock::now();
    const std::vector<MCTriangle> tris = dualContourVolume(voxels, dimX, dimY, dimZ, rto_host::vec3(gridMin[0], gridMin[1], gridMin[2]), voxelSize, *params);
    const auto t1 = std::chrono::steady_clock::now();
    if (numTris) *numTris = (int64_t)tris.size();
    return std::chrono::duration<double, std::milli>(t1 - t0).count();
}
// dualVertexVolume: out holds dimX dimY dimZ rto_dual_vertex
void rtoh_dual_vertex_volume(const uint8_t* voxels, int dimX, int dimY, int dimZ, const float gridMin[3], float voxelSize, rto_dual_vertex* out) {
    const std::vector<rto_dual_vertex> v = dualVertexVolume(voxels, dimX, dimY, dimZ, rto_host::vec3(gridMin[0], gridMin[1], gridMin[2]), voxelSize);
    if (!v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(rto_dual_vertex));
}
// AdaptiveDualContouringRenderer on a grid of bytes: which == 0: dualVertices (out: 4 floats per voxel; *numTris untouched, NULL
// returned); which == 1: render's top-level call, a list for rtoh_tris_take
void* rtoh_adc_render(const uint8_t* voxels, int dimX, int dimY, int dimZ, const float gridMin[3], float voxelSize, int which, float* out,
                      int64_t* numTris) {
    VoxelGrid grid;
    grid.dimX = dimX; grid.dimY = dimY; grid.dimZ = dimZ;
    grid.minX = gridMin[0]; grid.minY = gridMin[1]; grid.minZ = gridMin[2];
    grid.voxelSize = voxelSize;
    grid.data.resize((size_t)dimX * dimY * dimZ);
    for (size_t i = 0; i < grid.data.size(); i++) grid.data[i] = voxels[i] == 1 ? VoxelState::FILLED : VoxelState::EMPTY;
    AdaptiveDualContouringRenderer r;
    if (which == 0) {
        const std::vector<rtmath::vec4> v = r.dualVertices(grid);
        if (!v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(rtmath::vec4));
        return nullptr;
    }
    auto* list = new std::vector<MCTriangle>(r.render(nullptr, grid, 0, 0, 0, grid.dimX));
    *numTris = (int64_t)list->size();
    return list;
}
// RayTracerBVH::dualContour / dualVertices
void* rtoh_rt_dual_contour(RayTracerBVH* rt, const rto_dc_params* params, rto_dc_summary* summary, int64_t* numTris) {
    auto* list = new IsoList();
    list->tris = rt->dualContour(*params, &list->cells, summary);
    *numTris = (int64_t)list->tris.size();
    return list;
}
int rtoh_rt_dual_vertices(RayTracerBVH* rt, const int64_t* voxels, int64_t n, rto_dual_vertex* out) {
    const std::vector<rto_dual_vertex> v = rt->dualVertices(voxels, n);
    if ((int64_t)v.size() != n) return 0;
    if (n > 0) std::memcpy(out, v.data(), (size_t)n * sizeof(rto_dual_vertex));
    return 1;
}
void rtoh_rt_finish(const RayTracerBVH* rt) { rt->finish(); }
void* rtoh_rt_context(const RayTracerBVH* rt) { return rt->context(); }
const char* rtoh_rt_last_error(const RayTracerBVH* rt) { return rt->lastError().c_str(); }

}  // extern "C"
