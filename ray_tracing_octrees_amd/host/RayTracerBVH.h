// RayTracerBVH.h -- drop-in for the reference class of the same name
// (453-skeleton/RayTracerBVH.h:28-80; used at 453-skeleton/main.cpp:1127-1131 and :1357-1363).
// Same public methods, same argument meaning, same error behaviour (void + a line on std::cerr);
// the OpenGL compute dispatch is replaced by hand-written gfx950 kernels behind the C ABI of
// include/rto_hip.h, loaded from librto_hip.so.  If that library or a gfx950 device is missing,
// ensureComputeInitialized() reports it on std::cerr and every render call keeps printing the
// reference's "[RayTracerBVH] Compute pipeline not initialized or failed." -- there is no CPU path.
//
// One addition: the reference leaves the image in a GL texture and never reads it back; here the
// last frame is available through framebuffer() (RGBA32F, row-major, row 0 = top).
#pragma once

#include <limits>
#include <string>
#include <vector>

// "OctreeVoxel.h" / "Camera.h" resolve to this directory's headers by default.  Compiled with
// -DRTO_REFERENCE_HEADERS and the reference's 453-skeleton/ + glm first on the include path, the very same
// class builds against the reference's own OctreeNode / VoxelGrid / Camera (glm types): that is the
// drop-in build INTEGRATION.md describes; the repo's test tree builds and runs exactly that configuration.
#include "rto_hip.h"
#ifdef RTO_REFERENCE_HEADERS
#include <Camera.h>        // angle brackets: taken from the include path (the reference's 453-skeleton/), not from this directory
#include <OctreeVoxel.h>
#include <glm/glm.hpp>
namespace rto_host { using vec3 = glm::vec3; }
#else
#include "Camera.h"
#include "Frustum.h"
#include "OctreeVoxel.h"
#include "rtmath.h"
namespace rto_host { using vec3 = rtmath::vec3; }
#endif

// GPU-side node record, same name and layout as the reference's (RayTracerBVH.h:21-26)
struct GPUNodes {
    int x, y, z, size;
    int isLeaf, isSolid;
    int isUniform;
    int child[8];
};
static_assert(sizeof(GPUNodes) == sizeof(rto_node), "GPUNodes must stay 60 bytes");

struct Ray {
    rto_host::vec3 origin;
    rto_host::vec3 direction;
};

// What a ray query found (the fields of rto_hit, include/rto_hip.h): the accepted solid leaf's index in the resident array, its
// box (voxel units), the ray parameter t of the hit and the entry face (0..5 = 2 * axis + (d[axis] < 0), -1 = none).  A miss has
// node -1 and t 1e30.
struct RayHit {
    float t = 1e30f;
    int node = -1;
    int face = -1;
    int size = 0;
    int x = 0, y = 0, z = 0;
    bool hit() const { return node >= 0; }
};

// What a span query found (the fields of rto_span, include/rto_hip.h): the solid length the ray passes
// through inside its window (units of d), where it first enters and last leaves solid, how many octree leaves it crosses (leaves,
// not walls), and Closest's leaf and entry face.  A miss has length 0, leaves 0, node -1 and tEnter = tExit = 1e30.
struct RaySpan {
    float length = 0.0f;
    float tEnter = 1e30f, tExit = 1e30f;
    int leaves = 0;
    int node = -1;
    int face = -1;
    bool hit() const { return leaves > 0; }
};

// What a triangle query found (the fields of rto_tri_hit, include/rto_hip.h): the accepted triangle's index in the resident
// triangle buffer, the leaf that owns it, the ray parameter t, the hit point o + d t, the barycentrics u, v (the point is
// (1 - u - v) v0 + u v1 + v v2) and the stored face normal turned against the ray.  A miss has tri -1 and t 1e30.
struct TriangleHit {
    float t = 1e30f;
    int tri = -1;
    int node = -1;
    float u = 0.0f, v = 0.0f;
    rto_host::vec3 point = rto_host::vec3(0.0f, 0.0f, 0.0f);
    rto_host::vec3 normal = rto_host::vec3(0.0f, 0.0f, 0.0f);
    bool hit() const { return tri >= 0; }
};

// A voxel edit (rto_brush, include/rto_hip.h): a sphere (radius extent.x) or an axis-aligned box
// (half-sizes extent) in world units that carves voxels (-> EMPTY) or fills them (-> FILLED).
struct VoxelBrush {
    enum Shape { Sphere = RTO_BRUSH_SPHERE, Box = RTO_BRUSH_BOX };
    enum Op { Carve = RTO_EDIT_CARVE, Fill = RTO_EDIT_FILL };
    rto_host::vec3 centre;
    rto_host::vec3 extent;
    int shape;
    int op;
};

// What the region queries answer (rto_point_hit, rto_region, rto_nearest, include/rto_hip.h), exact in
// integers at 1/64 voxel.  PointLocation: the leaf that holds a point (node -1: none, or an invalid point).  RegionCensus: the
// voxels a VoxelBrush covers (its op is ignored) inside the grid and how many of them are solid (both -1: an invalid brush).
// NearestSolid: the nearest solid leaf, the closest point of its box in 1/64-voxel units and the distance in world units
// (dist2 -1 and distance +inf: none within maxDist, or an invalid record).
struct PointLocation {
    int node = -1;
    bool solid = false;
    int x = 0, y = 0, z = 0, size = 0;
    int depth = 0;
    bool found() const { return node >= 0; }
};
struct RegionCensus {
    int64_t filled = -1, covered = -1;
    int solidLeaves = 0;
    int firstNode = -1;
    bool valid() const { return covered >= 0; }
};
struct NearestSolid {
    int64_t dist2 = -1;
    int node = -1;
    int size = 0;
    int cq[3] = { 0, 0, 0 };
    double distance = std::numeric_limits<double>::infinity();
    bool found() const { return dist2 >= 0; }
};

// The lit render's terms (rto_lighting, include/rto_hip.h): the direction the light travels, a shadow ray
// per lit pixel, aoSamples (0..64) ambient-occlusion rays of length aoRadius (world units) per hit pixel, and the hash seed.
struct Lighting {
    rto_host::vec3 lightDir = rto_host::vec3(-1.0f, -1.0f, -1.0f);
    bool shadow = true;
    int aoSamples = 0;
    float aoRadius = 1.0f;
    uint32_t seed = 0;
};

class RayTracerBVH {
public:
    enum QueryMode { First = RTO_QUERY_FIRST, Closest = RTO_QUERY_CLOSEST, Any = RTO_QUERY_ANY };

    RayTracerBVH();
    ~RayTracerBVH();
    RayTracerBVH(const RayTracerBVH&) = delete;
    RayTracerBVH& operator=(const RayTracerBVH&) = delete;

    void setOctree(OctreeNode* root, const VoxelGrid& grid);
    void ensureComputeInitialized();
    void renderSceneCompute(const Camera& camera, int width, int height, float aspect, float fovDeg);
    void setFrustumCullingEnabled(bool enabled) { m_frustumCullingEnabled = enabled; }
    void renderSceneComputeWithCulling(const Camera& camera, int width, int height, float aspect, float fovDeg,
                                       bool updateFrustum);

    // ---- additions (not in the reference) ----
    // createOctreeFromVoxelGrid + setOctree in one step ON THE GPU (rto_build_octree): no pointer tree, no host
    // flatten.  The resident array equals what setOctree(createOctreeFromVoxelGrid(grid), grid) uploads.
    void setOctreeFromGrid(const VoxelGrid& grid);
    // Triangle ray path of BASELINE config 5 (no upstream counterpart): builds, in HBM, the per-leaf Marching-Cubes
    // triangle buffer (what MarchingCubesRenderer::render emits per leaf) from the grid given to setOctree() /
    // setOctreeFromGrid(); then renders with Moeller-Trumbore hits on those triangles and, if `shadow`, one shadow ray
    // per hit.  Same framebuffer() as the other calls.
    void buildLeafTriangles();
    void renderSceneTriangles(const Camera& camera, int width, int height, float aspect, float fovDeg, bool shadow);
#ifndef RTO_REFERENCE_HEADERS   // needs this repo's localMC: the same buffer made on the host and uploaded (cross-check)
    void buildLeafTrianglesOnHost();
#endif
    // Ray queries over the whole resident octree (rto_query_rays_host): one RayHit per Ray, d need not be normalised, t in units
    // of d, hits accepted for tMin <= t <= tMax.  The consumer the reference's struct Ray never had.
    void intersectRays(const std::vector<Ray>& rays, std::vector<RayHit>& hits, int mode = Closest, float tMin = 0.0f,
                       float tMax = 1e30f);
    // renderSceneCompute's frame with a shadow ray and ambient occlusion per hit pixel (rto_render_lit_host): same framebuffer().
    // The whole octree casts shadows, whatever the frustum culling.  With setDevices(n > 1) it renders on the first GPU alone.
    void renderSceneLit(const Camera& camera, int width, int height, float aspect, float fovDeg, const Lighting& lighting);
    // renderSceneTriangles' frame (the leaf triangles' surface) lit the same way (rto_render_lit_triangles_host; DESIGN.md section
    // 14).  Needs buildLeafTriangles(); without triangles resident it fails as intersectTriangles / pickSurface do: no frame, lastError set.
    void renderSurfaceLit(const Camera& camera, int width, int height, float aspect, float fovDeg, const Lighting& lighting);
    // A frame coloured by a per-voxel int32 volume of the resident grid (rto_render_field_host): a resident
    // field, the component labels, or with RTO_FIELD_CALLER `volume` (dimZ x dimY x dimX, x fastest).  lut: 256 entries, bytes
    // r g b a.  RTO_OK, or the refusal's code (lastError); framebuffer() holds the frame, fieldValues() the value under every
    // pixel (RTO_FIELD_PIXEL_MISS / _NONE where there is none), fieldSummary() the frame's counts and range.
    int renderField(const Camera& camera, int width, int height, float aspect, float fovDeg, const rto_field_view& view,
                    const uint32_t* lut, const int32_t* volume = nullptr);
    const std::vector<int32_t>& fieldValues() const { return m_fieldValues; }
    const rto_field_view_summary& fieldSummary() const { return m_fieldSummary; }
    // A frame whose pixels reduce such a volume over the voxels their rays cross in the grid or in the projection's section box
    // (rto_project_field_host): maximum, minimum, mean, count or first value in the window.  Sources, LUT
    // and return value as renderField's; the octree is not walked.  framebuffer() holds the frame, projectionValues() the value,
    // the deciding voxel, the sum and the count under every pixel, fieldSummary() the frame's counts and range.
    struct ProjectionValues {
        std::vector<int32_t> values, voxels, counts;
        std::vector<int64_t> sums;
    };
    int projectField(const Camera& camera, int width, int height, float aspect, float fovDeg, const rto_field_projection& projection,
                     const uint32_t* lut, const int32_t* volume = nullptr);
    const ProjectionValues& projectionValues() const { return m_projection; }
    // A frame in which such a volume is seen through: LUT colour and opacity per valued voxel, composited front to back along the
    // pixel rays and, with composite.occlude, stopped by the grid's solids (rto_composite_field_host).
    // Sources, LUT and return value as renderField's.  under: null, or width * height * 4 floats to composite over.
    // framebuffer() holds the frame, compositeValues() the transmittance, the first contributing voxel, the stopping voxel and
    // the contributions under every pixel, compositeSummary() the frame's counts.
    struct CompositeValues {
        std::vector<uint32_t> transmittance;
        std::vector<int32_t> first, stops, counts;
    };
    int compositeField(const Camera& camera, int width, int height, float aspect, float fovDeg, const rto_field_composite& composite,
                       const uint32_t* lut, const int32_t* volume = nullptr, const float* under = nullptr);
    const CompositeValues& compositeValues() const { return m_composite; }
    const rto_composite_summary& compositeSummary() const { return m_compositeSummary; }
    // The leaf renderSceneCompute shows at pixel (px, py) (row 0 = top) of a width x height frame of that camera: the render's own
    // ray and its FIRST rule (rto_query_pixels_host).  Replaces the reference's intersectBuildingVoxel (main.cpp:209-) in its
    // click handler.  false (and out a miss) when nothing is hit.
    bool pick(const Camera& camera, int px, int py, int width, int height, float aspect, float fovDeg, RayHit& out);
    // Span queries (rto_query_spans_host): one RaySpan per Ray, the solid path length between tMin and tMax.
    // Attenuation between two points: direction = b - a, tMax = 1, exp(-mu * length * |b - a|).  Fails as intersectRays does.
    void intersectSpans(const std::vector<Ray>& rays, std::vector<RaySpan>& spans, float tMin = 0.0f, float tMax = 1e30f);
    // The span of renderSceneCompute's own ray through pixel (px, py) (rto_query_span_pixels_host): thickness under the cursor.
    // false (and out a miss) when the ray meets no solid; fails as pick does.
    bool pickSpan(const Camera& camera, int px, int py, int width, int height, float aspect, float fovDeg, RaySpan& out);
    // The same queries against the resident leaf triangles (rto_query_triangles_host, DESIGN.md section 10 "Triangle queries"):
    // one TriangleHit per Ray.  First is renderSceneTriangles' rule, Closest the nearest surface, Any occlusion (a shadow ray
    // towards a point light: tMax = the distance to it in units of d).
    void intersectTriangles(const std::vector<Ray>& rays, std::vector<TriangleHit>& hits, int mode = Closest, float tMin = 0.0f,
                            float tMax = 1e30f);
    // The triangle renderSceneTriangles shows at pixel (px, py) (row 0 = top): the render's own ray and its FIRST rule
    // (rto_query_triangle_pixels_host), with the surface point, barycentrics and normal.  false (and out a miss) when nothing is hit.
    bool pickSurface(const Camera& camera, int px, int py, int width, int height, float aspect, float fovDeg, TriangleHit& out);
    // Scene edits: the brushes, in order, on the grid every GPU holds; the octree (and the leaf triangles, if resident) is then
    // rebuilt there, as setOctreeFromGrid would build it from the edited grid.  After setOctree() the first edit builds the octree
    // from the grid given to it.  flatNodes() is empty afterwards and buildLeafTriangles() uses the resident grid.  The reference's
    // click-to-carve: pickSurface (or pick), then editVoxels({{hit.point, vec3(r), VoxelBrush::Sphere, VoxelBrush::Carve}}).
    void editVoxels(const std::vector<VoxelBrush>& brushes);
    int64_t lastEditChanged() const { return m_lastEditChanged; }   // voxels the last editVoxels changed; -1: it failed
    // Connected components of the resident grid (rto_label_components / rto_edit_components): set is
    // RTO_SET_SOLID or RTO_SET_EMPTY, connectivity RTO_CONN_FACE (6) or RTO_CONN_FULL (26).  labelComponents labels the grid of the
    // first GPU and returns the table in ascending order of root (empty with lastError set on an error); componentLabels() is that
    // labelling's volume (one int32 per voxel, x fastest, -1 outside the set; empty once the grid has changed).  The edits act on
    // every GPU and rebuild as editVoxels does; each returns the number of voxels flipped, -1 on an error (lastEditChanged() too):
    // removeDebris clears the solid components of fewer than minVoxels voxels, fillCavities fills the empty components that touch
    // no face of the grid (6-connected: what a voxelized closed mesh encloses), keepLargest clears every solid component but the
    // largest, flipComponentAt flips the component of `set` that holds voxel (i, j, k) (0 when that voxel is not in the set).
    // After setOctree() the first of these builds the octree from the grid given to it, as the first editVoxels does.
    std::vector<rto_component> labelComponents(int set = RTO_SET_SOLID, int connectivity = RTO_CONN_FACE);
    int64_t lastComponentCount() const { return m_lastComponents; }   // components the last labelComponents found; -1: it failed
    std::vector<int32_t> componentLabels();
    int64_t removeDebris(int64_t minVoxels, int connectivity = RTO_CONN_FACE);
    int64_t fillCavities();
    int64_t keepLargest(int connectivity = RTO_CONN_FACE);
    int64_t flipComponentAt(int i, int j, int k, int set, int connectivity = RTO_CONN_FACE);
    // Distance fields and morphology of the resident grid (rto_distance_field / rto_edit_morphology).
    // distanceField makes the field of the first GPU's grid: one int32 per voxel, x fastest, the squared distance in voxel-index
    // units to the nearest voxel of `set`, RTO_DIST_NONE beyond maxDist (world units; INFINITY: no cap); d2 and summary may be null.
    // It returns RTO_OK or the refusal's code (lastError).  dilate / erode / open / close move the surface by `radius` (world units)
    // on every GPU and rebuild as editVoxels does; each returns the number of voxels changed (lastEditChanged() too), or the
    // refusal's code, which is negative.  thickestPoint is the FILLED voxel farthest from any EMPTY one (the smallest index among
    // equals) with its distance in world units; found stays false in a grid with no EMPTY or no FILLED voxel.
    // After setOctree() the first of these builds the octree from the grid given to it, as the first editVoxels does.
    struct ThickestPoint { bool found = false; int i = 0, j = 0, k = 0; int64_t d2 = 0; double distance = 0.0; };
    int distanceField(int set, float maxDist, std::vector<int32_t>* d2, rto_dist_summary* summary = nullptr);
    int64_t dilate(float radius);
    int64_t erode(float radius);
    int64_t open(float radius);
    int64_t close(float radius);
    int thickestPoint(ThickestPoint& out);
    // Geodesic fields, paths and flood edits of the resident grid (rto_geodesic_field / rto_geodesic_paths / rto_edit_geodesic;
    // DESIGN.md section 20).  geodesicField makes the field of the first GPU's grid: one int32 per voxel, x fastest, the length of
    // the shortest path inside `medium` from any of `seeds` (linear voxel indices), weight 1 per face move under RTO_CONN_FACE and
    // 3 / 4 / 5 per move under RTO_CONN_FULL, RTO_DIST_NONE outside the medium, out of reach or above `limit` (>= 0x7fffffff: none);
    // g and summary may be null.  pathsTo reads the routes back out of that field: maxLen voxels per target from the target down to a
    // seed, -1 behind the path, and every path's full length (-1: not reached).  floodFrom flips every voxel its own field reaches,
    // on every GPU, and rebuilds as editVoxels does: the number flipped (lastEditChanged() too).  farthestPoint is the reached voxel
    // farthest from the seeds (the smallest index among equals).  Each returns RTO_OK or the refusal's code, which is negative.
    // The CPU form of the same rule for a VoxelGrid is host/Geodesic.h.
    struct FarthestPoint { bool found = false; int i = 0, j = 0, k = 0; int64_t voxel = -1, g = -1, reached = 0; };
    int geodesicField(const std::vector<int64_t>& seeds, int medium, int connectivity, int64_t limit, std::vector<int32_t>* g,
                      rto_geo_summary* summary = nullptr);
    int pathsTo(const std::vector<int64_t>& targets, int64_t maxLen, std::vector<int64_t>& voxels, std::vector<int64_t>& lengths);
    int64_t floodFrom(const std::vector<int64_t>& seeds, int medium, int connectivity = RTO_CONN_FACE, int64_t limit = 0x7fffffffll);
    int farthestPoint(const std::vector<int64_t>& seeds, int medium, int connectivity, FarthestPoint& out);
    // Local thickness fields of the resident grid (rto_thickness_field).  thicknessField makes the field of the
    // first GPU's grid: one int32 per voxel, x fastest, the squared radius in voxel-index units of the largest ball inside `medium`
    // (RTO_SET_SOLID: the material, RTO_SET_EMPTY: the free space) that contains the voxel, for balls up to maxRadius (world units,
    // 1 to 8 voxels), 0 outside the medium; t2 and summary may be null.  thinnestPoint is the medium voxel with the smallest value
    // (the smallest index among equals), the number of voxels thinner than the cap, and the width 2 sqrt(t2) in world units; found
    // stays false in a grid with no voxel of the medium.  thicknessHistogram gives the last field's c + 1 bins.  Each returns
    // RTO_OK or the refusal's code, which is negative (lastError).  Arranged as section 19's methods are: they need the compute
    // pipeline, and the CPU form of the same rule for a VoxelGrid is host/Thickness.h.
    struct ThinnestPoint { bool found = false; int i = 0, j = 0, k = 0; int64_t t2 = 0, thin = 0; double width = 0.0; };
    int thicknessField(int medium, float maxRadius, std::vector<int32_t>* t2, rto_thick_summary* summary = nullptr);
    int thinnestPoint(int medium, float maxRadius, ThinnestPoint& out);
    int thicknessHistogram(std::vector<int64_t>& bins);
    // Skeletons of the resident grid (rto_skeleton_field / rto_edit_skeleton).  skeletonField thins `set` on the
    // first GPU under `connectivity` and `mode` (RTO_SKEL_TOPOLOGY / RTO_SKEL_CURVE): one int32 per voxel, x fastest, -1 outside
    // the set, 0 for the skeleton, p >= 1 for the pass that removed the voxel; `anchors` (linear voxel indices) are never removed;
    // k and summary may be null.  thin replaces the solid by its skeleton under RTO_CONN_FULL on every GPU and rebuilds as
    // editVoxels does: the number of voxels removed (lastEditChanged() too).  centreline gives the voxels, in ascending index order,
    // that are left of the free space under RTO_CONN_FULL and RTO_SKEL_TOPOLOGY with the two anchors held: in a simply connected
    // space the centred curve from one to the other (a space with tunnels keeps its loops as well); the grid is not edited.
    // Each returns RTO_OK or the refusal's code, which is negative (lastError).  They need the compute pipeline; the CPU form of the
    // same rule for a VoxelGrid is host/Skeleton.h.
    int skeletonField(int set, int connectivity, int mode, const std::vector<int64_t>& anchors, int64_t maxPasses, std::vector<int32_t>* k,
                      rto_skel_summary* summary = nullptr);
    int64_t thin(int mode = RTO_SKEL_CURVE, int64_t maxPasses = RTO_SKEL_NO_LIMIT);
    int centreline(int64_t anchorA, int64_t anchorB, std::vector<int64_t>& voxels);
    // Exposure fields of the resident grid (rto_exposure_field).  exposureField makes, on the first GPU, for
    // every evaluated EMPTY voxel (RTO_EXPO_ALL: all of them; RTO_EXPO_SKIN: those with a SOLID face neighbour) the sum of the
    // weights of the directions along which the ray from the voxel's centre crosses no SOLID voxel within `reach` voxels
    // (RTO_EXPO_NO_LIMIT: none): `dirs` holds three int32 a direction, `weights` one a direction or nothing for all ones; the
    // summary (may be null) gives the evaluated voxels, the sum, the dark and the fully open ones without a download.  exposure
    // downloads the resident field: one int32 per voxel, x fastest, -1 for a voxel that is not evaluated.  Each returns RTO_OK or
    // the refusal's code, which is negative (lastError).  They need the compute pipeline; the CPU form of the same rule for a
    // VoxelGrid is host/Exposure.h.
    int exposureField(const std::vector<int32_t>& dirs, const std::vector<int32_t>& weights, int mode = RTO_EXPO_SKIN, int reach = RTO_EXPO_NO_LIMIT,
                      rto_expo_summary* summary = nullptr);
    int exposure(std::vector<int32_t>& e);
    // Dose fields of the resident grid (rto_dose_field).  doseField makes, on the first GPU, for every
    // evaluated EMPTY voxel (RTO_DOSE_ALL / RTO_DOSE_SKIN) the sum over the point sources -- four int32 each: the voxel i, j, k
    // of the grid and the weight -- of the weight times transmit[k] in Q16, k the SOLID voxels the segment to the source crosses
    // (`transmit` empty: plain line of sight), divided by the squared distance under RTO_DOSE_FALLOFF_INVERSE_SQUARE, for the
    // sources within `reach` voxels; the summary (may be null) gives the evaluated voxels, the sum, the dark and the seen ones and
    // the peak without a download.  dose downloads the resident field (one int32 per voxel, x fastest, -1 for a voxel that is not
    // evaluated), doseCoverage the voxels with a clear view of each source of the last doseField, and hottestVoxel gives the
    // peak's voxel (the smallest index among equals) and value.  Each returns RTO_OK or the refusal's code, which is negative
    // (lastError).  They need the compute pipeline; the CPU form of the same rule for a VoxelGrid is host/Dose.h.
    int doseField(const std::vector<int32_t>& sources, const std::vector<uint32_t>& transmit = {}, int falloff = RTO_DOSE_FALLOFF_NONE,
                  int mode = RTO_DOSE_ALL, int reach = RTO_DOSE_NO_LIMIT, rto_dose_summary* summary = nullptr);
    int dose(std::vector<int32_t>& e);
    int doseCoverage(std::vector<int64_t>& covered);
    int hottestVoxel(int32_t ijk[3], int32_t* value = nullptr);
    // Part segmentation of the resident grid (rto_segment_parts / rto_edit_parts).  segmentParts runs the
    // watershed of the squared distance field of `set` on the first GPU under `connectivity` and merges basins with `ratio` in
    // [0, RTO_PARTS_RATIO_MAX] (0: the components, 1001: the basins): one int32 per voxel, x fastest, the part's number, -1 outside
    // the set; labels and summary may be null.  parts / necks / partLabels download what the last segmentParts left resident.
    // splitAtNecks segments afresh on every GPU, clears (or fills, for RTO_SET_EMPTY) the voxels of the set that touch a part of a
    // larger number, and rebuilds as editVoxels does: the number of voxels flipped (lastEditChanged() too).  Each returns RTO_OK
    // (splitAtNecks: the count) or the refusal's code, which is negative (lastError).  They need the compute pipeline; the CPU form
    // of the same rule for a VoxelGrid is host/Parts.h.
    int segmentParts(int set, int connectivity, int ratio, std::vector<int32_t>* labels, rto_parts_summary* summary = nullptr);
    int parts(std::vector<rto_part>& table);
    int necks(std::vector<rto_neck>& table);
    int partLabels(std::vector<int32_t>& labels);
    int64_t splitAtNecks(int set = RTO_SET_SOLID, int connectivity = RTO_CONN_FACE, int ratio = 800);
    // Component measures of the resident grid (rto_measure_components).  measureComponents labels `set` under
    // `connectivity` on the first GPU and measures every component: one rto_measure per component in the table's order (exposed
    // faces by direction, cell counts, Euler number, first and second moments of the voxel indices) and their sum; table and total
    // may be null.  surfaceArea is the total's exposed faces times voxelSize^2; centroid the centre of mass of the set in world
    // units (found stays false for an empty set); topology the number of pieces, of tunnels through them and of cavities inside
    // them under `connectivity` (the complement under the dual one).  Each returns RTO_OK or the refusal's code, which is negative
    // (lastError), and leaves the set's labels and measures resident.  The CPU form of the same rule is host/Measure.h.
    struct Centroid { bool found = false; double p[3] = { 0.0, 0.0, 0.0 }; int64_t voxels = 0; };
    struct Topology { int64_t pieces = 0, tunnels = 0, cavities = 0; };
    int measureComponents(int set, int connectivity, std::vector<rto_measure>* table, rto_measure* total = nullptr);
    int surfaceArea(int set, double& area);
    int centroid(int set, Centroid& out);
    int topology(int set, int connectivity, Topology& out);
    // Region queries over the whole resident octree on the first GPU (rto_query_points_host, rto_query_regions_host,
    // rto_query_nearest_host): one record per point or brush.  The reference's click handler finds the voxel
    // under the cursor by a CPU march over the dense grid; locate is its GPU counterpart, census says what an editVoxels of the same
    // brushes would change (Carve: filled, Fill: covered - filled) before anything is rebuilt, nearestSolid serves camera collision.
    // Each returns RTO_OK or the refusal's code with lastError set (RTO_E_NO_OCTREE before any octree is set), the records then
    // at their defaults.
    int locate(const std::vector<rto_host::vec3>& points, std::vector<PointLocation>& out);
    int census(const std::vector<VoxelBrush>& regions, std::vector<RegionCensus>& out);
    int nearestSolid(const std::vector<rto_host::vec3>& points, std::vector<NearestSolid>& out,
                     float maxDist = std::numeric_limits<float>::infinity());
    // The current grid: what setOctree / setOctreeFromGrid / loadMesh made, with every edit applied (downloaded when first asked
    // after an edit or a loadMesh).
    const VoxelGrid& grid() const;
    // Mesh in, octree out, with no host copy of the grid (rto_voxelize_mesh): the reference's
    // loadCSVDataIntoVoxelGrid rule on every GPU, then recenterFilledVoxels recenterPasses times (main.cpp runs it twice on the CSV
    // path), then the octree as setOctreeFromGrid builds it; triangles: the leaf triangles too.  xyz: nVerts rows (x, y, z); tris:
    // nTris faces of three row indices.  AUTO grid from voxelSize; false (lastError()) on any error.  grid() downloads the result.
    bool loadMesh(const double* xyz, int64_t nVerts, const int32_t* tris, int64_t nTris, float voxelSize, int recenterPasses = 0,
                  bool triangles = false);
    // The mesh of what the camera sees, made on the GPU (rto_extract_mesh): the list the reference's
    // renderOctree(root, grid, renderer, camera, aspect, extraMargin) returns for MarchingCubesRenderer (kind MeshMC; needs
    // buildLeafTriangles()) or VoxelCubeRenderer (kind MeshCubes; needs a resident grid: setOctreeFromGrid, loadMesh or an edit),
    // in its order.  Empty, with lastError set, on an error.  extractMeshPlanes: caller-supplied planes (nullptr: nothing culled).
    enum MeshKind { MeshMC = RTO_MESH_MC, MeshCubes = RTO_MESH_CUBES };
    std::vector<MCTriangle> extractMesh(int kind, const Camera& camera, float aspect, float extraMargin = 50.0f);
    std::vector<MCTriangle> extractMeshPlanes(int kind, const float* planes, float extraMargin);
    // The isosurface of a voxel field, made on the GPU (rto_extract_isosurface_host): marching cubes of the
    // resident distance, geodesic, thickness, skeleton, exposure or part-label field, the component labels, or with
    // RTO_FIELD_CALLER `volume` (dimZ x dimY x dimX, x fastest) at `level`, in the reference's marchingCubesVolume order, with
    // face normals.  outside: the value of every sample without one (unvalued voxels, the pad ring); pad: close the surface at the
    // grid's faces.  Empty, with lastError set, on an error.  offsetSurface: the surface at distanceInVoxels from the solids --
    // the distance field to RTO_SET_SOLID contoured at its square (half-integer distances give no degenerate triangle only
    // where their square is no field value: 2.5 -> 6.25 is none).  offsetSurface MAKES that distance field, so it replaces the
    // resident one: a field to RTO_SET_EMPTY made before is gone afterwards and has to be made again.  The CPU form of the same rule is host/MarchingCubes.h.
    std::vector<MCTriangle> isoSurface(int source, float level, float outside = 0.0f, bool pad = true, const int32_t* volume = nullptr,
                                       std::vector<int32_t>* triCell = nullptr, rto_iso_summary* summary = nullptr);
    std::vector<MCTriangle> offsetSurface(float distanceInVoxels);
    // Dual contouring of the resident grid, made on the GPU (rto_extract_dual_contour): the list the
    // reference's AdaptiveDualContouringRenderer gives by its per-voxel vertex rule and buildTrianglesCPU, in its order, with the
    // area rule and the clip box of cells in `params`.  Empty, with lastError set, on an error.  dualVertices: the vertex of each
    // of n voxels (linear indices, x fastest; outside the grid: points = -1); n entries, or none, with lastError set, on an error.
    // The CPU form of the same rule is host/DualContouring.h.
    std::vector<MCTriangle> dualContour(const rto_dc_params& params, std::vector<int32_t>* triCell = nullptr, rto_dc_summary* summary = nullptr);
    std::vector<rto_dual_vertex> dualVertices(const int64_t* voxels, int64_t n);
    // BFS numbering of setOctree (RayTracerBVH.cpp:443-490) without touching the GPU.
    static std::vector<GPUNodes> flatten(const OctreeNode* root);
    const std::vector<GPUNodes>& flatNodes() const { return m_flatNodes; }   // empty after setOctreeFromGrid
    int numNodes() const { return m_numNodes; }
    // The renders are asynchronous and leave the frame on the GPU, as the reference's texture is (its image is never
    // read back); framebuffer() copies it to the host on first use after a render (width*height*4 floats, row 0 = top)
    // and finish() just waits for the GPU -- the counterpart of glFinish for timing loops.
    const std::vector<float>& framebuffer() const;
    void finish() const;
    int frameWidth() const { return m_frameW; }
    int frameHeight() const { return m_frameH; }
    void setDevice(int ordinal) { m_device = ordinal; }                  // before ensureComputeInitialized()
    // Multi-GPU (no upstream counterpart; before ensureComputeInitialized()): the GPUs `m_device .. m_device + n - 1` of this
    // node each hold the octree and render the bands `b % n` of every frame (bands of bandRows rows; from 4 GPUs on the first
    // one only gathers and assembles and the others render the bands `b % (n - 1)`); ONE grouped RCCL
    // send/recv per frame lands the parts on the first GPU, which assembles the image (rto_comm_* in rto_hip.h).  The
    // reference's call sequence stays as it is; framebuffer() reads the assembled frame.
    void setDevices(int n, int bandRows = 16) { m_numDevices = n < 1 ? 1 : n; m_bandRows = bandRows; }
    int numDevices() const { return m_numDevices; }
    rto_context* context() const { return m_ctx; }
    const std::string& lastError() const { return m_lastError; }

private:
    void renderLit(const Camera& camera, int width, int height, float aspect, float fovDeg, const Lighting& lighting, bool surface);
    bool render(const Camera& camera, int width, int height, float aspect, float fovDeg);

    OctreeNode* m_octreeRoot;
    mutable VoxelGrid m_grid;
    mutable bool m_gridStale = false;         // the GPUs hold an edited grid that m_grid does not show yet (grid())
    int64_t m_lastEditChanged = 0;
    int64_t m_lastComponents = 0;
    std::vector<GPUNodes> m_flatNodes;
    int m_numNodes;

    bool m_computeInited;
    bool m_computeOk;
    bool m_frustumCullingEnabled;
    int m_device;
    int m_numDevices = 1, m_bandRows = 16;
    rto_context* m_ctx;                       // the first GPU's context (== m_ctxs[0])
    std::vector<rto_context*> m_ctxs;         // one per GPU
    std::vector<rto_comm*> m_comms;           // setDevices(n > 1): the single-process communicator group
    template <class F> bool forEachContext(F&& call, const char* what);
    bool renderFrame(const rto_frame& f, int mode);
    int regionFailed(int rc, const char* what);
    bool computeUsable(const char* who);
    bool makeGridResident(const char* what);
    template <class Make>
    int fieldInto(const char* who, const char* what, std::vector<int32_t>* out, Make&& make, int (*download)(rto_context*, int32_t*, int64_t));
    int64_t editComponents(int set, int connectivity, int select, int64_t arg);
    int64_t editMorphology(int op, float radius);
    mutable std::string m_lastError;
    std::vector<int32_t> m_fieldValues;                // the last renderField's value per pixel
    rto_field_view_summary m_fieldSummary = { 0, 0, 0, 0, 0, 0 };
    ProjectionValues m_projection;                     // the last projectField's outputs per pixel
    CompositeValues m_composite;                       // the last compositeField's outputs per pixel
    rto_composite_summary m_compositeSummary{ 0, 0, 0, 0 };
    int m_doseSources = 0;                             // the last doseField's sources: the length of its coverage table

    mutable std::vector<float> m_frame;
    mutable bool m_frameStale = false;   // the GPU holds a newer frame than m_frame
    int m_frameW, m_frameH;
};
