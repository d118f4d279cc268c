// Projection.h -- field projections on the CPU (include/rto_hip.h, rto_project_field_*): the plain
// voxel-by-voxel walk of one ray through the dense grid and the reduction of an int32 volume over it.  No brick table, no entry by
// rank, no jump: the walk starts at the ray's start state and takes one event at a time, which is the rule as it is written.  All
// float arithmetic is float32, one IEEE operation per operator (the library is built with -ffp-contract=off).
#pragma once

#include <cstdint>
#include <vector>

namespace rto_host {

struct ProjectionVoxel { int32_t x, y, z; };

struct ProjectionResult {
    int64_t value;      // RTO_FIELD_PIXEL_MISS, RTO_FIELD_PIXEL_NONE or the op's value
    int64_t voxel;      // the deciding voxel's linear index, -1 without one
    int64_t sum;        // of the valued voxels
    int64_t count;
};

// The visited voxels of the ray (o, d) in walk order: the states of the whole-grid walk that lie in [lo, hi) on every axis.
std::vector<ProjectionVoxel> projectionWalk(const float gridMin[3], float voxelSize, const int32_t dim[3], const float o[3],
                                            const float d[3], const int32_t lo[3], const int32_t hi[3]);

// The reduction of volume (dimZ x dimY x dimX, x fastest) over a walk under op (RTO_PROJECT_*) and the window [validLo, validHi].
ProjectionResult projectionReduce(const int32_t* volume, const int32_t dim[3], const ProjectionVoxel* cells, int64_t n, int op,
                                  int32_t validLo, int32_t validHi);

}  // namespace rto_host
