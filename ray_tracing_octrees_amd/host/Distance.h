// Distance fields of a VoxelGrid on the CPU: the rule of rto_distance_field / rto_edit_morphology (include/rto_hip.h; DESIGN.md
// section 19) in plain integer C++: the exact squared Euclidean distance, in voxel-index units, from every voxel to the nearest
// voxel of a set, as three separable passes (a two-sided sweep along x, the lower envelope of parabolas along y and z), and the
// morphology that is a threshold on it.  The tests pin the GPU's fields against the numpy statement of the rule and this against
// the same; tools/distance_bench.py times it as the thing the GPU has to beat.  No GPU, no HIP library: usable from any C++ program.
#pragma once

#include <cstdint>
#include <vector>

#include "OctreeVoxel.h"
#include "rto_hip.h"

// mq of a distance (floor(dist / voxelSize * 64 + 0.5) in double; -1 for +inf: no cap).  false for NaN, a negative value or more
// than 2^28 quanta: where rto_distance_field answers RTO_E_INVALID.
bool quantizeDistanceCPU(float dist, float voxelSize, int64_t& mq);

// d2: one int32 per voxel, x fastest: the squared distance to the nearest voxel of `set` (RTO_SET_SOLID / RTO_SET_EMPTY),
// RTO_DIST_NONE where the set is empty or 4096 d2 > mq^2 (mq < 0: no cap).  summary may be null.  false for an unknown set or a grid
// the 32-bit field cannot serve (more than 2^31 - 2 voxels, or a squared diagonal of 2^31 - 1 or more); d2 is then empty.
bool distanceFieldCPU(const VoxelGrid& grid, int set, int64_t mq, std::vector<int32_t>& d2, rto_dist_summary* summary);

// rto_edit_morphology on the CPU for rq quanta: RTO_MORPH_DILATE / ERODE / OPEN / CLOSE applied to `grid` in place; the number of
// voxels whose final value differs from the one before the call, -1 where the call is refused (the grid is then untouched).
int64_t applyMorphologyCPU(VoxelGrid& grid, int op, int64_t rq);
