// Geodesic distance fields of a VoxelGrid on the CPU: the rule of rto_geodesic_field / rto_geodesic_paths / rto_edit_geodesic
// (include/rto_hip.h) in plain integer C++.  The shortest path inside a medium from a set of seeds is found
// with a bucket queue: the weights are at most 5, so the values in the queue at any time span at most 6 consecutive integers and
// six buckets used in rotation are exact.  The tests pin the GPU's fields against the Python statement of the rule and this against
// the same; tools/geodesic_bench.py times it as the thing the GPU has to beat; the drop-in class falls back to it.  No GPU, no HIP
// library: usable from any C++ program.
#pragma once

#include <cstdint>
#include <vector>

#include "OctreeVoxel.h"
#include "rto_hip.h"

// g: one int32 per voxel, x fastest: the smallest total weight of a path of moves inside `medium` (RTO_SET_SOLID / RTO_SET_EMPTY)
// from any of the n seeds (linear indices; those outside the medium are ignored), RTO_DIST_NONE outside the medium, out of reach or
// above `limit` (>= 0x7fffffff: none).  summary may be null.  The code is RTO_OK or the refusal's, in rto_geodesic_field's order
// (RTO_E_INVALID: unknown medium or connectivity, n < 1, null seeds, limit < 0, a seed out of range; RTO_E_UNSUPPORTED: a grid the
// 32-bit field cannot serve); g is then empty.
int geodesicFieldCPU(const VoxelGrid& grid, int medium, int connectivity, const int64_t* seeds, int64_t n, int64_t limit,
                     std::vector<int32_t>& g, rto_geo_summary* summary);

// The paths of rto_geodesic_paths on a field g of `grid` made under `connectivity`: row i of outVoxels (maxLen entries, may be null
// when maxLen is 0) takes the first min(len, maxLen) voxels of target i's path, -1 behind them; outLen[i] the full length, -1 for a
// target the field does not reach.  RTO_OK, or RTO_E_INVALID (n < 1, null pointers, maxLen < 0, a target out of range, a field of
// another size).
int geodesicPathsCPU(const VoxelGrid& grid, int connectivity, const std::vector<int32_t>& g, const int64_t* targets, int64_t n,
                     int64_t maxLen, int64_t* outVoxels, int64_t* outLen);

// rto_edit_geodesic on the CPU: every voxel the field reaches is flipped in place; the number flipped, or the refusal's code
// (negative; the grid is then untouched).
int64_t floodGeodesicCPU(VoxelGrid& grid, int medium, int connectivity, const int64_t* seeds, int64_t n, int64_t limit);
