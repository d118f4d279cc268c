// Part segmentation of a VoxelGrid on the CPU: the rule of rto_segment_parts / rto_edit_parts (include/rto_hip.h; DESIGN.md section
// 26) in plain integer C++ over host/Distance's transform: every voxel of a set climbs to the nearest local maximum of its squared
// distance to the other set, and basins are merged across necks that are wide relative to the lower of the two peaks.  The tests
// pin the GPU's labels and tables against the numpy statement of the rule and this against the same; tools/parts_bench.py times it
// as the thing the GPU has to beat.  No GPU, no HIP library: usable from any C++ program.
#pragma once

#include <cstdint>
#include <vector>

#include "OctreeVoxel.h"
#include "rto_hip.h"

// Segments the voxels of `set` (RTO_SET_SOLID / RTO_SET_EMPTY) under `connectivity` (RTO_CONN_FACE / RTO_CONN_FULL) with the merge
// ratio `ratio` in [0, RTO_PARTS_RATIO_MAX].  labels: one int32 per voxel, x fastest: the part's number (ascending order of the
// parts' smallest voxel), -1 outside the set.  summary may be null.  Returns the number of parts, -1 where rto_segment_parts answers
// RTO_E_INVALID or RTO_E_UNSUPPORTED (everything is then empty).
int64_t segmentPartsCPU(const VoxelGrid& grid, int set, int connectivity, int ratio, std::vector<int32_t>& labels, std::vector<rto_part>& parts,
                        std::vector<rto_neck>& necks, rto_parts_summary* summary);

// rto_edit_parts on the CPU: flips every voxel of the set that has a neighbour of a larger part number; the number of voxels
// flipped, -1 where the call is refused (the grid is then untouched).
int64_t splitAtNecksCPU(VoxelGrid& grid, int set, int connectivity, int ratio);
