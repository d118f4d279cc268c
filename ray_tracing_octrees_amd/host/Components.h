// Connected components of a VoxelGrid on the CPU: the rule of rto_label_components (include/rto_hip.h) as a
// plain breadth-first search.  The tests pin the GPU's labels and table against it, and tools/component_bench.py times it as the
// thing the GPU has to beat.  No GPU, no HIP library: usable from any C++ program.
#pragma once

#include <cstdint>
#include <vector>

#include "OctreeVoxel.h"
#include "rto_hip.h"

// Labels the voxels of `set` (RTO_SET_SOLID / RTO_SET_EMPTY) under `connectivity` (RTO_CONN_FACE / RTO_CONN_FULL).  labels: one
// int32 per voxel, x fastest: the component's number (ascending order of root = smallest linear index), -1 outside the set.
// Returns the number of components, -1 for an unknown set or connectivity or a grid of more than 2^31 - 2 voxels.
int64_t labelComponentsCPU(const VoxelGrid& grid, int set, int connectivity, std::vector<int32_t>& labels,
                           std::vector<rto_component>& table);

// rto_edit_components' selection on the CPU: flips every voxel of the selected components of `grid`; the number of voxels flipped,
// -1 where rto_edit_components answers RTO_E_INVALID or RTO_E_UNSUPPORTED (the grid is then untouched).
int64_t applyComponentSelectionCPU(VoxelGrid& grid, int set, int connectivity, int select, int64_t arg);
