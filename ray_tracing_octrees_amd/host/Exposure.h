// Exposure fields of a VoxelGrid on the CPU: the rule of rto_exposure_field (include/rto_hip.h) in plain
// integer C++: for every evaluated EMPTY voxel the sum of the weights of the directions along which the ray from the voxel's centre
// crosses no SOLID voxel of the grid within the reach.  Every voxel marches the same template of a direction, one period of the
// crossed offsets, shifted by the direction period after period.  The tests pin the GPU's fields against the numpy statement of the
// rule and this against the same; tools/exposure_bench.py times it as the thing the GPU has to beat.  No GPU, no HIP library: usable
// from any C++ program.
#pragma once

#include <cstdint>
#include <vector>

#include "OctreeVoxel.h"
#include "rto_hip.h"

// One period of the voxels crossed by the ray from a voxel's centre along d, as offsets from that voxel (3 int32 an entry, in the
// order they are crossed); prim is d divided by the gcd of its components, and the last entry.  False for a zero direction or a
// component beyond +-RTO_EXPO_MAX_COMP (offsets then empty).
bool exposureTemplate(const int32_t d[3], std::vector<int32_t>& offsets, int32_t prim[3]);

// e: one int32 per voxel, x fastest: -1 for a voxel that is not evaluated, else the sum of the weights of its open directions;
// summary and steps may be null; *steps = the template entries tested, summed over voxels and directions.  RTO_OK, or the refusal's
// code in rto_exposure_field's order, e then empty: RTO_E_INVALID (null dirs; n below 1 or above RTO_EXPO_MAX_DIRS; a zero direction
// or a component beyond +-255; a negative weight or a sum above 2^31 - 1; unknown mode; reach below 1), RTO_E_UNSUPPORTED (an empty
// grid, or more than 2^31 - 2 voxels).
int exposureFieldCPU(const VoxelGrid& grid, const int32_t* dirs, const int32_t* weights, int n, int mode, int reach, std::vector<int32_t>& e,
                     rto_expo_summary* summary, int64_t* steps = nullptr);
