// Local thickness fields of a VoxelGrid on the CPU: the rule of rto_thickness_field (include/rto_hip.h) in
// plain integer C++ over host/Distance.cpp's transform: at every voxel of a medium the squared radius of the largest ball that fits
// inside the medium and contains the voxel, for balls of squared radius up to c <= 64, with the histogram and the summary.  The
// tests pin the GPU's fields against the numpy statement of the rule and this against the same; tools/thickness_bench.py times it
// as the thing the GPU has to beat.  No GPU, no HIP library: usable from any C++ program.
#pragma once

#include <cstdint>
#include <vector>

#include "Distance.h"

// t2: one int32 per voxel, x fastest; bins: c + 1 counts (bins[t] = medium voxels with t2 = t); summary may be null.  mq: the radius
// in quanta (quantizeDistanceCPU); c = floor(mq^2 / 4096).  RTO_OK, or the refusal's code in rto_thickness_field's order, t2 and
// bins then empty: RTO_E_INVALID (unknown medium; mq below 0 or above 2^28; c = 0), RTO_E_UNSUPPORTED (c > 64; a grid the 32-bit
// transform cannot serve).
int thicknessFieldCPU(const VoxelGrid& grid, int medium, int64_t mq, std::vector<int32_t>& t2, std::vector<int64_t>& bins,
                      rto_thick_summary* summary);
