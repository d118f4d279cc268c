// Dose fields of a VoxelGrid on the CPU: the rule of rto_dose_field (include/rto_hip.h) in plain integer C++:
// for every evaluated EMPTY voxel the sum over point sources of the source's weight, attenuated by a table indexed with the number
// of SOLID voxels that the straight segment from the voxel's centre to the source's crosses and, if asked for, divided by the squared
// distance.  Every (voxel, source) pair walks the template of its own d = s - p: the plane crossings t = (2 m + 1) / (2 |d_a|) in
// order, equal times merged into one step, the last step (the arrival at s) left out.  The tests pin the GPU's fields against the
// numpy statement of the rule and this against the same; tools/dose_bench.py times it as the thing the GPU has to beat.  No GPU, no
// HIP library: usable from any C++ program.
#pragma once

#include <cstdint>
#include <vector>

#include "OctreeVoxel.h"
#include "rto_hip.h"

// The voxels crossed by the open segment from the centre of p to the centre of s, as linear-index-free coordinates (3 int32 an
// entry, in the order they are crossed), p and s themselves left out.  Empty when p == s.
void doseSegment(const int32_t p[3], const int32_t s[3], std::vector<int32_t>& crossed);

// e: one int32 per voxel, x fastest: -1 for a voxel that is not evaluated, else the sum of the contributions of the sources;
// covered: one int64 per source (may be null); summary and steps may be null; *steps = the crossed voxels tested, summed over the
// pairs.  `transmit` null stands for {65536} (m is then not read).  RTO_OK, or the refusal's code in rto_dose_field's order, e and
// covered then empty: RTO_E_INVALID (null sources; n below 1 or above RTO_DOSE_MAX_SOURCES; a negative weight or a sum above
// 2^31 - 1; m below 1 or above RTO_DOSE_MAX_TABLE; a table entry above 65,536; unknown falloff or mode; reach below 1),
// RTO_E_UNSUPPORTED (an empty grid, or more than 2^31 - 2 voxels), RTO_E_INVALID (a source outside the grid; *badSource, if given,
// is its index).
int doseFieldCPU(const VoxelGrid& grid, const int32_t* sources, int n, const uint32_t* transmit, int m, int falloff, int mode, int reach,
                 std::vector<int32_t>& e, std::vector<int64_t>* covered, rto_dose_summary* summary, int64_t* steps = nullptr,
                 int* badSource = nullptr);
