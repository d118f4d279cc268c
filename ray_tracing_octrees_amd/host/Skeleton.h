// Skeletons of a VoxelGrid on the CPU: the rule of rto_skeleton_field / rto_edit_skeleton (include/rto_hip.h)
// in plain integer C++: topology-preserving thinning of a set (the FILLED or the EMPTY voxels) in passes of one mark and eight
// subfield sub-steps, with the pass number of every removed voxel.  The tests pin the GPU's fields against the numpy statement of the
// rule and this against the same; tools/skeleton_bench.py times it as the thing the GPU has to beat.  No GPU, no HIP library: usable
// from any C++ program.
#pragma once

#include <cstdint>
#include <vector>

#include "OctreeVoxel.h"
#include "rto_hip.h"

// Is the centre of the 27-bit neighbourhood mask (bit (dx + 1) + 3 (dy + 1) + 9 (dz + 1); bit 13, the centre, is ignored) a simple
// point of the set whose voxels are the mask's ones, under `connectivity`?
bool skeletonSimpleCPU(uint32_t mask, int connectivity);

// k: one int32 per voxel, x fastest: -1 outside the set, 0 for the skeleton, p >= 1 for the pass that removed the voxel; summary
// may be null.  RTO_OK, or the refusal's code in rto_skeleton_field's order, k then empty: RTO_E_INVALID (unknown set, connectivity
// or mode; CURVE with FACE; n < 0 or null anchors with n > 0; maxPasses below 1; an anchor out of range), RTO_E_UNSUPPORTED (an
// empty grid, or more than 2^31 - 2 voxels).
int skeletonFieldCPU(const VoxelGrid& grid, int set, int connectivity, int mode, const int64_t* anchors, int64_t n, int64_t maxPasses,
                     std::vector<int32_t>& k, rto_skel_summary* summary);

// rto_edit_skeleton on the CPU: every voxel with k > 0 is flipped in place; the number flipped, or the refusal's code (negative).
int64_t thinCPU(VoxelGrid& grid, int set, int connectivity, int mode, const int64_t* anchors, int64_t n, int64_t maxPasses);
