// MarchingCubes.h -- whole-volume marching cubes on the CPU (include/rto_hip.h, rto_extract_isosurface_*).
// marchingCubesVolume carries the reference's name and signature (453-skeleton/MarchingCubes.h:19-23) and its outputs, placeholder
// normals (0, 1, 0) included; isoSurfaceVolume is the CPU form of the whole rule: an int32 volume, the validity window, `outside`,
// the pad ring and the clip box, face normals, tri_cell and the summary.  Both walk the cells in a plain triple loop, z slowest;
// float32, one IEEE operation per operator (the library is built with -ffp-contract=off).  The case table is LocalMC's
// (mc_cases.inc), which equals the reference's edgeTable / triTable (tests/golden/make_golden_iso.py asserts it).
#pragma once

#include <cstdint>
#include <vector>

#include "OctreeVoxel.h"
#include "rto_hip.h"

std::vector<MCTriangle> marchingCubesVolume(const float* scalarField, int dimX, int dimY, int dimZ, const rtmath::vec3& origin, float spacing,
                                            float isoValue);

// volume: dimZ x dimY x dimX, x fastest.  The checks are the C ABI's (RTO_E_INVALID for a bad window, level, pad or clip box:
// an empty list and *rc, when given, set to the code).  triCell and summary may be null.
std::vector<MCTriangle> isoSurfaceVolume(const int32_t* volume, int dimX, int dimY, int dimZ, const rtmath::vec3& gridMin, float voxelSize,
                                         const rto_iso_params& params, std::vector<int32_t>* triCell = nullptr,
                                         rto_iso_summary* summary = nullptr, int* rc = nullptr);
