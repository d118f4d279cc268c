// Component measures on the CPU: the rule of rto_measure_components (include/rto_hip.h) as plain loops over
// a label volume: per component and for the whole set the exposed faces by direction, the cell counts and the Euler number, the
// first and second moments of the voxel indices.  The tests pin the GPU's table against the numpy statement of the rule and this
// against the same; tools/measure_bench.py times it as the thing the GPU has to beat.  No GPU, no HIP library: usable from any C++
// program.
#pragma once

#include <cstdint>
#include <vector>

#include "rto_hip.h"

// labels: one int32 per voxel, x fastest: the component's number in [0, count), -1 outside the set (what labelComponentsCPU and
// rto_download_labels give).  connectivity: the one the labels were made under (RTO_CONN_FACE / RTO_CONN_FULL); it chooses the
// cells.  out: count records; total (may be null): their sum.  RTO_OK, or the refusal's code, out then empty: RTO_E_INVALID
// (unknown connectivity, a dimension below 1, a negative count, a label outside [-1, count)), RTO_E_UNSUPPORTED (a dimension above
// 32768).
int measureComponentsCPU(int dimX, int dimY, int dimZ, const int32_t* labels, int64_t count, int connectivity,
                         std::vector<rto_measure>& out, rto_measure* total);
