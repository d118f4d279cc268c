// Composite.h -- field compositing on the CPU (include/rto_hip.h, rto_composite_field_*): the plain
// voxel-by-voxel walk of host/Projection.h, composited front to back by the rule.  No brick table, no solid table, no LDS tables: the
// index is the field views' own search, the state is four unsigned 32-bit integers, and the six float operations at the end are
// float32, one IEEE operation per operator (the library is built with -ffp-contract=off).
#pragma once

#include <cstdint>

#include "Projection.h"
#include "rto_hip.h"

namespace rto_host {

enum CompositeEnd { COMPOSITE_THROUGH = 0, COMPOSITE_SATURATED = 1, COMPOSITE_OCCLUDED = 2 };

struct CompositeResult {
    uint32_t T, R, G, B;    // the transmittance (Q16) and the premultiplied colour sums
    int64_t first;          // the first contributing voxel's linear index, -1 without one
    int64_t stop;           // the occluding or the saturating voxel, -1 when the walk went through
    int32_t count;          // contributions
    int32_t end;            // CompositeEnd
};

// The field views' LUT index of a valued value v under `scale` and the range (lo, hi); lo < hi unless scale is CATEGORY.
int compositeIndex(int32_t v, int32_t lo, int32_t hi, int scale);

// thr[k], k = 0 .. 255: the smallest w = clamp(v) - lo whose index is at least k, LINEAR ceil(k s / 255) and SQRT ceil(k k s /
// 65025) with s = hi - lo: what the march kernel keeps in LDS.  The index of w is the largest k with thr[k] <= w.
void compositeThresholds(int scale, int32_t lo, int32_t hi, uint32_t thr[256]);

// One ray: its visited voxels (projectionWalk's) composited under `comp`.  grid: the resident bytes (dimZ x dimY x dimX), read
// only when comp.occlude is set.
CompositeResult compositeRay(const int32_t* volume, const uint8_t* grid, const int32_t dim[3], const ProjectionVoxel* cells, int64_t n,
                             const rto_field_composite& comp, const uint32_t lut[256]);

// The pixel's colour from its result; visited: the ray met a voxel; under: the pixel of the frame below, or null.
void compositeColour(const CompositeResult& r, bool visited, const rto_field_composite& comp, const float* under, float out[4]);

}  // namespace rto_host
