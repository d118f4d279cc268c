// Projection.cpp -- see Projection.h.
#include "Projection.h"

#include <cmath>

#include "rto_hip.h"

namespace rto_host {

namespace {

// One axis of the walk: a moving axis at coordinate c meets plane c + up next.
struct Axis {
    float o, inv, g;
    int32_t dim, c, up;
    bool moving;
    float t(float vs, int32_t j) const {
        const volatile float jv = static_cast<float>(j) * vs;       // one rounding each
        const volatile float p = g + jv;
        const volatile float s = p - o;
        return s * inv;
    }
};

}  // namespace

std::vector<ProjectionVoxel> projectionWalk(const float gridMin[3], float voxelSize, const int32_t dim[3], const float o[3],
                                            const float d[3], const int32_t lo[3], const int32_t hi[3]) {
    std::vector<ProjectionVoxel> out;
    if (!(std::isfinite(o[0]) && std::isfinite(o[1]) && std::isfinite(o[2]))) return out;
    Axis ax[3];
    bool any = false;
    for (int a = 0; a < 3; a++) {
        Axis& A = ax[a];
        const volatile float inv = 1.0f / d[a];
        A.o = o[a]; A.inv = inv; A.g = gridMin[a]; A.dim = dim[a];
        A.moving = std::isfinite(A.inv);
        A.up = A.inv > 0.0f ? 1 : 0;
        if (!A.moving) {
            const volatile float s = A.o - A.g;
            const volatile float q0 = s / voxelSize;
            const float q = std::floor(q0);
            if (!(q >= static_cast<float>(lo[a]) && q < static_cast<float>(hi[a]))) return out;
            A.c = static_cast<int32_t>(q);
            continue;
        }
        any = true;
        // the planes crossed at the start, counted in the direction of travel until the first T > 0
        int32_t crossed = 0;
        while (crossed <= A.dim && !(A.t(voxelSize, A.up ? crossed : A.dim - crossed) > 0.0f)) crossed++;
        A.c = A.up ? crossed - 1 : A.dim - crossed;
    }
    if (!any) return out;
    auto inside = [&]() {
        for (int a = 0; a < 3; a++) if (ax[a].c < lo[a] || ax[a].c >= hi[a]) return false;
        return true;
    };
    // an axis has a next event while its next plane exists: c + up in 0 .. dim
    auto has_next = [&](const Axis& A) { return A.moving && A.c + A.up >= 0 && A.c + A.up <= A.dim; };
    bool entered = false;
    for (;;) {
        if (inside()) {
            entered = true;
            out.push_back(ProjectionVoxel{ ax[0].c, ax[1].c, ax[2].c });
        } else if (entered) {
            break;                                  // coordinates are monotone: the visited states are one run
        }
        int best = -1;
        float bestT = 0.0f;
        for (int a = 0; a < 3; a++) {
            if (!has_next(ax[a])) continue;
            const float t = ax[a].t(voxelSize, ax[a].c + ax[a].up);
            if (best < 0 || t < bestT) { best = a; bestT = t; }       // ties: the lower axis stays
        }
        if (best < 0) break;
        ax[best].c += ax[best].up ? 1 : -1;
    }
    return out;
}

ProjectionResult projectionReduce(const int32_t* volume, const int32_t dim[3], const ProjectionVoxel* cells, int64_t n, int op,
                                  int32_t validLo, int32_t validHi) {
    ProjectionResult r{ RTO_FIELD_PIXEL_MISS, -1, 0, 0 };
    if (n <= 0) return r;
    r.value = RTO_FIELD_PIXEL_NONE;
    int64_t best = 0, bestVoxel = -1, first = 0, firstVoxel = -1;
    for (int64_t i = 0; i < n; i++) {
        const int64_t idx = (static_cast<int64_t>(cells[i].z) * dim[1] + cells[i].y) * dim[0] + cells[i].x;
        const int32_t v = volume[idx];
        if (v < validLo || v > validHi) continue;
        if (r.count == 0) { first = best = v; firstVoxel = bestVoxel = idx; }
        r.count++;
        r.sum += v;
        if ((op == RTO_PROJECT_MAX && v > best) || (op == RTO_PROJECT_MIN && v < best)) { best = v; bestVoxel = idx; }
    }
    if (r.count == 0) return r;
    r.voxel = firstVoxel;
    switch (op) {
        case RTO_PROJECT_MAX: case RTO_PROJECT_MIN: r.value = best; r.voxel = bestVoxel; break;
        case RTO_PROJECT_MEAN: {
            int64_t q = r.sum / r.count;
            if (r.sum % r.count != 0 && r.sum < 0) q--;             // floor towards minus infinity
            r.value = q;
            break;
        }
        case RTO_PROJECT_COUNT: r.value = r.count; break;
        default: r.value = first; break;
    }
    return r;
}

}  // namespace rto_host
