// Composite.cpp -- see Composite.h.
#include "Composite.h"

namespace rto_host {

namespace {

uint32_t mix32(uint32_t v) {                         // the lit render's
    v ^= v >> 16; v *= 0x7feb352du; v ^= v >> 15; v *= 0x846ca68bu; v ^= v >> 16;
    return v;
}

}  // namespace

int compositeIndex(int32_t v, int32_t lo, int32_t hi, int scale) {
    if (scale == RTO_SCALE_CATEGORY) return static_cast<int>(mix32(static_cast<uint32_t>(v)) & 255u);
    const int64_t s = static_cast<int64_t>(hi) - lo;
    if (s <= 0) return 0;
    const int64_t cl = v < lo ? lo : (v > hi ? hi : v);
    const int64_t w = cl - lo;
    if (scale == RTO_SCALE_LINEAR) return static_cast<int>(w * 255 / s);
    int k = 0;
    while (k < 255 && static_cast<int64_t>(k + 1) * (k + 1) * s <= w * 65025) k++;
    return k;
}

void compositeThresholds(int scale, int32_t lo, int32_t hi, uint32_t thr[256]) {
    const int64_t s = static_cast<int64_t>(hi) - lo;
    for (int64_t k = 0; k < 256; k++) {
        const int64_t num = (scale == RTO_SCALE_SQRT ? k * k : k) * s, den = scale == RTO_SCALE_SQRT ? 65025 : 255;
        thr[k] = scale == RTO_SCALE_CATEGORY ? 0u : static_cast<uint32_t>((num + den - 1) / den);
    }
}

CompositeResult compositeRay(const int32_t* volume, const uint8_t* grid, const int32_t dim[3], const ProjectionVoxel* cells, int64_t n,
                             const rto_field_composite& comp, const uint32_t lut[256]) {
    CompositeResult r{ 65536u, 0u, 0u, 0u, -1, -1, 0, COMPOSITE_THROUGH };
    for (int64_t i = 0; i < n; i++) {
        const int64_t idx = (static_cast<int64_t>(cells[i].z) * dim[1] + cells[i].y) * dim[0] + cells[i].x;
        if (comp.occlude && grid[idx] == 1) { r.end = COMPOSITE_OCCLUDED; r.stop = idx; break; }
        const int32_t v = volume[idx];
        if (v < comp.valid_lo || v > comp.valid_hi) continue;
        const uint32_t e = lut[compositeIndex(v, comp.range_lo, comp.range_hi, comp.scale)];
        const uint32_t a = e >> 24, ap = a + (a >> 7);
        if (ap == 0) continue;
        const uint32_t c = (r.T * ap) >> 8;
        r.R += c * (e & 255u); r.G += c * ((e >> 8) & 255u); r.B += c * ((e >> 16) & 255u);
        r.T -= c;
        if (r.count == 0) r.first = idx;
        r.count++;
        if (r.T <= static_cast<uint32_t>(comp.stop_q16)) { r.end = COMPOSITE_SATURATED; r.stop = idx; break; }
    }
    return r;
}

void compositeColour(const CompositeResult& r, bool visited, const rto_field_composite& comp, const float* under, float out[4]) {
    if (!under && !visited) {
        for (int k = 0; k < 4; k++) out[k] = comp.miss_rgba[k];
        return;
    }
    const float* bg = under ? under : comp.background_rgba;
    const volatile float tf = static_cast<float>(r.T) / 65536.0f;       // one rounding each
    const uint32_t sums[3] = { r.R, r.G, r.B };
    for (int k = 0; k < 3; k++) {
        const volatile float own = static_cast<float>(sums[k]) / 16711680.0f;
        const volatile float below = tf * bg[k];
        out[k] = own + below;
    }
    const volatile float own = static_cast<float>(65536u - r.T) / 65536.0f;
    const volatile float below = tf * bg[3];
    out[3] = own + below;
}

}  // namespace rto_host
