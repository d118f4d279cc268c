// composite_selftest.cpp -- the CPU form of a field composite (host/Composite.cpp over host/Projection.cpp's walk) against a
// brute-force statement of the rule of DESIGN.md section 29 that shares no code with it: the walk is the sorted-events walk of
// projection_selftest.cpp, the index is found by a downward scan of the field views' inequality in 128-bit integers, the state is
// kept in 64 bits, and the thresholds are checked to give that index.  Host code only; meant to be built and run with sanitizers:
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -Iinclude
//       -Iray_tracing_octrees_amd/host tools/composite_selftest.cpp ray_tracing_octrees_amd/host/Composite.cpp
//       ray_tracing_octrees_amd/host/Projection.cpp -o composite_selftest
//   ./composite_selftest [rays]
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <tuple>
#include <vector>

#include "Composite.h"
#include "Projection.h"
#include "rto_hip.h"

using rto_host::ProjectionVoxel;

static float plane_t(float g, float vs, float o, float inv, int j) {
    const volatile float jv = static_cast<float>(j) * vs;
    const volatile float p = g + jv;
    const volatile float s = p - o;
    return s * inv;
}

// The rule, sorted: every event, then the filter.
static std::vector<ProjectionVoxel> brute_walk(const float g[3], float vs, const int32_t dim[3], const float o[3], const float d[3],
                                               const int32_t lo[3], const int32_t hi[3]) {
    std::vector<ProjectionVoxel> out;
    if (!(std::isfinite(o[0]) && std::isfinite(o[1]) && std::isfinite(o[2]))) return out;
    int c[3], step[3] = { 0, 0, 0 };
    std::vector<std::tuple<float, int, int>> events;
    bool any = false;
    for (int a = 0; a < 3; a++) {
        const volatile float inv = 1.0f / d[a];
        if (!std::isfinite(inv)) {
            const volatile float s = o[a] - g[a];
            const volatile float q0 = s / vs;
            const float q = std::floor(q0);
            if (!(q >= static_cast<float>(lo[a]) && q < static_cast<float>(hi[a]))) return out;
            c[a] = static_cast<int>(q);
            continue;
        }
        any = true;
        const bool up = inv > 0.0f;
        int crossed = 0;
        for (int k = 0; k <= dim[a]; k++) {
            const float t = plane_t(g[a], vs, o[a], inv, up ? k : dim[a] - k);
            if (t > 0.0f) events.emplace_back(t, a, k); else crossed++;
        }
        c[a] = up ? crossed - 1 : dim[a] - crossed;
        step[a] = up ? 1 : -1;
    }
    if (!any) return out;
    std::sort(events.begin(), events.end());
    auto inside = [&]() { return c[0] >= lo[0] && c[0] < hi[0] && c[1] >= lo[1] && c[1] < hi[1] && c[2] >= lo[2] && c[2] < hi[2]; };
    if (inside()) out.push_back(ProjectionVoxel{ c[0], c[1], c[2] });
    for (const auto& e : events) {
        c[std::get<1>(e)] += step[std::get<1>(e)];
        if (inside()) out.push_back(ProjectionVoxel{ c[0], c[1], c[2] });
    }
    return out;
}

static uint32_t brute_mix32(uint32_t v) {
    v ^= v >> 16; v *= 0x7feb352du; v ^= v >> 15; v *= 0x846ca68bu; v ^= v >> 16;
    return v;
}

// The field views' index, from the top: the largest k with k m(k) s <= w D.
static int brute_index(int64_t v, int64_t lo, int64_t hi, int scale) {
    if (scale == RTO_SCALE_CATEGORY) return static_cast<int>(brute_mix32(static_cast<uint32_t>(static_cast<int32_t>(v))) & 255u);
    const __int128 s = hi - lo, w = std::min(std::max(v, lo), hi) - lo;
    for (int k = 255; k > 0; k--) {
        const __int128 lhs = (scale == RTO_SCALE_SQRT ? static_cast<__int128>(k) * k : static_cast<__int128>(k)) * s;
        if (lhs <= w * (scale == RTO_SCALE_SQRT ? 65025 : 255)) return k;
    }
    return 0;
}

int main(int argc, char** argv) {
    const int rays = argc > 1 ? std::atoi(argv[1]) : 20000;
    std::mt19937 rng(4321);
    auto uni = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    auto integer = [&](int a, int b) { return std::uniform_int_distribution<int>(a, b)(rng); };
    const int32_t adversarial[12] = { 0, 1, 0x7ffffffe, -1, -7, INT32_MIN + 2, INT32_MAX, 2, 1000, -(1 << 30), 5, 77 };
    const int32_t windows[3][2] = { { INT32_MIN + 2, INT32_MAX }, { 0, 0x7ffffffe }, { -7, 77 } };
    const int32_t ranges[4][2] = { { INT32_MIN, INT32_MAX }, { 0, 1000 }, { -7, 77 }, { 1, 2 } };
    const int32_t stops[4] = { 0, 256, 32768, 65535 };
    long long nonempty = 0, voxels = 0, contributions = 0, ends[3] = { 0, 0, 0 }, indices = 0;

    // the thresholds give the index: every w of small spans, seeded w of the widest
    for (int scale = RTO_SCALE_LINEAR; scale <= RTO_SCALE_SQRT; scale++)
        for (const auto& r : ranges) {
            uint32_t thr[256];
            rto_host::compositeThresholds(scale, r[0], r[1], thr);
            const int64_t s = static_cast<int64_t>(r[1]) - r[0];
            const int n = s <= 1000 ? static_cast<int>(s) + 1 : 4000;
            for (int i = 0; i < n; i++) {
                const int64_t w = s <= 1000 ? i : (i < 4 ? (i < 2 ? i : s - (i - 2)) : static_cast<int64_t>(uni(0, 1) * static_cast<float>(s)) % (s + 1));
                int k = 0;
                for (int t = 1; t < 256; t++) if (thr[t] <= static_cast<uint64_t>(w)) k = t;
                const int want = brute_index(r[0] + w, r[0], r[1], scale);
                const int host = rto_host::compositeIndex(static_cast<int32_t>(r[0] + w), r[0], r[1], scale);
                if (k != want || host != want) {
                    std::printf("FAIL index: scale %d range %d..%d w %lld: thresholds %d, host %d, expected %d\n", scale, r[0], r[1], (long long)w, k,
                                host, want);
                    return 1;
                }
                indices++;
            }
        }

    for (int i = 0; i < rays; i++) {
        const int kind = i % 4;
        int32_t dim[3] = { integer(1, 21), integer(1, 21), integer(1, 21) };
        float g[3], o[3], d[3], vs;
        if (kind == 0) {                                     // exact lattice: edges and corners, ties
            vs = 1.0f;
            for (int a = 0; a < 3; a++) { g[a] = (float)integer(-5, 4); o[a] = g[a] + (float)integer(-6, 27); d[a] = g[a] + (float)integer(0, dim[a]) - o[a]; }
        } else if (kind == 1) {                              // still axes
            vs = uni(0.01f, 0.3f);
            const float still[4] = { 0.0f, -0.0f, 1e-42f, -1e-45f };
            for (int a = 0; a < 3; a++) { g[a] = uni(-1, 1); o[a] = g[a] + uni(-0.2f, 1.2f) * vs * dim[a]; d[a] = g[a] + uni(0, 1) * vs * dim[a] - o[a]; }
            d[integer(0, 2)] = still[integer(0, 3)];
        } else if (kind == 2) {                              // inside the grid or on a plane
            vs = 1.0f / 64;
            for (int a = 0; a < 3; a++) { g[a] = uni(-1, 1); o[a] = g[a] + (float)integer(0, dim[a]) * vs; d[a] = uni(-1, 1); }
        } else {
            vs = uni(0.01f, 0.3f);
            const int m = std::max(dim[0], std::max(dim[1], dim[2]));
            for (int a = 0; a < 3; a++) { g[a] = uni(-1, 1); o[a] = g[a] + uni(-1, 2) * vs * m; d[a] = g[a] + uni(0, 1) * vs * dim[a] - o[a]; }
        }
        int32_t lo[3] = { 0, 0, 0 }, hi[3] = { dim[0], dim[1], dim[2] };
        if (integer(0, 1)) for (int a = 0; a < 3; a++) { lo[a] = integer(0, dim[a] - 1); hi[a] = integer(lo[a] + 1, dim[a]); }
        const std::vector<ProjectionVoxel> want = brute_walk(g, vs, dim, o, d, lo, hi);
        const std::vector<ProjectionVoxel> got = rto_host::projectionWalk(g, vs, dim, o, d, lo, hi);
        if (want.size() != got.size()) { std::printf("FAIL walk: ray %d: %zu voxels, the sorted statement has %zu\n", i, got.size(), want.size()); return 1; }
        if (want.empty()) continue;
        nonempty++;
        voxels += (long long)want.size();
        std::vector<int32_t> vol((size_t)dim[0] * dim[1] * dim[2]);
        std::vector<uint8_t> grid(vol.size());
        for (size_t k = 0; k < vol.size(); k++) { vol[k] = adversarial[(k * 7 + k / 5) % 12]; grid[k] = (k * 11 + k / 3) % 9 == 0 ? 1 : ((k % 13 == 0) ? 2 : 0); }
        uint32_t lut[256];
        const int lutKind = i % 3;                           // fog, a ramp with a zero-alpha run, opaque
        for (uint32_t k = 0; k < 256; k++) {
            const uint32_t a = lutKind == 0 ? 1 + k / 32 : (lutKind == 1 ? ((k >= 64 && k < 192) ? 0 : (k >= 248 ? 255 : 40 + k / 2)) : 255);
            lut[k] = (k * 2654435761u & 0xffffffu) | (a << 24);
        }
        rto_field_composite comp;
        std::memset(&comp, 0, sizeof comp);
        comp.source = RTO_FIELD_CALLER;
        comp.scale = (i / 3) % 3;
        comp.valid_lo = windows[(i / 9) % 3][0]; comp.valid_hi = windows[(i / 9) % 3][1];
        comp.range_lo = ranges[(i / 27) % 4][0]; comp.range_hi = ranges[(i / 27) % 4][1];
        comp.stop_q16 = stops[(i / 4) % 4];
        comp.occlude = (i / 16) % 2;
        const float bgc[4] = { 0.25f, 0.5f, 0.125f, 0.5f }, missc[4] = { 0.0f, 0.125f, 0.25f, 1.0f };
        std::memcpy(comp.background_rgba, bgc, sizeof bgc);
        std::memcpy(comp.miss_rgba, missc, sizeof missc);
        const rto_host::CompositeResult r = rto_host::compositeRay(vol.data(), grid.data(), dim, got.data(), (int64_t)got.size(), comp, lut);
        // the statement in 64 bits
        uint64_t T = 65536, R = 0, G = 0, B = 0;
        int64_t first = -1, stop = -1, count = 0;
        int end = 0;
        for (const ProjectionVoxel& c : want) {
            const int64_t idx = ((int64_t)c.z * dim[1] + c.y) * dim[0] + c.x;
            if (comp.occlude && grid[(size_t)idx] == 1) { end = 2; stop = idx; break; }
            const int64_t v = vol[(size_t)idx];
            if (v < comp.valid_lo || v > comp.valid_hi) continue;
            const uint32_t e = lut[brute_index(v, comp.range_lo, comp.range_hi, comp.scale)];
            const uint64_t a = (e >> 24) + ((e >> 24) >> 7);
            if (a == 0) continue;
            const uint64_t cc = (T * a) / 256;
            R += cc * (e & 255); G += cc * ((e >> 8) & 255); B += cc * ((e >> 16) & 255);
            T -= cc;
            if (!count) first = idx;
            count++;
            if (T <= (uint64_t)comp.stop_q16) { end = 1; stop = idx; break; }
        }
        if (R > 16711680 || G > 16711680 || B > 16711680 || R > 255 * (65536 - T)) { std::printf("FAIL bound: ray %d\n", i); return 1; }
        if (r.T != T || r.R != R || r.G != G || r.B != B || r.first != first || r.stop != stop || r.count != count || r.end != end) {
            std::printf("FAIL composite: ray %d: T %u R %u G %u B %u first %lld stop %lld count %d end %d, expected %llu %llu %llu %llu %lld %lld %lld %d\n",
                        i, r.T, r.R, r.G, r.B, (long long)r.first, (long long)r.stop, r.count, r.end, (unsigned long long)T, (unsigned long long)R,
                        (unsigned long long)G, (unsigned long long)B, (long long)first, (long long)stop, (long long)count, end);
            return 1;
        }
        // the colour against double: each float32 result is within one rounding per operation of the real value
        const float under[4] = { 0.5f, 1.25f, -0.5f, 0.75f };
        float out[4];
        rto_host::compositeColour(r, true, comp, i % 2 ? under : nullptr, out);
        const float* bg = i % 2 ? under : comp.background_rgba;
        const double tf = (double)T / 65536.0, sums[3] = { (double)R, (double)G, (double)B };
        for (int k = 0; k < 4; k++) {
            const double real = (k < 3 ? sums[k] / 16711680.0 : (65536.0 - (double)T) / 65536.0) + tf * bg[k];
            if (std::fabs((double)out[k] - real) > 4e-7 * (1.0 + std::fabs(real))) { std::printf("FAIL colour: ray %d channel %d: %g, real %g\n", i, k, out[k], real); return 1; }
        }
        contributions += count;
        ends[end]++;
    }
    if (nonempty * 4 < rays || !ends[0] || !ends[1] || !ends[2]) { std::printf("FAIL: only %lld of %d rays visit a voxel, ends %lld %lld %lld\n", nonempty, rays, ends[0], ends[1], ends[2]); return 1; }
    std::printf("composite_selftest: %lld indices from the thresholds; %d rays, %lld visit the box, %lld voxels, %lld contributions; %lld walks "
                "went through, %lld saturated, %lld were occluded: host/Composite equals the brute-force statement\n", indices, rays, nonempty, voxels,
                contributions, ends[0], ends[1], ends[2]);
    return 0;
}
