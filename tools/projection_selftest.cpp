// projection_selftest.cpp -- the CPU form of a field projection (host/Projection.cpp: the plain voxel-by-voxel walk) against a
// second statement of the rule of DESIGN.md section 28 that shares no code with it: collect every event of every moving axis,
// sort them by (T, axis, order of travel), walk them all and keep the states inside the box.  Then the reductions against a
// straight loop.  Host code only; meant to be built and run with sanitizers:
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -Iinclude
//       -Iray_tracing_octrees_amd/host tools/projection_selftest.cpp ray_tracing_octrees_amd/host/Projection.cpp -o projection_selftest
//   ./projection_selftest [rays]
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <tuple>
#include <vector>

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
static std::vector<ProjectionVoxel> brute(const float g[3], float vs, const int32_t dim[3], const float o[3], const float d[3],
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
            const int j = up ? k : dim[a] - k;
            const float t = plane_t(g[a], vs, o[a], inv, j);
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

int main(int argc, char** argv) {
    const int rays = argc > 1 ? std::atoi(argv[1]) : 20000;
    std::mt19937 rng(12345);
    auto uni = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    auto integer = [&](int a, int b) { return std::uniform_int_distribution<int>(a, b)(rng); };
    const int32_t adversarial[10] = { 0, 1, 0x7ffffffe, -1, -7, INT32_MIN + 2, INT32_MAX, 2, 1000, -(1 << 30) };
    long long nonempty = 0, voxels = 0;
    for (int i = 0; i < rays; i++) {
        const int kind = i % 5;
        int32_t dim[3] = { integer(1, 21), integer(1, 21), integer(1, 21) };
        float g[3], o[3], d[3], vs;
        if (kind == 0) {                                     // exact lattice: edges and corners, ties
            vs = 1.0f;
            for (int a = 0; a < 3; a++) { g[a] = (float)integer(-5, 4); o[a] = g[a] + (float)integer(-6, 27); d[a] = g[a] + (float)integer(0, dim[a]) - o[a]; }
        } else if (kind == 1) {                              // still axes, -0.0 and overflowing reciprocals among them
            vs = uni(0.01f, 0.3f);
            const float still[4] = { 0.0f, -0.0f, 1e-42f, -1e-45f };
            for (int a = 0; a < 3; a++) { g[a] = uni(-1, 1); o[a] = g[a] + uni(-0.2f, 1.2f) * vs * dim[a]; d[a] = g[a] + uni(0, 1) * vs * dim[a] - o[a]; }
            d[integer(0, 2)] = still[integer(0, 3)];
            if (integer(0, 1)) d[integer(0, 2)] = still[integer(0, 3)];
        } else if (kind == 2) {                              // inside the grid or on a plane
            vs = 1.0f / 64;
            for (int a = 0; a < 3; a++) { g[a] = uni(-1, 1); o[a] = g[a] + (float)integer(0, dim[a]) * vs; d[a] = uni(-1, 1); }
            if (integer(0, 1)) o[integer(0, 2)] += uni(0, 1) * vs;
        } else if (kind == 3) {                              // far away: consecutive planes share a T
            vs = 1.0f / 64;
            const float far = std::pow(10.0f, uni(2, 7));
            float n = 0;
            for (int a = 0; a < 3; a++) { d[a] = uni(-1, 1); n += d[a] * d[a]; }
            n = std::sqrt(n);
            for (int a = 0; a < 3; a++) { d[a] /= n; g[a] = uni(-1, 1); o[a] = g[a] + 0.5f * vs * dim[a] - d[a] * far; }
        } else {
            vs = uni(0.01f, 0.3f);
            const int m = std::max(dim[0], std::max(dim[1], dim[2]));
            for (int a = 0; a < 3; a++) { g[a] = uni(-1, 1); o[a] = g[a] + uni(-1, 2) * vs * m; d[a] = g[a] + uni(0, 1) * vs * dim[a] - o[a]; }
        }
        int32_t lo[3] = { 0, 0, 0 }, hi[3] = { dim[0], dim[1], dim[2] };
        if (integer(0, 1)) for (int a = 0; a < 3; a++) { lo[a] = integer(0, dim[a] - 1); hi[a] = integer(lo[a] + 1, dim[a]); }
        const std::vector<ProjectionVoxel> want = brute(g, vs, dim, o, d, lo, hi);
        const std::vector<ProjectionVoxel> got = rto_host::projectionWalk(g, vs, dim, o, d, lo, hi);
        bool same = want.size() == got.size();
        for (size_t k = 0; same && k < want.size(); k++) same = want[k].x == got[k].x && want[k].y == got[k].y && want[k].z == got[k].z;
        if (!same) {
            std::printf("FAIL walk: ray %d kind %d dim %d %d %d: %zu voxels, the sorted statement has %zu\n", i, kind, dim[0], dim[1], dim[2],
                        got.size(), want.size());
            return 1;
        }
        if (want.empty()) continue;
        nonempty++;
        voxels += (long long)want.size();
        std::vector<int32_t> vol((size_t)dim[0] * dim[1] * dim[2]);
        for (size_t k = 0; k < vol.size(); k++) vol[k] = adversarial[(k * 7 + k / 5) % 10];
        const int32_t windows[3][2] = { { INT32_MIN + 2, INT32_MAX }, { 0, 0x7ffffffe }, { -7, -1 } };
        for (int op = RTO_PROJECT_MAX; op <= RTO_PROJECT_FIRST; op++)
            for (const auto& w : windows) {
                const rto_host::ProjectionResult r = rto_host::projectionReduce(vol.data(), dim, got.data(), (int64_t)got.size(), op, w[0], w[1]);
                int64_t sum = 0, count = 0, mx = 0, mn = 0, first = 0, vmx = -1, vmn = -1, vfirst = -1;
                for (const ProjectionVoxel& c : want) {
                    const int64_t idx = ((int64_t)c.z * dim[1] + c.y) * dim[0] + c.x;
                    const int64_t v = vol[(size_t)idx];
                    if (v < w[0] || v > w[1]) continue;
                    if (!count) { mx = mn = first = v; vmx = vmn = vfirst = idx; }
                    count++; sum += v;
                    if (v > mx) { mx = v; vmx = idx; }
                    if (v < mn) { mn = v; vmn = idx; }
                }
                int64_t value = RTO_FIELD_PIXEL_NONE, voxel = count ? vfirst : -1;
                if (count) {
                    if (op == RTO_PROJECT_MAX) { value = mx; voxel = vmx; }
                    else if (op == RTO_PROJECT_MIN) { value = mn; voxel = vmn; }
                    else if (op == RTO_PROJECT_MEAN) value = (int64_t)std::floor((long double)sum / (long double)count);
                    else if (op == RTO_PROJECT_COUNT) value = count;
                    else value = first;
                }
                if (r.value != value || r.voxel != voxel || r.sum != sum || r.count != count) {
                    std::printf("FAIL reduce: ray %d op %d window %d..%d: value %lld voxel %lld sum %lld count %lld, expected %lld %lld %lld %lld\n", i, op,
                                w[0], w[1], (long long)r.value, (long long)r.voxel, (long long)r.sum, (long long)r.count, (long long)value,
                                (long long)voxel, (long long)sum, (long long)count);
                    return 1;
                }
            }
    }
    if (nonempty * 4 < rays) { std::printf("FAIL: only %lld of %d rays visit a voxel\n", nonempty, rays); return 1; }
    std::printf("projection_selftest: %d rays, %lld visit the box, %lld voxels: the walk and the reductions equal the sorted statement\n", rays,
                nonempty, voxels);
    return 0;
}
