// Stand-alone host check of the unwrap entry points that need no device: mdsp_unwrap_geometry_for and mdsp_unwrap_emulate_host (the host emulation of the
// device code, csrc/unwrap_scan.h) against the serial recurrence of src/unwrap.jl:25,34, out of place and in place, for every cut -- meant to be built with
// the host side under AddressSanitizer and UndefinedBehaviorSanitizer (a program of its own: nothing is preloaded, no device is touched):
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/unwrap_host_check.cpp dsp.jl_amd/csrc/unwrap.hip -o build/unwrap_host_check && build/unwrap_host_check
//
// unwrap.hip needs one symbol of the rest of the library, mdsp::set_error; this file supplies it.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../include/mi355dsp.h"

namespace mdsp {
int set_error(int code, const char* fmt, ...) {
    (void)fmt;
    return code;
}
}  // namespace mdsp

static int failures = 0;
#define EXPECT(cond, ...)                  \
    do {                                   \
        if (!(cond)) {                     \
            ++failures;                    \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");             \
        }                                  \
    } while (0)

// accumulate!(unwrap_kernel(range), y, m; dims) on an (inner, len, outer) array; built with -ffp-contract=off: one rounding per operation
template <typename T> static void serial(const std::vector<T>& m, std::vector<T>& y, int64_t inner, int64_t len, int64_t outer, T range) {
    for (int64_t o = 0; o < outer; ++o)
        for (int64_t i = 0; i < inner; ++i) {
            const int64_t base = i + inner * len * o;
            if (len > 0) y[base] = m[base];
            for (int64_t j = 1; j < len; ++j) {
                const T cur = m[base + inner * j], prev = y[base + inner * (j - 1)];
                const T q = (cur - prev) / range;
                const T r = std::nearbyint(q) * range;
                y[base + inner * j] = cur - r;
            }
        }
}

template <typename T> static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    for (size_t k = 0; k < a.size(); ++k)
        if (!(a[k] == b[k] || (std::isnan(a[k]) && std::isnan(b[k])))) return false;   // signed zeros equal, NaN equals NaN
    return true;
}

template <typename T> static void run_case(const char* name, const std::vector<T>& m, int64_t inner, int64_t len, int64_t outer, double range, int dtype) {
    std::vector<T> ref(m.size()), out(m.size());
    serial<T>(m, ref, inner, len, outer, (T)range);
    for (int64_t seg : {0, 1, 2, 3, 7, 1000000}) {
        int route = -1;
        int64_t S = 0, seglen = 0, ws = 0;
        EXPECT(mdsp_unwrap_geometry_for(inner, len, outer, dtype, seg, &route, &S, &seglen, &ws) == MDSP_OK, "%s geometry", name);
        EXPECT(route == (inner == 1 ? 0 : 1) && S >= 1 && (len == 0 || ((S - 1) * seglen < len && len <= S * seglen)), "%s: segments do not tile the line", name);
        std::fill(out.begin(), out.end(), (T)-1);
        EXPECT(mdsp_unwrap_emulate_host(m.data(), out.data(), inner, len, outer, dtype, range, seg) == MDSP_OK, "%s emulate", name);
        EXPECT(same(out, ref), "%s segments %lld out of place", name, (long long)seg);
        out = m;
        EXPECT(mdsp_unwrap_emulate_host(out.data(), out.data(), inner, len, outer, dtype, range, seg) == MDSP_OK, "%s emulate in place", name);
        EXPECT(same(out, ref), "%s segments %lld in place", name, (long long)seg);
    }
}

template <typename T> static void all_cases(int dtype) {
    std::mt19937_64 gen(dtype + 1);
    std::uniform_real_distribution<double> step(-2.8, 2.8);   // wrapped random walk: tie margin >= (pi - 2.8) / 2 pi
    const double two_pi = 2.0 * (double)(T)M_PI;
    const int64_t shapes[][3] = {{1, 1, 1}, {1, 2, 3}, {1, 3, 1}, {1, 65, 2}, {1, 1000, 1}, {1, 10007, 1}, {2, 17, 1}, {3, 1000, 3}, {65, 17, 2}, {64, 2, 1}, {5, 1, 2}};
    for (const auto& sh : shapes) {
        const int64_t inner = sh[0], len = sh[1], outer = sh[2];
        std::vector<T> m((size_t)(inner * len * outer));
        for (int64_t o = 0; o < outer; ++o)
            for (int64_t i = 0; i < inner; ++i) {
                double u = 0.0;
                for (int64_t j = 0; j < len; ++j) {
                    u += step(gen);
                    m[(size_t)(i + inner * (j + len * o))] = (T)(u - 2.0 * M_PI * std::nearbyint(u / (2.0 * M_PI)));
                }
            }
        char name[64];
        std::snprintf(name, sizeof name, "walk %lldx%lldx%lld dtype %d", (long long)inner, (long long)len, (long long)outer, dtype);
        run_case<T>(name, m, inner, len, outer, two_pi, dtype);
        if (len >= 17) {   // a non-finite sample inside, one at the start
            std::vector<T> bad = m;
            bad[(size_t)(inner * 9)] = (T)INFINITY;
            run_case<T>("inf inside", bad, inner, len, outer, two_pi, dtype);
            bad = m;
            bad[0] = (T)NAN;
            run_case<T>("nan first", bad, inner, len, outer, two_pi, dtype);
            bad[0] = -(T)INFINITY;
            run_case<T>("-inf first", bad, inner, len, outer, two_pi, dtype);
        }
    }
    std::vector<T> mod(100);
    for (int k = 0; k < 100; ++k) mod[(size_t)k] = (T)((k + 1) % 10);
    run_case<T>("mod 10", mod, 1, 100, 1, 10.0, dtype);
    const std::vector<T> a{(T)0.1, (T)3, (T)-3, (T)INFINITY, (T)0.2, (T)0.3}, b{(T)INFINITY, (T)3, (T)-3, (T)0.2};
    run_case<T>("stated case 1", a, 1, 6, 1, two_pi, dtype);
    run_case<T>("stated case 2", b, 1, 4, 1, two_pi, dtype);
    run_case<T>("empty", std::vector<T>(), 3, 0, 2, two_pi, dtype);
    // beyond the documented range the result is unspecified, the call must stay defined: increments that overflow, counts far above 2^24
    const T big = std::numeric_limits<T>::max();
    std::vector<T> wild{big, -big, big, (T)0, (T)1e30, (T)-1e30, (T)5, big}, out(wild.size());
    for (int64_t seg : {1, 3})
        EXPECT(mdsp_unwrap_emulate_host(wild.data(), out.data(), 1, (int64_t)wild.size(), 1, dtype, 1e-3, seg) == MDSP_OK, "wild increments");
}

int main() {
    all_cases<float>(MDSP_F32);
    all_cases<double>(MDSP_F64);
    float x[4] = {0, 0, 0, 0};
    EXPECT(mdsp_unwrap_emulate_host(x, x, 1, -4, 1, MDSP_F32, 1.0, 0) == MDSP_ERR_ARGUMENT, "negative size");
    EXPECT(mdsp_unwrap_emulate_host(x, x, 1, 4, 1, MDSP_F32, 0.0, 0) == MDSP_ERR_ARGUMENT, "range 0");
    EXPECT(mdsp_unwrap_emulate_host(x, x, 1, 4, 1, MDSP_C32, 1.0, 0) == MDSP_ERR_ARGUMENT, "complex dtype");
    EXPECT(mdsp_unwrap_geometry_for(1, INT64_MAX / 2, 4, MDSP_F32, 0, nullptr, nullptr, nullptr, nullptr) == MDSP_ERR_ARGUMENT, "overflowing size");
    std::printf(failures ? "%d failure(s)\n" : "unwrap host check: all passed (%d failures)\n", failures);
    return failures ? 1 : 0;
}
