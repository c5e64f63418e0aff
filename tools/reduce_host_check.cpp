// Stand-alone host check of the reduce and shift entry points that need no device: mdsp_reduce_geometry_for / mdsp_reduce_emulate (the host emulation of
// the device code, csrc/reduce_op.h) against serial definitions for every cut and phase, and mdsp_shift_geometry_for / mdsp_shift_emulate (the planner and
// the host walk of its schedules, csrc/shift_plan.h) against the plain shift for every route and unit order -- meant to be built with the host side under
// AddressSanitizer and UndefinedBehaviorSanitizer (a program of its own: nothing is preloaded, no device is touched):
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/reduce_host_check.cpp dsp.jl_amd/csrc/reduce.hip dsp.jl_amd/csrc/shift.hip -o build/reduce_host_check && build/reduce_host_check
//
// The two sources need one symbol of the rest of the library, mdsp::set_error; this file supplies it.
#include <cmath>
#include <complex>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

static const int64_t SEGMENTS[] = {0, 1, 2, 3, 7, 64, 1000000};

template <typename T> static long double abs2l(T x) { return (long double)x * (long double)x; }
template <typename R> static long double abs2l(std::complex<R> x) { return (long double)x.real() * x.real() + (long double)x.imag() * x.imag(); }
template <typename T> static void fill(std::vector<T>& v, std::mt19937_64& gen) {
    std::normal_distribution<double> g;
    for (auto& e : v) e = (T)g(gen);
}
template <typename R> static void fill(std::vector<std::complex<R>>& v, std::mt19937_64& gen) {
    std::normal_distribution<double> g;
    for (auto& e : v) e = std::complex<R>((R)g(gen), (R)g(gen));
}

// SUMABS2 and SUMABS2_W on an (inner, len, outer) array against long double sums: within depth x 2^-53 (+ 3 roundings inside a Float64 term)
template <typename T> static void check_sums(int dtype, bool weighted, int64_t inner, int64_t len, int64_t outer, std::mt19937_64& gen) {
    const int op = weighted ? MDSP_REDUCE_SUMABS2_W : MDSP_REDUCE_SUMABS2, words = weighted ? 2 : 1;
    const double step = 0.00625;
    std::vector<T> x((size_t)(inner * len * outer));
    fill(x, gen);
    std::vector<double> out((size_t)(inner * outer * words));
    for (int64_t seg : SEGMENTS)
        for (int64_t phase = 0; phase < 4; ++phase) {
            int route = -1;
            int64_t S = 0, seglen = 0, depth = 0, ws = 0, reached = -1;
            EXPECT(mdsp_reduce_geometry_for(inner, len, outer, op, dtype, seg, &route, &S, &seglen, &depth, &ws) == MDSP_OK, "geometry");
            EXPECT(route == (inner == 1 ? 0 : 1) && S >= 1 && (len == 0 || ((S - 1) * seglen < len && len <= S * seglen)), "segments do not tile the line");
            EXPECT(ws == (S > 1 ? inner * outer * S * 8 * words : 0), "workspace");
            std::fill(out.begin(), out.end(), -1.0);
            EXPECT(mdsp_reduce_emulate(x.data(), out.data(), inner, len, outer, op, dtype, step, 0, seg, phase, &reached) == MDSP_OK, "emulate");
            EXPECT(reached <= depth, "depth %lld < reached %lld", (long long)depth, (long long)reached);
            for (int64_t o = 0; o < outer; ++o)
                for (int64_t i = 0; i < inner; ++i) {
                    long double num = 0, den = 0;
                    for (int64_t j = 0; j < len; ++j) {
                        const T v = x[(size_t)(i + inner * (j + len * o))];
                        if (weighted) {
                            // the terms as the library rounds them (abs2 in the element's real type, the two products in Float64): only the additions differ
                            const auto re = std::real(v), im = std::imag(v);
                            const decltype(re) p = (decltype(re))((decltype(re))(re * re) + (decltype(re))(im * im));
                            num += (long double)((double)p * (double)(step * (double)j));
                            den += (long double)(double)p;
                        } else den += abs2l(v);
                    }
                    const long double tol = 1.01L * (long double)(depth + 3) * 0x1p-53L;
                    const int64_t line = i + inner * o;
                    if (weighted) {
                        EXPECT(std::fabs((long double)out[(size_t)(2 * line)] - num) <= tol * num, "weighted sum, segments %lld", (long long)seg);
                        EXPECT(std::fabs((long double)out[(size_t)(2 * line + 1)] - den) <= tol * den, "sum of weights, segments %lld", (long long)seg);
                    } else EXPECT(std::fabs((long double)out[(size_t)line] - den) <= tol * den, "sum, dtype %d segments %lld phase %lld", dtype, (long long)seg, (long long)phase);
                }
        }
}

// util.jl:338-346 on one line: larger |x|, then nearer to centre, then the smaller index; NaN raises the flag and does not compete
template <typename T> static void rule(const T* x, int64_t inc, int64_t len, int64_t centre, int64_t* idx, int64_t* flag) {
    double best = -1.0;
    *idx = -1;
    *flag = 0;
    for (int64_t j = 0; j < len; ++j) {
        const double v = std::fabs((double)x[j * inc]);
        if (std::isnan(v)) {
            *flag = 1;
            continue;
        }
        const int64_t dj = j > centre ? j - centre : centre - j, db = *idx > centre ? *idx - centre : centre - *idx;
        if (v > best || (v == best && dj < db)) {
            best = v;
            *idx = j;
        }
    }
}

template <typename T> static void check_argmax(int dtype, int64_t inner, int64_t len, int64_t outer, std::mt19937_64& gen) {
    std::vector<T> x((size_t)(inner * len * outer));
    std::uniform_int_distribution<int> small(-3, 3);            // few distinct magnitudes: ties everywhere
    for (auto& e : x) e = (T)small(gen);
    if (len > 10) {
        x[(size_t)(inner * 4)] = (T)NAN;
        x[(size_t)(inner * 7)] = (T)INFINITY;
        x[(size_t)(inner * (len - 2))] = -(T)INFINITY;
    }
    std::vector<int64_t> out((size_t)(inner * outer * 2));
    for (int64_t seg : SEGMENTS)
        for (int64_t centre : {(int64_t)0, len / 2, len - 1 > 0 ? len - 1 : 0, len + 9})
            for (int64_t phase = 0; phase < 4; ++phase) {
                std::fill(out.begin(), out.end(), -9);
                EXPECT(mdsp_reduce_emulate(x.data(), out.data(), inner, len, outer, MDSP_REDUCE_ABSARGMAX, dtype, 0.0, centre, seg, phase, nullptr) == MDSP_OK, "emulate");
                for (int64_t o = 0; o < outer; ++o)
                    for (int64_t i = 0; i < inner; ++i) {
                        int64_t idx, flag;
                        rule<T>(x.data() + i + inner * len * o, inner, len, centre, &idx, &flag);
                        const int64_t line = i + inner * o;
                        EXPECT(out[(size_t)(2 * line)] == idx && out[(size_t)(2 * line + 1)] == flag, "argmax %lldx%lldx%lld segments %lld centre %lld: %lld, want %lld",
                               (long long)inner, (long long)len, (long long)outer, (long long)seg, (long long)centre, (long long)out[(size_t)(2 * line)], (long long)idx);
                    }
            }
}

template <typename E> static void check_shift(int64_t tile) {
    const int64_t esize = (int64_t)sizeof(E);
    for (int64_t l : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)3, tile - 1, tile, tile + 1, 2 * tile + 1, 5 * tile + 3}) {
        std::vector<E> x((size_t)l), want((size_t)l), got((size_t)l);
        for (int64_t k = 0; k < l; ++k) std::memset(&x[(size_t)k], (int)(1 + k % 250), sizeof(E));
        for (int64_t s = -l - 1; s <= l + 1; s += (l > 3 * tile ? 7 : 1)) {
            for (int64_t i = 0; i < l; ++i) {
                if (i - s >= 0 && i - s < l) want[(size_t)i] = x[(size_t)(i - s)];
                else std::memset(&want[(size_t)i], 0, sizeof(E));
            }
            for (int in_place = 0; in_place < 2; ++in_place)
                for (int route = MDSP_SHIFT_AUTO; route <= MDSP_SHIFT_STAGED; ++route) {
                    int r = -1;
                    int64_t t = 0, chunk = 0, ntiles = 0, ws = 0;
                    const int st = mdsp_shift_geometry_for(l, s, esize, in_place, tile, route, &r, &t, &chunk, &ntiles, &ws);
                    const int64_t a = s < 0 ? -s : s;
                    if (a > l) {
                        EXPECT(st == MDSP_ERR_DOMAIN, "|s| > l must be a domain error");
                        continue;
                    }
                    const bool overlap = in_place && a > 0 && 2 * a < l;
                    const bool allowed = route == MDSP_SHIFT_DISJOINT ? !overlap : route == MDSP_SHIFT_HALO ? (in_place && a > 0) : true;
                    EXPECT((st == MDSP_OK) == allowed, "route %d in_place %d l %lld s %lld: status %d", route, in_place, (long long)l, (long long)s, st);
                    if (st != MDSP_OK) continue;
                    EXPECT(ws == esize * (r == MDSP_SHIFT_HALO ? ntiles * a : r == MDSP_SHIFT_STAGED ? l - a : 0), "workspace");
                    for (int order = 0; order < 3; ++order) {
                        int64_t bad = -1;
                        got = x;
                        std::vector<E> dst((size_t)l);
                        E* y = in_place ? got.data() : dst.data();
                        EXPECT(mdsp_shift_emulate(got.data(), y, l, s, esize, tile, route, order, &bad) == MDSP_OK, "shift emulate");
                        EXPECT(bad == 0 && (l == 0 || std::memcmp(y, want.data(), (size_t)(l * esize)) == 0), "shift l %lld s %lld route %d->%d in_place %d order %d: %lld violations",
                               (long long)l, (long long)s, route, r, in_place, order, (long long)bad);
                    }
                }
        }
    }
}

struct E4 { unsigned char b[4]; };
struct E8 { unsigned char b[8]; };
struct E16 { unsigned char b[16]; };

int main() {
    std::mt19937_64 gen(7);
    const int64_t shapes[][3] = {{1, 0, 1}, {1, 1, 1}, {1, 2, 3}, {1, 63, 1}, {1, 65, 2}, {1, 257, 1}, {1, 1023, 2}, {1, 10007, 1}, {2, 17, 1}, {3, 1000, 3}, {65, 17, 2}, {64, 2, 1}, {5, 1, 2}};
    for (const auto& sh : shapes) {
        check_sums<float>(MDSP_F32, false, sh[0], sh[1], sh[2], gen);
        check_sums<double>(MDSP_F64, false, sh[0], sh[1], sh[2], gen);
        check_sums<std::complex<float>>(MDSP_C32, false, sh[0], sh[1], sh[2], gen);
        check_sums<std::complex<double>>(MDSP_C64, false, sh[0], sh[1], sh[2], gen);
        check_sums<std::complex<float>>(MDSP_C32, true, sh[0], sh[1], sh[2], gen);
        check_sums<std::complex<double>>(MDSP_C64, true, sh[0], sh[1], sh[2], gen);
        check_argmax<float>(MDSP_F32, sh[0], sh[1], sh[2], gen);
        check_argmax<double>(MDSP_F64, sh[0], sh[1], sh[2], gen);
    }
    for (int64_t tile : {16, 64, 256}) {
        check_shift<E4>(tile);
        check_shift<E8>(tile);
        check_shift<E16>(tile);
    }
    float x[4] = {0, 0, 0, 0};
    double out[4];
    EXPECT(mdsp_reduce_emulate(x, out, 1, -4, 1, MDSP_REDUCE_SUMABS2, MDSP_F32, 0, 0, 0, 0, nullptr) == MDSP_ERR_ARGUMENT, "negative size");
    EXPECT(mdsp_reduce_emulate(x, out, 1, 4, 1, MDSP_REDUCE_SUMABS2_W, MDSP_F32, 0, 0, 0, 0, nullptr) == MDSP_ERR_ARGUMENT, "real bins");
    EXPECT(mdsp_reduce_emulate(x, out, 1, 4, 1, MDSP_REDUCE_ABSARGMAX, MDSP_C32, 0, 0, 0, 0, nullptr) == MDSP_ERR_ARGUMENT, "complex arg-max");
    EXPECT(mdsp_reduce_geometry_for(1, INT64_MAX / 2, 4, 0, MDSP_F32, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == MDSP_ERR_ARGUMENT, "overflowing size");
    int64_t S = 0, seglen = 0;
    EXPECT(mdsp_reduce_geometry_for(1, (int64_t)1 << 33, 1, 0, MDSP_F32, 0, nullptr, &S, &seglen, nullptr, nullptr) == MDSP_OK && (S - 1) * seglen < ((int64_t)1 << 33) &&
               ((int64_t)1 << 33) <= S * seglen, "2^33 elements");
    EXPECT(mdsp_shift_geometry_for(10, 1, 3, 1, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == MDSP_ERR_ARGUMENT, "element size 3");
    std::printf(failures ? "%d failure(s)\n" : "reduce host check: all passed (%d failures)\n", failures);
    return failures ? 1 : 0;
}
