// Host check of the folded butterflies of dsp.jl_amd/csrc/fft_lds.h (bfly16_tw, bfly8_tw, bfly16_tail<DIR, true>, bfly16_h): a product that
// only feeds an add / subtract pair rides in the pair as three fused multiply-adds.  On the host fft_lds.h compiles the scalar forms, one
// fmaf per half of each packed instruction the kernels issue, in the same order.  Every entry runs on random Float32 inputs next to the
// unfolded form it replaces (twmul_all + bfly16 / bfly8, the plain bfly16_tail, product + bfly16), both against a long-double DFT.
// Built and run by tests/test_fold_butterflies.py with g++ (no GPU needed); also meant to run under -fsanitize=address,undefined.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>

#include "../../dsp.jl_amd/csrc/fft_lds.h"

using namespace mdsp::fft;
typedef std::complex<long double> zl;
static const long double PI = 3.141592653589793238462643383279502884L;

static uint64_t rng_state = 1776;   // splitmix64: the same inputs on every host
static double uniform() {
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    z ^= z >> 31;
    return (double)(z >> 11) / 9007199254740992.0 - 0.5;
}
static cx<float> rnd() { return {(float)uniform(), (float)uniform()}; }
static cx<float> unit_root() {   // a twiddle as the tables hold it: a Float32 rounding of a point on the unit circle
    const long double a = 2 * PI * (long double)uniform();
    return {(float)cosl(a), (float)sinl(a)};
}
static zl Z(cx<float> a) { return {a.x, a.y}; }

// DFT of RDX points x[n] f[n], exponent sign DIR, in long double
template <int RDX> static void dft(const zl (&x)[RDX], int dir, zl (&X)[RDX]) {
    for (int k = 0; k < RDX; ++k) {
        zl acc = 0;
        for (int n = 0; n < RDX; ++n) {
            const long double a = (dir < 0 ? -2 : 2) * PI * (long double)((n * k) % RDX) / RDX;
            acc += x[n] * zl(cosl(a), sinl(a));
        }
        X[k] = acc;
    }
}
template <int RDX> static double relerr(const cx<float> (&v)[RDX], const zl (&ref)[RDX]) {
    long double e2 = 0, n2 = 0;
    for (int k = 0; k < RDX; ++k) {
        e2 += std::norm(Z(v[k]) - ref[k]);
        n2 += std::norm(ref[k]);
    }
    return (double)sqrtl(e2 / n2);
}

struct Pair {
    double plain = 0, folded = 0;   // maximum over the trials of || got - ref || / || ref ||
};

// bfly16_tw / bfly8_tw against twmul_all + bfly; WDIR < 0 with W0 is the spectrum-product entry bfly16_h against product + bfly16
template <int RDX, int DIR, bool SPECTRUM> static Pair check_tw(int trials) {
    Pair r;
    for (int it = 0; it < trials; ++it) {
        cx<float> v[RDX], w[RDX], a[RDX], b[RDX];
        zl x[RDX], ref[RDX];
        for (int i = 0; i < RDX; ++i) {
            v[i] = rnd();
            w[i] = SPECTRUM ? cx<float>{(float)(2 * uniform()), (float)(2 * uniform())} : unit_root();   // a filter spectrum is no unit root
            if (i == 0 && !SPECTRUM) w[0] = {1.f, 0.f};
            const zl wl = (SPECTRUM || DIR < 0) ? Z(w[i]) : std::conj(Z(w[i]));
            x[i] = Z(v[i]) * wl;
            a[i] = b[i] = v[i];
        }
        dft<RDX>(x, DIR, ref);
        if constexpr (SPECTRUM) {
            for (int i = 0; i < RDX; ++i) a[i] = cmul(a[i], w[i]);
            bfly<RDX, DIR>(a);
            bfly16_h<DIR>(b, w);
        } else {
            twmul_all<DIR, RDX>(a, w);
            bfly<RDX, DIR>(a);
            if constexpr (RDX == 16) bfly16_tw<DIR>(b, w);
            else bfly8_tw<DIR>(b, w);
        }
        r.plain = std::max(r.plain, relerr<RDX>(a, ref));
        r.folded = std::max(r.folded, relerr<RDX>(b, ref));
    }
    return r;
}

// bfly16_tail<DIR, true> against bfly16_tail<DIR>: v[m + 4q] = y[m][q] in, X[4p + q] = sum_m W4^{mp} W16^{mq} y[m][q] out (natural order)
template <int DIR> static Pair check_tail(int trials) {
    Pair r;
    for (int it = 0; it < trials; ++it) {
        cx<float> a[16], b[16];
        zl ref[16];
        for (int i = 0; i < 16; ++i) a[i] = b[i] = rnd();
        for (int p = 0; p < 4; ++p)
            for (int q = 0; q < 4; ++q) {
                zl acc = 0;
                for (int m = 0; m < 4; ++m) {
                    const long double ang = (DIR < 0 ? -2 : 2) * PI * (long double)((4 * m * p + m * q) % 16) / 16;
                    acc += Z(a[m + 4 * q]) * zl(cosl(ang), sinl(ang));
                }
                ref[4 * p + q] = acc;
            }
        bfly16_tail<DIR>(a);
        bfly16_tail<DIR, true>(b);
        r.plain = std::max(r.plain, relerr<16>(a, ref));
        r.folded = std::max(r.folded, relerr<16>(b, ref));
    }
    return r;
}

static int report(const char* name, Pair f, Pair i) {
    const Pair r = {std::max(f.plain, i.plain), std::max(f.folded, i.folded)};
    const bool ok = r.folded <= 2 * r.plain && r.plain < 1e-6;   // one more rounding in `minus`: at most twice the unfolded form's error
    printf("%-12s unfolded %.3e folded %.3e ratio %.3f %s\n", name, r.plain, r.folded, r.folded / r.plain, ok ? "ok" : "FAIL");
    return ok ? 0 : 1;
}

int main() {
    const int trials = 4000;
    int bad = 0;
    bad |= report("bfly16_tw", check_tw<16, -1, false>(trials), check_tw<16, +1, false>(trials));
    bad |= report("bfly8_tw", check_tw<8, -1, false>(trials), check_tw<8, +1, false>(trials));
    bad |= report("bfly16_tail", check_tail<-1>(trials), check_tail<+1>(trials));
    bad |= report("bfly16_h", check_tw<16, +1, true>(trials), check_tw<16, -1, true>(trials));
    printf(bad ? "FAIL\n" : "OK\n");
    return bad;
}
