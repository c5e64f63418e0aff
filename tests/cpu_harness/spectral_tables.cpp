// The host part of dsp.jl_amd/csrc/spectral_tables.h -- the root table and the working-precision window every spectral plan uploads at its creation --
// printed for tests/test_spectral_tables_cpu.py to compare with numpy.  One value per line as the hexadecimal of its bits: nothing is lost in the text.
//   spectral_tables roots  f32|f64 n
//   spectral_tables window f32|f64 n nfft have_window       (the window is win[i] = 1 / (i + 3): one correctly rounded division, few values representable in Float32)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../dsp.jl_amd/csrc/spectral_tables.h"

static void put(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    std::printf("%08" PRIx32 "\n", u);
}
static void put(double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    std::printf("%016" PRIx64 "\n", u);
}

template <typename R> static int run(const std::string& what, char** arg) {
    if (what == "roots") {
        for (const auto& w : mdsp::root_table<R>(std::atoll(arg[0]))) {
            put(w.x);
            put(w.y);
        }
        return 0;
    }
    const int n = std::atoi(arg[0]);
    const int64_t nfft = std::atoll(arg[1]);
    std::vector<double> win((size_t)n);
    for (int i = 0; i < n; ++i) win[(size_t)i] = 1.0 / (i + 3.0);
    for (R v : mdsp::working_window<R>(std::atoi(arg[2]) ? win.data() : nullptr, n, nfft)) put(v);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const std::string what = argv[1], prec = argv[2];
    if ((what != "roots" && what != "window") || (what == "window" && argc < 6)) return 2;
    return prec == "f64" ? run<double>(what, argv + 3) : run<float>(what, argv + 3);
}
