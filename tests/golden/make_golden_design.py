#!/usr/bin/env python3
"""Pack the yardsticks of the filter-design tests into ``tests/golden/design_golden.npz`` (a few kilobytes; the tests read only that file).

    DSP_REFERENCE=<a checkout of DSP.jl> python tests/golden/make_golden_design.py

Two groups.

From DSP.jl's ``test/data`` (decimal text files, read as ``make_golden_response.py`` reads them):

  freqs-eg1.txt                                        50 x 3: w, abs(h), phase in degrees (MATLAB freqs)     test/filter_response.jl:164-183
  digitalfilter_hamming_12{8,9}_{bandpass,highpass,bandstop}[_scaled]_*.txt   SciPy firwin taps               test/filter_design.jl:998-1080
  (the low-pass tap files are in dsp_golden.npz already)

From ``scipy.signal`` (an independent implementation of the same designs), each as ``<name>_z``, ``<name>_p``, ``<name>_k``:

  ap_<family>_<n>                   buttap(n), cheb1ap(n, 1), cheb2ap(n, 1), ellipap(n, 0.5, 40) at n = 1, 2, 5, 8
  dig_<family>_<band>_<n>           butter(n, Wn), cheby1(n, 1, Wn), cheby2(n, 40, Wn), ellip(n, 0.5, 40, Wn), output="zpk", n = 4, 7, for
                                    lowpass 0.2, highpass 0.3, bandpass (0.1, 0.4), bandstop (0.25, 0.35)
  ana_<family>_<band>_<n>           the same with analog=True at the edges 4 tan(pi Wn / 2) (``ana_edges_<band>``), the pre-warped edges of a
                                    bilinear transform at a sampling frequency of 2
  iirnotch_b, iirnotch_a            iirnotch(0.2, 0.2 / 0.05)
"""
import math
import os
import sys

import numpy as np

REF = os.environ.get("DSP_REFERENCE", "")
DATA = os.path.join(REF, "test", "data")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "design_golden.npz")

TAP_FILES = [
    "digitalfilter_hamming_128_bandpass_fc0.1_0.2_fs1.0", "digitalfilter_hamming_128_bandpass_scaled_fc0.1_0.2_fs1.0",
    "digitalfilter_hamming_129_bandpass_fc0.1_0.2_fs1.0", "digitalfilter_hamming_129_bandpass_scaled_fc0.1_0.2_fs1.0",
    "digitalfilter_hamming_129_bandstop_fc0.1_0.2_fs1.0", "digitalfilter_hamming_129_bandstop_scaled_fc0.1_0.2_fs1.0",
    "digitalfilter_hamming_129_highpass_fc0.25_fs1.0", "digitalfilter_hamming_129_highpass_scaled_fc0.25_fs1.0",
]
BANDS = {"lowpass": 0.2, "highpass": 0.3, "bandpass": (0.1, 0.4), "bandstop": (0.25, 0.35)}
PROTOTYPE_ORDERS = (1, 2, 5, 8)
DESIGN_ORDERS = (4, 7)


def read_reference_data(name):
    """readdlm(file, '\\t') as a 2-D array: row r = line r; a single column or row as a vector."""
    rows = []
    with open(os.path.join(DATA, name + ".txt")) as f:
        for line in f:
            line = line.strip()
            if line:
                rows.append([float(tok) for tok in line.replace(",", " ").split()])
    a = np.array(rows, dtype=np.float64)
    return a[:, 0] if a.shape[1] == 1 else (a[0] if a.shape[0] == 1 else a)


def main():
    if not REF or not os.path.isdir(DATA):
        sys.exit("set DSP_REFERENCE to a checkout of DSP.jl (its test/data directory is read)")
    import scipy.signal as ss
    arrays = {"freqs_eg1": read_reference_data("freqs-eg1")}
    for name in TAP_FILES:
        arrays[name.replace(".", "p")] = read_reference_data(name)

    def put(name, zpk):
        z, p, k = zpk
        arrays[name + "_z"] = np.atleast_1d(np.asarray(z, dtype=np.complex128))
        arrays[name + "_p"] = np.atleast_1d(np.asarray(p, dtype=np.complex128))
        arrays[name + "_k"] = np.float64(k)

    for n in PROTOTYPE_ORDERS:
        put(f"ap_butter_{n}", ss.buttap(n))
        put(f"ap_cheby1_{n}", ss.cheb1ap(n, 1))
        put(f"ap_cheby2_{n}", ss.cheb2ap(n, 1))
        put(f"ap_ellip_{n}", ss.ellipap(n, 0.5, 40))
    families = {"butter": lambda n, wn, **kw: ss.butter(n, wn, **kw), "cheby1": lambda n, wn, **kw: ss.cheby1(n, 1, wn, **kw),
                "cheby2": lambda n, wn, **kw: ss.cheby2(n, 40, wn, **kw), "ellip": lambda n, wn, **kw: ss.ellip(n, 0.5, 40, wn, **kw)}
    for band, wn in BANDS.items():
        warped = np.array([4 * math.tan(math.pi * w / 2) for w in np.atleast_1d(wn)])
        arrays[f"ana_edges_{band}"] = warped
        for fam, design in families.items():
            for n in DESIGN_ORDERS:
                put(f"dig_{fam}_{band}_{n}", design(n, wn, btype=band, output="zpk"))
                put(f"ana_{fam}_{band}_{n}", design(n, warped if len(warped) > 1 else warped[0], btype=band, analog=True, output="zpk"))
    b, a = ss.iirnotch(0.2, 0.2 / 0.05)
    arrays["iirnotch_b"], arrays["iirnotch_a"] = np.asarray(b, np.float64), np.asarray(a, np.float64)
    np.savez_compressed(OUT, **arrays)
    print(f"{len(arrays)} arrays; wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
