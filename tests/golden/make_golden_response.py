#!/usr/bin/env python3
"""Pack the reference's golden data of the filter responses into ``tests/golden/response_golden.npz``.

    DSP_REFERENCE=<a checkout of DSP.jl> python tests/golden/make_golden_response.py

Reads the tab-delimited decimal text files that DSP.jl's ``test/filter_response.jl`` loads with ``read_reference_data`` (``readdlm``: one line per
matrix row) and keeps that orientation -- MATLAB results for b = 0.05634 conv([1, 1], [1, -1.0166, 1]), a = conv([1, -0.683], [1, -1.4461, 0.7957]):

  freqz-eg1.txt      2001 x 2: w, abs(h)                                  test/filter_response.jl:17-18
  responses-eg1.txt  512 x 5:  f, impz, stepz, abs(freqz), phasez        test/filter_response.jl:87-111
  grpdelay_eg1.txt   512 x 2:  w, grpdelay                                test/filter_response.jl:200-211
"""
import os
import sys

import numpy as np

REF = os.environ.get("DSP_REFERENCE", "")
DATA = os.path.join(REF, "test", "data")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "response_golden.npz")


def read_reference_data(name):
    """readdlm(file, '\\t') as a 2-D array: row r = line r."""
    rows = []
    with open(os.path.join(DATA, name + ".txt")) as f:
        for line in f:
            line = line.strip()
            if line:
                rows.append([float(tok) for tok in line.split("\t")])
    return np.array(rows, dtype=np.float64)


def main():
    if not REF or not os.path.isdir(DATA):
        sys.exit("set DSP_REFERENCE to a checkout of DSP.jl (its test/data directory is read)")
    arrays = {"freqz_eg1": read_reference_data("freqz-eg1"),
              "responses_eg1": read_reference_data("responses-eg1"),
              "grpdelay_eg1": read_reference_data("grpdelay_eg1")}
    for k, v in arrays.items():
        print(f"{k:14s} {v.shape}")
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
