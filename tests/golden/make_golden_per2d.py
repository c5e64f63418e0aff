#!/usr/bin/env python3
"""Pack the reference's golden data of the 2-D periodogram into ``tests/golden/per2d_golden.npz``.

Run in the authoring container (where ``/root/reference`` is mounted):

    python tests/golden/make_golden_per2d.py

Reads the tab-delimited decimal text files that DSP.jl's "2D" testset loads with ``read_reference_data``
(``test/FilterTestHelpers.jl:8``, ``readdlm``: one line per matrix row) and keeps that orientation:

  per2dx.txt     data2d, 32 x 32                       test/periodograms.jl:270
  per2dsum.txt   vec(...): radialsum of data2d (17)    test/periodograms.jl:271, :275 (Octave raPsd2d with nansum)
  per2dmean.txt  vec(...): radialavg of data2d (17)    test/periodograms.jl:272, :280 (Octave raPsd2d)
"""
import os
import sys

import numpy as np

REF = os.environ.get("DSP_REFERENCE", "/root/reference")
DATA = os.path.join(REF, "test", "data")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "per2d_golden.npz")


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
    if not os.path.isdir(DATA):
        sys.exit(f"reference data directory not found: {DATA}")
    arrays = {"per2dx": read_reference_data("per2dx"),
              "per2dsum": read_reference_data("per2dsum").ravel(order="F"),      # vec(...)
              "per2dmean": read_reference_data("per2dmean").ravel(order="F")}
    for k, v in arrays.items():
        print(f"{k:12s} {v.shape}")
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
