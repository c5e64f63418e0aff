"""build.SOURCES against csrc/: every translation unit is compiled exactly once, and every listed unit exists."""
import glob
import importlib
import os

import dsp_jl_amd  # noqa: F401  (the import shim that gives the package its importable name)

build = importlib.import_module("dsp_jl_amd.build")   # the module: the package's `build` attribute is its build() function


def test_every_hip_file_is_built_exactly_once():
    on_disk = sorted(os.path.basename(p) for p in glob.glob(os.path.join(build.CSRC, "*.hip")))
    assert on_disk, "no sources found"
    assert sorted(build.SOURCES) == on_disk   # (sorted lists: a file listed twice, an orphan and a stale entry all differ)
