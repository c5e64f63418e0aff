"""The folded butterflies of the headline overlap-save kernel on the host (tests/cpu_harness/fold_emul.cpp, no GPU): fft_lds.h's scalar forms -- one
fmaf per half of each packed instruction, in the kernel's order -- of bfly16_tw, bfly8_tw, bfly16_tail<DIR, true> and the spectrum-product entry
bfly16_h, next to the unfolded forms they replace, both against a long-double DFT of the same random Float32 inputs (seed 1776, 4000 butterflies per
direction).  A fold forms (a + W b, a - W b) in three multiply-adds; the difference carries one more rounding than the sum, so a folded entry may
show at most TWICE the unfolded form's maximum relative error.  Measured (maximum over the trials of ||got - ref|| / ||ref||, unfolded -> folded):
bfly16_tw 1.298e-07 -> 1.271e-07, bfly8_tw 1.330e-07 -> 1.229e-07, bfly16_tail 9.695e-08 -> 9.367e-08, bfly16_h 1.320e-07 -> 1.301e-07."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_folded_butterflies_on_the_host(tmp_path):
    exe = str(tmp_path / "fold_emul")
    r = subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpu_harness", "fold_emul.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    rows = dict((m.group(1), (float(m.group(2)), float(m.group(3)))) for m in re.finditer(r"^(\w+)\s+unfolded (\S+) folded (\S+) ratio", r.stdout, re.M))
    assert sorted(rows) == ["bfly16_h", "bfly16_tail", "bfly16_tw", "bfly8_tw"], r.stdout[-3000:]
    for name, (plain, folded) in rows.items():
        assert 0 < plain < 1e-6, (name, plain)              # the unfolded form itself is a Float32 butterfly
        assert folded <= 2 * plain, (name, plain, folded)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:]
