"""CPU: the static error bounds of the approximate family (SlotSum, ApproxPolynomial, ApproxInvSqrt, ApproxProductSum) and
ApproxInvSqrt::balanced_guess_scale are the SAME DOUBLES, bit for bit, as tests/golden/approx_bounds.json over the grid of
tests/cpp/bounds/approx_bounds.cpp (log2 N 12 and 15; 3 and 7 data primes; degrees 2, 7, 15; 1 and 3 Newton steps; 1 and 8 terms; blocks 2 and 64).

The fixture was recorded with this program from the library of commit c609eff, the last one before the bounds were rewritten on one shared kit of
units (N, H, u, u8), key-switch term and level ladder: the rewrite may move an expression into a helper, never change the order of its operations.
A point the library rejects is recorded as its error code.  No device is opened."""
import json
import os
import subprocess

import cpp_build

GOLDEN = os.path.join(cpp_build.ROOT, "tests", "golden", "approx_bounds.json")


def test_bounds_are_the_recorded_doubles():
    os.makedirs(os.path.join(cpp_build.BIN_DIR, "bounds"), exist_ok=True)   # (cpp_build makes tests/cpp/bin but no directory below it)
    exe = cpp_build.build_program("bounds/approx_bounds")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    got = out.stdout.splitlines()
    with open(GOLDEN) as f:
        want = json.load(f)
    assert len(want) == 44 and sum("error" not in l for l in want) == 38   # the grid; six points need more limbs than the three-prime chain has
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
