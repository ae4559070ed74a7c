"""CPU: the per-lane code of the sum of tensor products (csrc/mul_sum.h MulSumLane, what kernels_mul.h tensor3_sum_kernel runs between its loads and its
stores) emulated word position by word position (tools/emulate_mul_sum.cpp) against Python integers, for every arithmetic policy that takes the prime, with the
precondition counter of the lazy sums (DPFHE_EMU_ASSERT) armed: it must stay at zero.  Columns and term counts: tests/mul_sum_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import sympy

from mul_sum_ref import KINDS, TERMS, column, want

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64P = C.POINTER(C.c_uint64)
CLASSES = {"shoup": 0, "fold": 1, "f64": 2, "fold_scaled": 3, "f64_wide": 4}   # csrc/tables.h LimbClass
# per class: primes at the edges of what it takes
PRIMES = {
    "fold": ((1 << 60) - 93, (1 << 60) - 16383, int(sympy.nextprime((1 << 60) - (1 << 24)))),          # d small, the pinned chain's size, d just below 2^24
    "f64": (12289, 2013265921, int(sympy.prevprime(1 << 47))),
    "fold_scaled": ((1 << 48) - 59, (1 << 55) - 55, (1 << 59) - 55),
    "f64_wide": (int(sympy.prevprime((1 << 50) - (1 << 45))), int(sympy.prevprime(1 << 50))),
    "shoup": (12289, int(sympy.prevprime((1 << 59) + (1 << 57))), (1 << 60) - 93, int(sympy.prevprime((1 << 60) - (1 << 30)))),
}


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu") / "libemu_mul_sum.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "emulate_mul_sum.cpp")])
    lib = C.CDLL(so)
    lib.emu_mul_sum.argtypes = [C.c_int, C.c_uint64, U64P, U64P, U64P, U64P, C.c_size_t, U64P, U64P]
    lib.emu_mul_sum.restype = C.c_int
    lib.emu_mul_sum_takes.argtypes = [C.c_int, C.c_uint64]
    lib.emu_mul_sum_overflows.restype = C.c_long
    return lib


def run(emu, cls, q, cols, prev=None):
    arrs = [(C.c_uint64 * len(c))(*c) for c in cols]
    out = (C.c_uint64 * 3)()
    p = (C.c_uint64 * 3)(*prev) if prev is not None else None
    assert emu.emu_mul_sum(CLASSES[cls], q, *arrs, len(cols[0]), p, out) == 0
    return tuple(int(v) for v in out)


def test_declared_periods_are_covered_by_the_term_counts(emu):
    """every fold period p the header declares, at p - 1, p, p + 1 and 2 p + 1 products: the outer components take one product per term, the middle one two"""
    for which, per_term in ((0, 1), (1, 2)):
        p = emu.emu_mul_sum_period(which)
        assert 1 <= p <= 8
        for products in (p - 1, p, p + 1, 2 * p + 1):
            assert {products // per_term, -(-products // per_term)} - {0} <= set(TERMS), (which, products)
    assert {1, 2, 3, 16, 17, 64} <= set(TERMS)


@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_policy_takes_its_primes_only(emu, cls):
    for q in PRIMES[cls]:
        assert sympy.isprime(q) and emu.emu_mul_sum_takes(CLASSES[cls], q) == 1
    assert emu.emu_mul_sum(CLASSES["fold"], (1 << 55) - 55, None, None, None, None, 1, None, None) == 2000
    if cls in ("fold", "f64", "fold_scaled", "f64_wide"):
        assert emu.emu_mul_sum_takes(CLASSES[cls], int(sympy.prevprime((1 << 59) + (1 << 57)))) == 0


@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_lane_sums_match_python_integers(emu, cls):
    rng = np.random.default_rng(CLASSES[cls] + 19)
    for q in PRIMES[cls]:
        for terms in TERMS:
            for kind in KINDS:
                for _ in range(3 if kind == "random" else 1):
                    cols = column(q, terms, kind, rng)
                    assert run(emu, cls, q, cols) == want(q, *cols), (cls, q, terms, kind)
    assert emu.emu_mul_sum_overflows() == 0


@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_accumulate_continues_from_a_canonical_result(emu, cls):
    """the kernel's `accumulate`: a sum cut into two ranges of terms, the second starting from the first's canonical words, gives the words of the whole;
    and a start from q - 1 in every component (the largest canonical word) on top of the largest products"""
    rng = np.random.default_rng(CLASSES[cls] + 23)
    for q in PRIMES[cls]:
        for terms in TERMS:
            for cut in sorted({1, terms // 2, terms - 1} - {0, terms}):
                for kind in ("random", "all_max", "land_qm1", "land_half"):
                    cols = column(q, terms, kind, rng)
                    first = run(emu, cls, q, [c[:cut] for c in cols])
                    assert first == want(q, *[c[:cut] for c in cols])
                    assert run(emu, cls, q, [c[cut:] for c in cols], prev=first) == want(q, *cols), (cls, q, terms, cut, kind)
            cols = column(q, terms, "all_max", rng)
            assert run(emu, cls, q, cols, prev=(q - 1,) * 3) == want(q, *cols, prev=(q - 1,) * 3)
    assert emu.emu_mul_sum_overflows() == 0
