"""CPU: the per-lane code of the products with a shared complement factor (csrc/mul_complement.h MulComplementLane, what kernels_mul.h
tensor3_complement_kernel runs between its loads and its stores) emulated word position by word position (tools/emulate_mul_complement.cpp) against Python
integers, for every arithmetic policy that takes the prime, with the precondition counter of the lazy products (DPFHE_EMU_ASSERT) armed: it must stay at
zero.  Columns and item counts: tests/mul_complement_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import sympy

import mul_complement_ref as mc
from test_emulated_mul_sum import CLASSES, PRIMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64P = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu") / "libemu_mul_complement.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "emulate_mul_complement.cpp")])
    lib = C.CDLL(so)
    lib.emu_mul_complement.argtypes = [C.c_int, C.c_uint64, U64P, U64P, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64, U64P, U64P]
    lib.emu_mul_complement.restype = C.c_int
    lib.emu_mul_complement_takes.argtypes = [C.c_int, C.c_uint64]
    lib.emu_mul_complement_overflows.restype = C.c_long
    return lib


def run(emu, cls, q, x0, x1, b0, b1, kappa):
    """-> (the factor's two words, [items] triples)"""
    n = len(x0)
    f, out = (C.c_uint64 * 2)(), (C.c_uint64 * (3 * n))()
    assert emu.emu_mul_complement(CLASSES[cls], q, (C.c_uint64 * n)(*x0), (C.c_uint64 * n)(*x1), n, b0, b1, kappa, f, out) == 0
    return (int(f[0]), int(f[1])), [tuple(int(v) for v in out[3 * k:3 * k + 3]) for k in range(n)]


@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_policy_takes_its_primes_only(emu, cls):
    for q in PRIMES[cls]:
        assert sympy.isprime(q) and emu.emu_mul_complement_takes(CLASSES[cls], q) == 1
    assert emu.emu_mul_complement(CLASSES["fold"], (1 << 55) - 55, None, None, 1, 0, 0, 0, None, None) == 2000


@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_factor_is_canonical_on_its_edges(emu, cls):
    """f0 = 0 (b0 = kappa), f0 = kappa (b0 = 0), f0 = q - 1 (b0 = kappa + 1); f1 = 0 for b1 = 0 - not q -, f1 = q - 1 for b1 = 1; kappa in {0, 1, q - 1}"""
    rng = np.random.default_rng(CLASSES[cls] + 31)
    for q in PRIMES[cls]:
        for kk in mc.KAPPA_KINDS:
            kappa = mc.kappa_of(q, kk, rng)
            for kind, f0, f1 in (("b0_kappa", 0, None), ("b0_zero", kappa, None), ("b0_kappa_p1", q - 1, None), ("b1_zero", None, 0), ("b1_one", None, q - 1)):
                b0, b1 = mc.denominator(q, kappa, kind, rng)
                f, _ = run(emu, cls, q, [1], [1], b0, b1, kappa)
                assert f == mc.factor(q, b0, b1, kappa) and f[0] < q and f[1] < q, (cls, q, kk, kind)
                assert (f0 is None or f[0] == f0) and (f1 is None or f[1] == f1), (cls, q, kk, kind, f)
    assert emu.emu_mul_complement_overflows() == 0


@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_lane_products_match_python_integers(emu, cls):
    """every denominator kind under every kappa kind, 1, 4, 5 and 9 numerators and the self product: random words, the largest, and products solved to land on
    0, 1, q - 1 and either side of q / 2"""
    rng = np.random.default_rng(CLASSES[cls] + 37)
    assert set(mc.ITEMS) == {1, 4, 5, 9}
    for q in PRIMES[cls]:
        for kk in mc.KAPPA_KINDS:
            kappa = mc.kappa_of(q, kk, rng)
            for kind in mc.B_KINDS:
                for items in mc.ITEMS:
                    for first in range(0, len(mc.ms.KINDS), 3):
                        b0, b1 = mc.denominator(q, kappa, kind, rng)
                        x0, x1 = mc.numerators(q, items, *mc.factor(q, b0, b1, kappa), rng, first=first)
                        x0, x1 = x0 + [b0], x1 + [b1]                        # the self product last
                        _, got = run(emu, cls, q, x0, x1, b0, b1, kappa)
                        assert got == mc.want(q, x0, x1, b0, b1, kappa), (cls, q, kk, kind, items, first)
    assert emu.emu_mul_complement_overflows() == 0


def test_planted_operands_are_their_own_reference():
    """the builder the GPU test uses: shapes, canonical words, and every landing target present among the words it expects"""
    q = PRIMES["fold"][0]
    a, b, out = mc.planted_operands((q, 12289), 64, 9, (q - 1, 1), 3)
    assert a.shape == (9, 2, 2, 64) and b.shape == (2, 2, 64) and out.shape == (10, 3, 2, 64)
    assert int(a[:, :, 0].max()) < q and int(a[:, :, 1].max()) < 12289 and int(out[:, :, 1].max()) < 12289
    assert {0, 1, q - 1, q // 2, q // 2 + 1} <= set(int(v) for v in out[:, 0, 0].ravel())
