"""CPU: the per-lane code of the all-pairs tensor product (csrc/mul_outer.h MulOuterLane, what kernels_mul.h tensor3_outer_kernel runs between its loads and
its stores) emulated word position by word position (tools/emulate_mul_outer.cpp) against Python integers, for every arithmetic policy that takes the prime,
with the precondition counter of the lazy products (DPFHE_EMU_ASSERT) armed: it must stay at zero.  A query is prepared ONCE and multiplied by all the keys, as
the kernel does.  Columns: tests/mul_outer_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import sympy

import mul_outer_ref as mo
from test_emulated_mul_sum import CLASSES, PRIMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64P = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu") / "libemu_mul_outer.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "emulate_mul_outer.cpp")])
    lib = C.CDLL(so)
    lib.emu_mul_outer.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, U64P, U64P, C.c_size_t, U64P]
    lib.emu_mul_outer.restype = C.c_int
    lib.emu_mul_outer_takes.argtypes = [C.c_int, C.c_uint64]
    lib.emu_mul_outer_overflows.restype = C.c_long
    return lib


def run(emu, cls, q, a0, a1, b0, b1):
    """one prepared query against the keys -> [keys] triples"""
    n = len(b0)
    out = (C.c_uint64 * (3 * n))()
    assert emu.emu_mul_outer(CLASSES[cls], q, a0, a1, (C.c_uint64 * n)(*b0), (C.c_uint64 * n)(*b1), n, out) == 0
    return [tuple(int(v) for v in out[3 * j:3 * j + 3]) for j in range(n)]


@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_policy_takes_its_primes_only(emu, cls):
    for q in PRIMES[cls]:
        assert sympy.isprime(q) and emu.emu_mul_outer_takes(CLASSES[cls], q) == 1
    assert emu.emu_mul_outer(CLASSES["fold"], (1 << 55) - 55, 0, 0, None, None, 1, None) == 2000
    assert emu.emu_mul_outer_mid_products() == 2


@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_lane_products_match_python_integers(emu, cls):
    """every query kind against every key kind, at every rotation of the kinds: operands 0, 1, q - 1, the largest halves, and keys solved so that the products
    land on 0, 1, q - 1 and either side of q / 2"""
    rng = np.random.default_rng(CLASSES[cls] + 41)
    for q in PRIMES[cls]:
        landed = set()
        for first in range(len(mo.K_KINDS)):
            a0, a1, b0, b1 = mo.column(q, 9, 2 * len(mo.K_KINDS), rng, first=first)
            wants = mo.products(q, a0, a1, b0, b1)
            for i in range(9):
                got = run(emu, cls, q, a0[i], a1[i], b0, b1)
                assert got == wants[i], (cls, q, first, i)
                landed |= {w for t in got for w in t}
        assert {0, 1, q - 1, q // 2, q // 2 + 1} <= landed, (cls, q)
    assert emu.emu_mul_outer_overflows() == 0


def test_fold_columns_at_their_largest(emu):
    """the pair that maximises the middle component's Dot30 columns - both products of halves at their largest -, with the assertions of the stated bounds
    (mul_outer.h: s0 < 2, s1 < 4, s2 < 2 in units of 2^60) armed: all four words on q - 1 (high halves 2^30 - 1), on 2^60 - 2^30 - 1 (low halves 2^30 - 1),
    and every mixture of the two"""
    for q in PRIMES["fold"]:
        big = (q - 1, mo.lowmax(q))
        assert big[1] == (1 << 60) - (1 << 30) - 1 and big[1] & 0x3fffffff == 0x3fffffff and (q - 1) >> 30 == 0x3fffffff
        for a0 in big:
            for a1 in big:
                b0, b1 = [x for x in big for _ in big], [y for _ in big for y in big]
                assert run(emu, "fold", q, a0, a1, b0, b1) == [mo.want(q, a0, a1, x, y) for x, y in zip(b0, b1)]
    assert emu.emu_mul_outer_overflows() == 0


def test_planted_operands_are_their_own_reference():
    """the builder the GPU test uses: shapes, canonical words, every landing target present among the words it expects, and the two layouts"""
    q = PRIMES["fold"][0]
    a, b, out = mo.planted_operands((q, 12289), 64, 5, 9, 3)
    assert a.shape == (5, 2, 2, 64) and b.shape == (9, 2, 2, 64) and out.shape == (5, 9, 3, 2, 64)
    assert int(a[:, :, 0].max()) < q and int(a[:, :, 1].max()) < 12289 and int(out[:, :, :, 1].max()) < 12289
    assert {0, 1, q - 1, q // 2, q // 2 + 1} <= set(int(v) for v in out[:, :, :, 0].ravel())
    assert {0, 1, q - 1, mo.lowmax(q)} <= set(int(v) for v in a[:, :, 0].ravel()) and {0, 1, q - 1, mo.lowmax(q)} <= set(int(v) for v in b[:, :, 0].ravel())
    full = mo.full_layout(out)
    assert full.shape == (45, 3, 2, 64) and np.array_equal(full[2 * 9 + 7], out[2, 7])
    sq = out[:, :5]
    causal = mo.causal_layout(sq)
    assert causal.shape == (15, 3, 2, 64) and np.array_equal(causal[4 * 5 // 2 + 3], sq[4, 3]) and np.array_equal(causal[0], sq[0, 0])
