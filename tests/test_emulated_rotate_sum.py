"""CPU: the per-lane code of the hoisted slot sums (csrc/rotate_sum.h QpSumLane, what kernels_rotate_sum.h hoisted_qp_sum_kernel runs between its loads and
its stores) emulated one word pair of one tile at a time (tools/emulate_rotate_sum.cpp) against Python integers, for every arithmetic policy that takes the
prime, with the precondition counter of the lazy sums (DPFHE_EMU_ASSERT) armed: it must stay at zero.  The emulator walks the kernel's term loop - R rotations
of J terms, the fold period counted across rotations.  Columns: tests/rotate_sum_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import sympy

import rotate_sum_ref as rs
from test_emulated_mul_sum import CLASSES, PRIMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64P = C.POINTER(C.c_uint64)
P_SPECIAL = (1 << 60) - 93        # reduced by the lane (p_operand), whatever the prime


def build_emulator(directory):
    """tools/emulate_rotate_sum.cpp as a shared library with its prototypes set (tests/test_remainder_edges_cpu.py builds it too)"""
    so = os.path.join(str(directory), "libemu_rotate_sum.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "emulate_rotate_sum.cpp")])
    lib = C.CDLL(so)
    lib.emu_rotate_sum.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint, C.c_int, C.c_int, C.c_uint, U64P, U64P, U64P]
    lib.emu_rotate_sum.restype = C.c_int
    lib.emu_rotate_sum_takes.argtypes = [C.c_int, C.c_uint64]
    lib.emu_rotate_sum_overflows.restype = C.c_long
    lib.emu_rotate_sum_notes_reset.restype = None
    lib.emu_rotate_sum_notes_get.argtypes = [C.POINTER(C.c_uint), C.c_int]
    return lib


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build_emulator(tmp_path_factory.mktemp("emu"))


def run(emu, cls, q, p_special, J, has_p, x, keys):
    """the lane over the column's terms -> [rows][4] Python integers (c0 half 0, c0 half 1, c1 half 0, c1 half 1)"""
    total, rows = len(x), len(x[0])
    assert total % J == 0 and len(keys) == total
    xs, ks = np.array(x, np.uint64).reshape(-1), np.array(keys, np.uint64).reshape(-1)
    out = np.zeros(rows * 4, np.uint64)
    assert emu.emu_rotate_sum(CLASSES[cls], q, p_special, total // J, J, int(has_p), rows, xs.ctypes.data_as(U64P), ks.ctypes.data_as(U64P), out.ctypes.data_as(U64P)) == 0
    return [[int(v) for v in out[4 * i:4 * i + 4]] for i in range(rows)]


@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_policy_takes_its_primes_only(emu, cls):
    for q in PRIMES[cls]:
        assert sympy.isprime(q) and emu.emu_rotate_sum_takes(CLASSES[cls], q) == 1
    z = (C.c_uint64 * 16)()
    assert emu.emu_rotate_sum(CLASSES["fold"], (1 << 55) - 55, 1, 1, 1, 0, 1, z, z, z) == 2000
    assert emu.emu_rotate_sum(CLASSES["fold"], PRIMES["fold"][0], 1, 1, 1, 0, 5, z, z, z) == 2000          # more rows than a tile holds
    assert emu.emu_rotate_sum_tile() == 4 and emu.emu_rotate_sum_period() == rs.PERIOD


@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_lane_sums_match_python_integers(emu, cls):
    """R in {1, 2, 9, 64} rotations of J in {1, 2, 4, 8, 9, 15, 41} terms, with and without the P c0 term, 1 to 4 live rows (all four at every shape on the
    fold lane, cycling on the others), operands from {0, 1, q - 1, lowmax, random}"""
    rng = np.random.default_rng(CLASSES[cls] + 71)
    shape = 0
    for q in PRIMES[cls]:
        p = P_SPECIAL % q
        for R in rs.ROTATIONS:
            for J in rs.TERMS_PER_ROTATION:
                for has_p in ((0, 1) if J >= 2 else (0,)):
                    shape += 1
                    for rows in ((1, 2, 3, 4) if cls == "fold" else (1 + shape % 4,)):
                        x, keys = rs.column(q, R, J, rows, rng, first=shape + rows)
                        assert run(emu, cls, q, P_SPECIAL, J, has_p, x, keys) == rs.want(q, p, J, has_p, x, keys), (cls, hex(q), R, J, has_p, rows)
    assert emu.emu_rotate_sum_overflows() == 0


SATURATED_SHAPES = ((17, 1, 0), (1, 17, 0), (2, 9, 1), (3, 6, 1), (9, 2, 1), (5, 4, 1), (3, 8, 0), (3, 8, 1), (64, 9, 1), (9, 41, 1))     # (R, J, has_p): 17+ terms


def test_fold_columns_at_their_largest(emu):
    """every gathered word and every key word on q - 1 (high half 2^30 - 1) or on lowmax = 2^60 - 2^30 - 1 (low half 2^30 - 1), every mixture of the two and
    both alternations, the P operand on lowmax: each period of eight terms brings its columns as near 2^64 as canonical words can, over two full periods and
    a remainder at least, and the words still equal Python integers with no assertion fired"""
    for q in PRIMES["fold"]:
        low = rs.lowmax(q)
        assert low == (1 << 60) - (1 << 30) - 1 and low & rs.MASK30 == rs.MASK30 and (q - 1) >> 30 == rs.MASK30
        for R, J, has_p in SATURATED_SHAPES:
            assert R * J >= 2 * rs.PERIOD + 1
            for xp in range(4):
                for kp in range(4):
                    x, keys = rs.saturated_column(q, R, J, 1 + (xp + kp) % 4, xp, kp)
                    assert run(emu, "fold", q, low, J, has_p, x, keys) == rs.want(q, low, J, has_p, x, keys), (hex(q), R, J, has_p, xp, kp)
    assert emu.emu_rotate_sum_overflows() == 0


def test_the_saturated_words_are_sharp():
    """in Python integers: eight terms of the saturated words keep the middle column below 2^64, nine put it at or above (9 * 2 * (2^30 - 1)^2 > 2^64), so a
    schedule one term too long wraps on exactly these words - and then computes another residue"""
    assert 8 * 2 * rs.MASK30 ** 2 < 1 << 64 < 9 * 2 * rs.MASK30 ** 2
    for q in PRIMES["fold"]:
        big = (q - 1, rs.lowmax(q))
        for a in big:
            for b in big:
                assert 8 * rs.dot30_columns([(a, b)])[1] < 1 << 64 <= 9 * rs.dot30_columns([(a, b)])[1], (hex(q), a, b)
                assert 7 * rs.dot30_columns([(a, b)])[1] < 14 << 60              # what dot30_mac asserts before the eighth term
                pairs = [(a, b)] * 17
                assert rs.dot30_columns(pairs[:8]) == rs.dot30_columns(pairs[:8], wrap=False)
                assert rs.dot30_columns(pairs[:9]) != rs.dot30_columns(pairs[:9], wrap=False)
                exact = 17 * a * b % q
                assert rs.lazy_sum(q, pairs, rs.PERIOD) == exact and rs.lazy_sum(q, pairs, rs.PERIOD + 1) != exact
