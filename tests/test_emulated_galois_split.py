"""CPU: dpfhe_ntt_inv_galois at N = 32768 and 65536 - the Galois form of the split inverse transform - in the thread-by-thread emulator
(tools/emulate.cpp emu_ctx_ntt_inv_galois): the sub-transform kernel's own per-thread code (source sub-block and offset per sub-block, gather plan,
staged loads, LDS rows) and the column stages, on the bytes csrc/ctx_tables.h builds, word for word against the oracle's
sigma_g(INTT(x)) and with the lazy-arithmetic overflow counters armed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import class_edges
from deeppowers_amd.params import ntt_primes
from oracle import pyoracle as po
from oracle.cbind import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = C.POINTER(C.c_uint64)
LAUNCH, GENERIC = 0, 3   # tools/emulate.cpp emu_ctx_ntt's `form`


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(ROOT, "tools", "libemu.so")
    src = os.path.join(ROOT, "tools", "emulate.cpp")
    deps = [src] + [os.path.join(ROOT, "deeppowers_amd", "csrc", f) for f in ("ntt_core.h", "ntt_top.h", "ntt_halves.h", "ntt_quarters.h", "modarith.h", "tables.h", "ctx_tables.h", "devtables.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src])
    lib = C.CDLL(so)
    lib.emu_overflows.restype = C.c_long
    lib.emu_ctx_ntt_inv_galois.argtypes = [C.c_int, C.c_int, U, U, C.c_int, C.c_int, C.c_uint32, U, U]
    lib.emu_ctx_ntt_inv_galois.restype = C.c_int
    return lib


def _fold_primes_n32768():
    """two fold primes = 1 mod 2^16, found as tests/test_emulated_kernels.py _fold_primes_n32768 finds them"""
    n = 1 << 15
    qs = [c for c in ((1 << 60) - (k * 2 * n - 1) for k in range(1, 1 << (24 - 15 - 1))) if c % (2 * n) == 1 and po.is_prime(c)][:2]
    return qs, [po.min_primitive_2n_root(n, q) for q in qs]


def _primes_n65536():
    p = ntt_primes(16, 2)
    return list(p.moduli), list(p.psi)


def elements(ln):
    """the identity, 3 and its inverse, -1, an element that is 1 mod 2 N1 (every sub-block is its own source, with a non-zero offset), a far power of 3"""
    two_n, n1 = 2 << ln, 1 << (ln - 12)
    return [1, 3, pow(3, -1, two_n), two_n - 1, 2 * n1 + 1, pow(3, 77, two_n)]


@pytest.mark.parametrize("ln,primes,forms", [(15, _fold_primes_n32768, (LAUNCH, GENERIC)), (16, _primes_n65536, (LAUNCH, GENERIC))], ids=["n32768", "n65536"])
def test_emulated_split_galois_inverse_matches_oracle(emu, ln, primes, forms):
    qs, psis = primes()
    n, L = 1 << ln, len(qs)
    assert {class_edges.expected_class(q) for q in qs} == {"fold"}
    m, w = np.array(qs, np.uint64), np.array(psis, np.uint64)
    before = emu.emu_overflows()
    for limb, (q, psi) in enumerate(zip(qs, psis)):
        orc = Oracle(ln, [q], [psi])
        for x in (orc.fill(1, 900 + limb).ravel().copy(), np.full(n, q - 1, np.uint64)):
            x = np.ascontiguousarray(x, dtype=np.uint64)
            inv = orc.ntt_inv(x)
            for g in elements(ln):
                want = orc.apply_galois(inv, g)
                for form in forms:
                    out = np.zeros_like(x)
                    rc = emu.emu_ctx_ntt_inv_galois(ln, L, m.ctypes.data_as(U), w.ctypes.data_as(U), limb, form, g, x.ctypes.data_as(U), out.ctypes.data_as(U))
                    assert rc == 0 and np.array_equal(out, want), (limb, g, form)
    assert emu.emu_overflows() == before, "lazy arithmetic wrapped around 2^64"


def test_emulated_split_galois_inverse_rejects_what_the_entry_rejects(emu):
    qs, psis = _fold_primes_n32768()
    m, w = np.array(qs, np.uint64), np.array(psis, np.uint64)
    x, out = np.zeros(1 << 15, np.uint64), np.zeros(1 << 15, np.uint64)
    args = (15, 2, m.ctypes.data_as(U), w.ctypes.data_as(U), 0, LAUNCH)
    assert emu.emu_ctx_ntt_inv_galois(*args, 2, x.ctypes.data_as(U), out.ctypes.data_as(U)) == 2000        # even
    assert emu.emu_ctx_ntt_inv_galois(*args, 1 << 16, x.ctypes.data_as(U), out.ctypes.data_as(U)) == 2000  # >= 2N
