"""CPU: the per-limb arithmetic classes at the edges of their prime ranges (tests/class_edges.py).

Three layers, each checked against the one below it:
  - the catalogue itself: every entry is a prime = 1 mod 2N of its class, the first prime across each bound has another class, and the C rule of
    tables.h (through the emulator, which is built from it) agrees with the Python statement;
  - the reference (oracle.c), which the GPU tests are held to: its transforms and its ct_mul equal direct evaluation at the odd powers of psi and the
    negacyclic schoolbook product (Python integers) at every edge prime;
  - the per-thread kernel code (tools/emulate.cpp) at every edge prime, every geometry, extreme residues, with the lazy-arithmetic counters armed."""
import ctypes as C

import numpy as np
import pytest

from class_edges import FSCALED_KS, catalogue, entry_class, expected_class, neighbour
from deeppowers_amd.params import is_prime
from oracle import pyoracle as po
from oracle.cbind import Oracle
from test_emulated_kernels import GEOS, U, _class_patterns, emu, run  # noqa: F401  (emu: the module fixture that builds tools/libemu.so)

ARITH = {"shoup": 0, "fold": 1, "f64": 2, "fold_scaled": 3, "f64_wide": 4}
LOG2NS = (8, 10, 11, 12, 13, 14, 16)
EMU_LOG2NS = sorted({ln for ln, _ in GEOS})
# entries that start at their bound and run upwards (the prime across the bound lies below entry[0]); the others run downwards
UPWARD = ("fold_edge", "fscaled_edge_", "f64_wide_low", "shoup_above_", "smallest")


def _upward(name):
    return any(name == u or (u.endswith("_") and name.startswith(u)) for u in UPWARD)


@pytest.mark.parametrize("log2n", LOG2NS)
def test_catalogue_entries_are_edge_primes_of_their_class(log2n):
    n = 1 << log2n
    cat = catalogue(log2n)
    print(f"\nN = {n}: " + ", ".join(f"{name} {[hex(q) for q, _ in e]}" for name, e in cat.items()))
    for name in ("fold_edge", "fold_near", "shoup60", "f64_edge", "f64_wide_low", "f64_wide_edge", "smallest", "shoup_above_50", "shoup_above_59", "fscaled_out_59"):
        assert name in cat, name          # these exist at every N up to 65536
    for name, entry in cat.items():
        want = entry_class(name)
        qs = [q for q, _ in entry]
        assert 1 <= len(qs) <= 4 and len(set(qs)) == len(qs)
        assert qs == sorted(qs, reverse=not _upward(name)), name       # ordered from the bound inward
        for q, psi in entry:
            assert is_prime(q) and (q - 1) % (2 * n) == 0, (name, q)
            assert 0 < psi < q and pow(psi, n, q) == q - 1, (name, q)
            assert expected_class(q) == want, (name, hex(q), expected_class(q))
        if name in ("fold_near", "smallest") or name.startswith("fscaled_out_"):
            continue   # no bound on the far side (nothing below 2N + 1 is 1 mod 2N, nothing above 2^60 is a limb); fscaled_out_k: the pairs below
        across = neighbour(qs[0], log2n, -1 if _upward(name) else +1)
        assert across is not None and expected_class(across) != want, (name, hex(qs[0]), across)
    # the pairs that share a bound: nothing of either class lies between them
    assert neighbour(cat["fold_edge"][0][0], log2n, -1) == cat["shoup60"][0][0]
    assert neighbour(cat["f64_edge"][0][0], log2n, +1) == cat["f64_wide_low"][0][0]
    assert expected_class(neighbour(cat["shoup_above_59"][0][0], log2n, -1)) == "fold_scaled"
    for k in FSCALED_KS:
        if f"fscaled_edge_{k}" in cat:
            assert neighbour(cat[f"fscaled_edge_{k}"][0][0], log2n, -1) == cat[f"fscaled_out_{k}"][0][0], k
            assert expected_class(cat[f"fscaled_out_{k}"][0][0]) == ("f64_wide" if k <= 50 else "shoup")


@pytest.mark.parametrize("log2n", EMU_LOG2NS)
def test_the_c_rule_admits_exactly_the_catalogued_classes(emu, log2n):
    """tables.h through the emulator: each policy's entry point accepts a prime (0) or refuses it (2000) by the same rule as expected_class -
    fold_eligible, q < 2^47, fold_scaled_shift != 0, q < 2^50.  In particular fscaled_out_k is refused by FoldScaledArith and fscaled_edge_k taken."""
    n = 1 << log2n
    le = next(le for ln, le in GEOS if ln == log2n)
    z = np.zeros(n, np.uint64)
    for name, entry in catalogue(log2n).items():
        for q, psi in entry:
            want = {1: expected_class(q) == "fold", 2: q < (1 << 47), 3: expected_class(q) == "fold_scaled", 4: q < (1 << 50), 0: True}
            for arith, ok in want.items():
                rc, _ = run(emu, arith, log2n, le, 0, q, psi, z)
                assert rc == (0 if ok else 2000), (name, hex(q), arith, rc)
        if name.startswith("fscaled_out_"):
            assert run(emu, 3, log2n, le, 0, entry[0][0], entry[0][1], z)[0] == 2000
        if name.startswith("fscaled_edge_"):
            assert run(emu, 3, log2n, le, 0, entry[0][0], entry[0][1], z)[0] == 0


# ---- the reference at the edges ---------------------------------------------------------------------------------------------------------------------------
def _inputs(orc, n, q, seed):
    rnd = orc.fill(1, seed).ravel().copy()
    return [rnd, np.full(n, q - 1, np.uint64), np.where(np.arange(n) % 2 == 0, q - 1, 0).astype(np.uint64)]


def _inverse_definition(A, q, psi):
    """a_j = N^-1 sum_k A_k psi^-(2 brv(k) + 1) j: direct evaluation with Python integers"""
    n = len(A)
    bits = n.bit_length() - 1
    ninv, ipsi = pow(n, q - 2, q), pow(psi, q - 2, q)
    acc = [0] * n
    for k, Ak in enumerate(A):
        w, wj = pow(ipsi, 2 * po.bit_reverse(k, bits) + 1, q), Ak
        for j in range(n):
            acc[j] += wj
            wj = wj * w % q
    return [v * ninv % q for v in acc]


@pytest.mark.parametrize("name", sorted(catalogue(8)))
def test_oracle_is_exact_at_the_edge_primes_n256(name):
    """oracle.c ntt_fwd / ntt_inv equal direct evaluation at the odd powers of psi, and oracle.c ct_mul equals the negacyclic schoolbook product,
    with Python integers, at every prime of the entry: random words, all q - 1, alternating q - 1 / 0"""
    n = 256
    for i, (q, psi) in enumerate(catalogue(8)[name]):
        orc = Oracle(8, [q], [psi])
        pats = _inputs(orc, n, q, 300 + i)
        for a in pats:
            ai = [int(v) for v in a]
            assert [int(v) for v in orc.ntt_fwd(a)] == po.ntt_forward_definition(ai, q, psi), (hex(q), "fwd")
            assert [int(v) for v in orc.ntt_inv(a)] == _inverse_definition(ai, q, psi), (hex(q), "inv")
        for a0, a1, b0, b1 in ((pats[1], pats[1], pats[1], pats[1]), (pats[0], pats[2], pats[1], pats[0]), (pats[2], pats[1], pats[2], pats[0])):
            got = orc.ct_mul(np.stack([a0, a1]).reshape(1, 2, 1, n), np.stack([b0, b1]).reshape(1, 2, 1, n)).reshape(3, n)
            A0, A1, B0, B1 = ([int(v) for v in p] for p in (a0, a1, b0, b1))
            c1 = [(x + y) % q for x, y in zip(po.negacyclic_schoolbook(A0, B1, q), po.negacyclic_schoolbook(A1, B0, q))]
            want = [po.negacyclic_schoolbook(A0, B0, q), c1, po.negacyclic_schoolbook(A1, B1, q)]
            assert [[int(v) for v in row] for row in got] == want, (hex(q), "ct_mul")


@pytest.mark.parametrize("name", sorted(catalogue(12)))
def test_oracle_forward_transform_at_the_edge_primes_n4096_sampled(name):
    """N = 4096: 64 sampled output words of oracle.c's forward transform against direct evaluation, every prime of the entry, the same inputs"""
    n, bits = 4096, 12
    rng = np.random.default_rng(12)
    fixed = [0, n // 2 - 1, n // 2, n - 1]
    ks = fixed + [int(v) for v in rng.choice(np.setdiff1d(np.arange(n), fixed), 60, replace=False)]
    for i, (q, psi) in enumerate(catalogue(12)[name]):
        orc = Oracle(12, [q], [psi])
        for a in _inputs(orc, n, q, 400 + i):
            got = orc.ntt_fwd(a)
            ai = [int(v) for v in a]
            for k in ks:
                w, wj, acc = pow(psi, 2 * po.bit_reverse(k, bits) + 1, q), 1, 0
                for aj in ai:
                    acc += aj * wj
                    wj = wj * w % q
                assert int(got[k]) == acc % q, (hex(q), k)


# ---- the emulated kernels at the edges ----------------------------------------------------------------------------------------------------------------------
def _emu_entries(log2n):
    return [(name, q, psi) for name, e in catalogue(log2n).items() for q, psi in e]


@pytest.mark.parametrize("log2n", EMU_LOG2NS)
def test_emulated_transforms_at_the_edge_primes(emu, log2n):
    """emu_ntt on the policy of each catalogued prime's class, every geometry of GEOS at this N, both directions; emu_ntt_halves (N = 8192, fold and
    shoup) and emu_ntt_quarters (N = 16384, fold); no lazy-arithmetic precondition broken"""
    n = 1 << log2n
    emu.emu_ntt_halves.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint64, U, U]
    emu.emu_ntt_halves.restype = C.c_int
    emu.emu_ntt_quarters.argtypes = [C.c_int, C.c_uint64, C.c_uint64, U, U]
    emu.emu_ntt_quarters.restype = C.c_int
    before = emu.emu_overflows()
    geos = [le for ln, le in GEOS if ln == log2n]
    for name, q, psi in _emu_entries(log2n):
        cls = expected_class(q)
        orc = Oracle(log2n, [q], [psi])
        for a in _class_patterns(orc, n, q):
            a = np.ascontiguousarray(a)
            want = (orc.ntt_fwd(a), orc.ntt_inv(a))
            for le in geos:
                for inv in (0, 1):
                    rc, got = run(emu, ARITH[cls], log2n, le, inv, q, psi, a)
                    assert rc == 0 and np.array_equal(got, want[inv]), (name, hex(q), le, inv)
            for inv in (0, 1):
                out = np.zeros_like(a)
                if log2n == 13 and cls in ("fold", "shoup"):
                    assert emu.emu_ntt_halves(ARITH[cls], inv, q, psi, a.ctypes.data_as(U), out.ctypes.data_as(U)) == 0
                    assert np.array_equal(out, want[inv]), (name, hex(q), "halves", inv)
                if log2n == 14 and cls == "fold":
                    assert emu.emu_ntt_quarters(inv, q, psi, a.ctypes.data_as(U), out.ctypes.data_as(U)) == 0
                    assert np.array_equal(out, want[inv]), (name, hex(q), "quarters", inv)
    assert emu.emu_overflows() == before, "a lazy-arithmetic precondition was broken at an edge prime"


@pytest.mark.parametrize("log2n", [8, 10, 12, 13])
def test_emulated_fused_multiply_at_the_edge_primes(emu, log2n):
    """the fused multiply's data paths at every catalogued prime: emu_ct_mul (fold: lazy FoldArith products), emu_ct_mul_lazy_class (f64, f64_wide,
    fold_scaled: the quad / dual kernels' lazy products) and emu_ct_mul_class (the generic path through canonical words, shoup included), against
    oracle.c's ct_mul, with all q - 1 operands and mixtures of the extreme patterns"""
    n = 1 << log2n
    for fn in (emu.emu_ct_mul_lazy_class, emu.emu_ct_mul_class):
        fn.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint64, U, U, U, U, U]
        fn.restype = C.c_int
    emu.emu_ct_mul.argtypes = [C.c_int, C.c_uint64, C.c_uint64, U, U, U, U, U]
    emu.emu_ct_mul.restype = C.c_int
    before = emu.emu_overflows()
    for name, q, psi in _emu_entries(log2n):
        cls = expected_class(q)
        orc = Oracle(log2n, [q], [psi])
        p = _class_patterns(orc, n, q)
        for polys in ((p[1], p[1], p[1], p[1]), (p[0], p[3], p[1], p[4]), (p[5], p[1], p[3], p[2])):
            a0, a1, b0, b1 = (np.ascontiguousarray(v) for v in polys)
            want = orc.ct_mul(np.stack([a0, a1]).reshape(1, 2, 1, n), np.stack([b0, b1]).reshape(1, 2, 1, n)).reshape(3 * n)
            ptrs = [v.ctypes.data_as(U) for v in (a0, a1, b0, b1)]
            paths = []
            if cls == "fold":
                paths.append(("fold", lambda out: emu.emu_ct_mul(log2n, q, psi, *ptrs, out.ctypes.data_as(U))))
            else:
                if cls != "shoup":
                    paths.append(("lazy", lambda out: emu.emu_ct_mul_lazy_class(ARITH[cls], log2n, q, psi, *ptrs, out.ctypes.data_as(U))))
                paths.append(("generic", lambda out: emu.emu_ct_mul_class(ARITH[cls], log2n, q, psi, *ptrs, out.ctypes.data_as(U))))
            for path, call in paths:
                out = np.zeros(3 * n, np.uint64)
                assert call(out) == 0 and np.array_equal(out, want), (name, hex(q), path)
    assert emu.emu_overflows() == before, "a lazy-arithmetic precondition was broken at an edge prime"
