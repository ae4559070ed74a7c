"""CPU: the host twin of the last pass of a rotate-and-add step (include/dpfhe.h dpfhe_rotate_add_pass_host; csrc/rotate_add.h) against Python integers
(tests/rotate_add_ref.py: the division by P through the CRT integer of the coefficient, the automorphism as a(X^g) mod X^N + 1).

Rings N = 256 (less than one 512-word chunk) and N = 1024; the pinned 60-bit primes at Ld = 2 and Ld = 4 (FoldArith's folds), the widest generic primes and a
mixed-class context (the 128-bit Barrett path); elements 3, 3^(N/4), 2N - 1 and 2N - 3.  Planted on item 0: every combination of round(work / P), c0[k] and the
gathered word in {0, 1, q - 1}, the gathered word at a non-negated and at a negated position - the negation of 0 and the three-term sum 3 q - 3 among them -
over the six edges of P on the special limb.  The device kernel shares the per-word functions and is held to the oracle by tests/test_gpu_rotate_add.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

import class_edges
import fused_rescale_ref as fr
import rotate_add_ref as ra
from deeppowers_amd import _cabi

CONTEXTS = {
    "pinned_ld2": lambda ln: fr.pinned(ln, 3),
    "pinned_ld4": lambda ln: fr.pinned(ln, 5),
    "shoup": lambda ln: class_edges.edge_moduli("shoup", ln),               # four generic primes, 60 / 60 / 60 / 51 bits
    "f64_under_fold": lambda ln: class_edges.edge_moduli("f64_under_fold", ln),   # narrow data limbs under a fold special prime
}
ALL = {(r, d, s, neg) for r, d, s in itertools.product(ra.WORDS, repeat=3) for neg in (False, True)}


def expected_combinations(g, n):
    """3 and 2N - 3 offer all 54.  The other two are degenerate, and the plan holds what they offer: 3^(N/4) = N + 1 maps every coefficient onto itself (odd ones
    negated), so the gathered word IS the direct one; 2N - 1 maps k to -k, so every position but 0 is negated and position 0, which gathers itself, takes
    the first non-negated combination alone."""
    if g == n + 1:
        return {c for c in ALL if c[1] == c[2]}
    if g == 2 * n - 1:
        return {c for c in ALL if c[3]} | {("0", "0", "0", False)}
    return ALL


@pytest.mark.parametrize("log2n", (8, 10))
@pytest.mark.parametrize("name", sorted(CONTEXTS))
def test_pass_twin_equals_the_integers(name, log2n):
    p = CONTEXTS[name](log2n)
    for i, g in enumerate(ra.elements(p.n)):
        work, in2, plan = ra.pass_inputs(p, 2, 31 * log2n + i, g)
        # the integers reach every planted combination, on every data limb at once, over all six edges of P (a check of the test's own construction)
        got = ra.reached(p, work, in2, g, plan)
        assert {c[:4] for c in got} == expected_combinations(g, p.n), (name, g)
        assert {c[4] for c in got} == set(fr.P_EDGES)
        if g in (3, 2 * p.n - 3):   # the three-term sum 3 q - 3, plain and through a negation
            assert {("q-1", "q-1", "q-1", False), ("q-1", "q-1", "1", True)} <= {c[:4] for c in got}
        assert any(c[2] == "0" and c[3] for c in got)                                          # the negation of 0
        out = ra.pass_twin(p, work, in2, g)
        want = ra.pass_reference(p.moduli, work, in2, g)
        assert out.shape == want.shape == (2, 2, p.n_limbs - 1, p.n)
        assert np.array_equal(out, want), (name, g, np.argwhere(out != want)[:4])


def test_the_negation_of_zero_stays_zero_and_extreme_words_wrap():
    p = fr.pinned(8, 3)
    q = np.array(p.moduli, np.uint64)
    work, in2, _ = ra.pass_inputs(p, 1, 3, 3, planted=False)
    work[:] = 0
    in2[:] = 0
    assert not ra.pass_twin(p, work, in2, 2 * p.n - 1).any()
    in2[0] = (q[:-1] - np.uint64(1))[None, :, None]          # c0 = c1 = q - 1 everywhere; under 2N - 1 every coefficient but 0 gathers -(q - 1) = 1
    out = ra.pass_twin(p, work, in2, 2 * p.n - 1)
    assert np.array_equal(out, ra.pass_reference(p.moduli, work, in2, 2 * p.n - 1))
    assert not out[0, 0, :, 1:].any() and np.array_equal(out[0, 0, :, 0], q[:-1] - np.uint64(2)) and np.array_equal(out[0, 1], in2[0, 1])


def test_pass_twin_rejects_bad_arguments():
    lib = _cabi.load()
    p = fr.pinned(8, 3)
    m = (C.c_uint64 * 3)(*p.moduli)
    work, in2, _ = ra.pass_inputs(p, 1, 1, 3, planted=False)
    out = np.zeros_like(in2)
    f = lib.dpfhe_rotate_add_pass_host
    a = (out.ctypes.data, work.ctypes.data, in2.ctypes.data)
    assert f(m, 3, 8, *a, 3, 1) == 0
    assert f(None, 3, 8, *a, 3, 1) == 2000 and f(m, 3, 8, None, a[1], a[2], 3, 1) == 2000
    assert f(m, 3, 7, *a, 3, 1) == 2000
    assert f(m, 1, 8, *a, 3, 1) == 2002                                                   # no special prime
    assert f(m, 3, 8, *a, 4, 1) == 2000 and f(m, 3, 8, *a, 2 * p.n + 1, 1) == 2000        # even, >= 2N
    assert f(m, 3, 8, in2.ctypes.data, a[1], a[2], 3, 1) == 2000                          # out overlaps the input
    assert f(m, 3, 8, work.ctypes.data, a[1], a[2], 3, 1) == 2000                         # out overlaps the sums
    bad = work.copy()
    bad[0, 1, 2, 5] = p.moduli[2]
    assert f(m, 3, 8, out.ctypes.data, bad.ctypes.data, in2.ctypes.data, 3, 1) == 2000    # non-canonical words
    bad = in2.copy()
    bad[0, 0, 1, 7] = p.moduli[1]
    assert f(m, 3, 8, out.ctypes.data, work.ctypes.data, bad.ctypes.data, 3, 1) == 2000 and b"canonical" in lib.dpfhe_last_error()
    same = (C.c_uint64 * 3)(p.moduli[0], p.moduli[1], p.moduli[0])                        # P is not invertible modulo a data limb
    assert f(same, 3, 8, *a, 3, 1) == 2000 and b"coprime" in lib.dpfhe_last_error()
    # the device entry refuses a null context before anything else
    assert lib.dpfhe_rotate_add_hybrid(None, None, None, None, None, None, None, 1, 1, None) == 2000
