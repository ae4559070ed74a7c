"""CPU: the host twins of the fused rescales (include/dpfhe.h dpfhe_relinearize_rescale_pass_host, dpfhe_lincomb_rescale_host; csrc/fused_rescale.h) against
Python integers (tests/fused_rescale_ref.py: every value goes through the CRT integer of its coefficient).

Rings N = 256 (less than one 512-word chunk) and N = 1024; the pinned 60-bit primes at Ld = 2 (one output limb) and Ld = 4 (FoldArith's folds), the widest
generic primes and a mixed-class context (the 128-bit Barrett path).  The device kernels are held to the same words by tests/test_gpu_fused_rescale.py."""
import ctypes as C

import numpy as np
import pytest

import class_edges
import fused_rescale_ref as fr
from deeppowers_amd import _cabi

CONTEXTS = {
    "pinned_ld2": lambda ln: fr.pinned(ln, 3),
    "pinned_ld4": lambda ln: fr.pinned(ln, 5),
    "shoup": lambda ln: class_edges.edge_moduli("shoup", ln),               # four generic primes, 60 / 60 / 60 / 51 bits
    "f64_under_fold": lambda ln: class_edges.edge_moduli("f64_under_fold", ln),   # narrow data limbs under a fold special prime
}


@pytest.mark.parametrize("log2n", (8, 10))
@pytest.mark.parametrize("name", sorted(CONTEXTS))
def test_relin_rescale_pass_twin_equals_the_integers(name, log2n):
    p = CONTEXTS[name](log2n)
    work, in3, plan = fr.pass_a_inputs(p, 2, 11 + log2n)
    # the planted coefficients do land where they were aimed (a check of the test's own construction)
    for comp in range(2):
        t_last = fr.t_last_of(p, work, in3, 0, comp)
        assert [int(t_last[j]) for j, _, _ in plan] == [tgt for _, _, tgt in plan]
        assert [int(work[0, comp, -1, j]) for j, _, _ in plan] == [wp for _, wp, _ in plan]
    assert len({(wp, tgt) for _, wp, tgt in plan}) == 36
    got = fr.relin_rescale_pass_twin(p, work, in3)
    want = fr.relin_rescale_pass_reference(p.moduli, work, in3)
    assert got.shape == want.shape == (2, 2, p.n_limbs - 2, p.n)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


def test_relin_rescale_pass_twin_ignores_component_2_and_takes_extreme_words():
    p = fr.pinned(8, 5)
    work, in3, _ = fr.pass_a_inputs(p, 1, 5, planted=False)
    q = np.array(p.moduli, np.uint64)
    work[0, 0] = (q - np.uint64(1))[:, None]
    in3[0, 0] = (q[:-1] - np.uint64(1))[:, None]
    work[0, 1] = 0
    in3[0, 1] = 0
    want = fr.relin_rescale_pass_reference(p.moduli, work, in3)
    assert not want[0, 1].any()                       # 0 / P + 0, rescaled, is 0
    assert np.array_equal(fr.relin_rescale_pass_twin(p, work, in3), want)
    other = in3.copy()
    other[:, 2] = (q[:-1] - np.uint64(1))[:, None]
    assert np.array_equal(fr.relin_rescale_pass_twin(p, work, other), want)


@pytest.mark.parametrize("log2n", (8, 10))
@pytest.mark.parametrize("name", sorted(CONTEXTS))
@pytest.mark.parametrize("K", (1, 2, 15, 16))
def test_lincomb_rescale_twin_equals_the_integers(K, name, log2n):
    p = CONTEXTS[name](log2n)
    batch = 2 if K <= 2 else 1
    x, w = fr.lincomb_inputs(p, K, batch, 100 * K + log2n)
    got = fr.lincomb_rescale_twin(p, x, w)
    want = fr.lincomb_rescale_reference(p.moduli, x, w)
    assert got.shape == want.shape == (batch, 2, p.n_limbs - 1, p.n)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


@pytest.mark.parametrize("name", ("pinned_ld2", "pinned_ld4", "shoup"))
def test_lincomb_rescale_twin_fullest_lazy_sum(name):
    """K = 16, every operand word and every weight (the constant too) q - 1: 17 terms of (q - 1)^2 on a 60-bit prime, the largest sum the 128 bits take"""
    p = CONTEXTS[name](8)
    x, w = fr.lincomb_inputs(p, 16, 1, 0, full=True)
    assert max(p.moduli).bit_length() == 60 and 16 * (max(p.moduli) - 1) ** 2 + max(p.moduli) - 1 < 1 << 125
    assert np.array_equal(fr.lincomb_rescale_twin(p, x, w), fr.lincomb_rescale_reference(p.moduli, x, w))


def test_lincomb_constant_goes_to_coefficient_0_of_component_0_only():
    p = fr.pinned(8, 3)
    x, w = fr.lincomb_inputs(p, 2, 2, 3)
    base = w.copy()
    base[-1] = 0
    a, b = fr.lincomb_rescale_twin(p, x, w), fr.lincomb_rescale_twin(p, x, base)
    diff = np.argwhere(a != b)
    assert len(diff) and all(c == 0 and k == 0 for _, c, _, k in diff)


def test_host_twins_reject_bad_arguments():
    lib = _cabi.load()
    p = fr.pinned(8, 3)
    m = (C.c_uint64 * 3)(*p.moduli)
    work, in3, _ = fr.pass_a_inputs(p, 1, 1, planted=False)
    out = np.zeros((1, 2, 1, p.n), np.uint64)
    a = (out.ctypes.data, work.ctypes.data, in3.ctypes.data)
    assert lib.dpfhe_relinearize_rescale_pass_host(m, 2, 8, *a, 1) == 2002             # Ld < 2: no data limb left to drop
    assert lib.dpfhe_relinearize_rescale_pass_host(None, 3, 8, *a, 1) == 2000
    assert lib.dpfhe_relinearize_rescale_pass_host(m, 3, 7, *a, 1) == 2000
    assert lib.dpfhe_relinearize_rescale_pass_host(m, 3, 8, work.ctypes.data, work.ctypes.data, in3.ctypes.data, 1) == 2000   # out overlaps the sums
    bad = work.copy()
    bad[0, 1, 2, 5] = p.moduli[2]
    assert lib.dpfhe_relinearize_rescale_pass_host(m, 3, 8, out.ctypes.data, bad.ctypes.data, in3.ctypes.data, 1) == 2000
    same = (C.c_uint64 * 3)(p.moduli[0], p.moduli[0], p.moduli[2])
    assert lib.dpfhe_relinearize_rescale_pass_host(same, 3, 8, *a, 1) == 2000 and b"coprime" in lib.dpfhe_last_error()

    x, w = fr.lincomb_inputs(p, 2, 1, 2)
    o = np.zeros((1, 2, 2, p.n), np.uint64)
    b = (o.ctypes.data, x.ctypes.data, w.ctypes.data)
    assert lib.dpfhe_lincomb_rescale_host(m, 3, 8, *b, 2, 1) == 0
    assert lib.dpfhe_lincomb_rescale_host(m, 1, 8, *b, 2, 1) == 2002                     # no limb left to drop
    assert lib.dpfhe_lincomb_rescale_host(m, 3, 8, *b, 0, 1) == 2000 and lib.dpfhe_lincomb_rescale_host(m, 3, 8, *b, 17, 1) == 2000
    assert lib.dpfhe_lincomb_rescale_host(m, 3, 8, *b, 2, 0) == 2000
    assert lib.dpfhe_lincomb_rescale_host(m, 3, 8, x.ctypes.data, x.ctypes.data, w.ctypes.data, 2, 1) == 2000
    wb = w.copy()
    wb[2, 1] = p.moduli[1]
    assert lib.dpfhe_lincomb_rescale_host(m, 3, 8, o.ctypes.data, x.ctypes.data, wb.ctypes.data, 2, 1) == 2000
    # the device entries refuse a null context before anything else
    assert lib.dpfhe_relinearize_rescale_hybrid(None, None, None, None, None, 1, None) == 2000
    assert lib.dpfhe_lincomb_rescale(None, None, None, None, 1, 1, None) == 2000
