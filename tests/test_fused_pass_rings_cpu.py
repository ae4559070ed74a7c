"""CPU: the four host twins of the fused last passes (include/dpfhe.h dpfhe_relinearize_rescale_pass_host, dpfhe_lincomb_rescale_host, dpfhe_rotate_add_pass_host,
dpfhe_relinearize_lincomb_rescale_pass_host) against the Python integers of tests/fused_rescale_ref.py, rotate_add_ref.py and relin_lincomb_ref.py on the kinds of
context their own CPU tests leave out (those run the pinned fold primes, four generic primes and f64 limbs under a fold special prime):

  mixed           class_edges.edge_moduli("mixed", 8): eight limbs, one of every class and of every width from 13 to 60 bits; Ld = 7, a 48-bit special prime under
                  60-bit data limbs, a 60-bit generic last data prime next to it, the smallest prime (7681) in the middle
  mixed_reversed  the same primes in reverse order: the 60-bit fold prime is the special prime, the 48-bit prime the first data limb, the 50-bit prime the last
  smallest        the three smallest primes = 1 mod 512 (13 and 14 bits): P and q_last far below 2^32

Planted with the helpers of the existing CPU tests (fr.pass_a_inputs, ra.pass_inputs, rl.pass_inputs).  Every planted combination is reachable on every one of
these contexts, the 13-bit limbs included: the six edges of P and of the last data prime are distinct as soon as both exceed 6, the words 0, 1 and q - 1 as soon
as q > 2, and the solved words (c_last, a term's word, the weights' inverses) exist modulo any prime.  So the full sets are asserted: 6 x 6, and for the
rotate-and-add pass what the element offers (test_rotate_add_cpu.expected_combinations: all 54 for 3 and 2N - 3) over all six edges of P.
tests/test_gpu_fused_pass_rings.py runs the device kernels on the mixed context at N = 4096 and 8192."""
import numpy as np
import pytest

import class_edges
import fused_rescale_ref as fr
import relin_lincomb_ref as rl
import rotate_add_ref as ra
import test_gpu_fused_pass_rings as rings
import test_rotate_add_cpu as rac
from deeppowers_amd.params import FheParams


def reversed_limbs(p):
    return FheParams(p.log2_n, tuple(reversed(p.moduli)), tuple(reversed(p.psi)))


CONTEXTS = {
    "mixed": lambda ln: class_edges.edge_moduli("mixed", ln),
    "mixed_reversed": lambda ln: reversed_limbs(class_edges.edge_moduli("mixed", ln)),
    "smallest": lambda ln: class_edges.edge_moduli("smallest", ln),
}
NAMES = sorted(CONTEXTS)


def test_the_contexts_are_the_ones_described():
    widths = [60, 47, 59, 13, 51, 50, 60, 48]
    assert [q.bit_length() for q in CONTEXTS["mixed"](8).moduli] == widths
    assert [q.bit_length() for q in CONTEXTS["mixed_reversed"](8).moduli] == widths[::-1]
    assert {class_edges.expected_class(q) for q in CONTEXTS["mixed"](8).moduli} == set(class_edges.CLASSES)
    assert class_edges.expected_class(CONTEXTS["mixed_reversed"](8).moduli[-1]) == "fold"
    assert CONTEXTS["smallest"](8).moduli == (7681, 10753, 11777)
    # the rings tests/test_gpu_fused_pass_rings.py runs the mixed context at: the same widths but for the smallest prime (16 and 17 bits)
    for ln, small in ((12, 16), (13, 17)):
        assert [q.bit_length() for q in CONTEXTS["mixed"](ln).moduli] == widths[:3] + [small] + widths[4:]


@pytest.mark.parametrize("log2n", (15, 16))
def test_the_gpu_modules_generic_primes_are_the_shoup_edge_contexts(log2n):
    """tests/test_gpu_fused_pass_rings.py builds its generic contexts at N = 32768 and 65536 from the catalogue's primes without the catalogue's roots"""
    assert rings.generic_primes(log2n) == class_edges.edge_moduli("shoup", log2n)
    assert rings.generic_primes(log2n, 2) == class_edges.edge_moduli("shoup60", log2n)
    assert {class_edges.expected_class(q) for q in rings.generic_primes(log2n).moduli} == {"shoup"}


@pytest.mark.parametrize("name", NAMES)
def test_relin_rescale_pass_twin_equals_the_integers(name):
    p = CONTEXTS[name](8)
    work, in3, plan = fr.pass_a_inputs(p, 2, 19)
    for comp in range(2):
        t_last = fr.t_last_of(p, work, in3, 0, comp)
        assert [int(t_last[j]) for j, _, _ in plan] == [tgt for _, _, tgt in plan]
        assert [int(work[0, comp, -1, j]) for j, _, _ in plan] == [wp for _, wp, _ in plan]
    assert len({(wp, tgt) for _, wp, tgt in plan}) == 36
    got = fr.relin_rescale_pass_twin(p, work, in3)
    want = fr.relin_rescale_pass_reference(p.moduli, work, in3)
    assert got.shape == want.shape == (2, 2, p.n_limbs - 2, p.n)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


@pytest.mark.parametrize("name", NAMES)
def test_lincomb_rescale_twin_equals_the_integers(name):
    """K = 1, 2, 15 and 16 and three items of K = 3; and the fullest lazy sum - 17 terms of (q - 1)^2 - on whatever widths the context has"""
    p = CONTEXTS[name](8)
    for K, batch, full in [(K, 2 if K <= 2 else 1, False) for K in (1, 2, 15, 16)] + [(3, 3, False), (16, 1, True)]:
        x, w = fr.lincomb_inputs(p, K, batch, 100 * K + 8, full=full)
        got = fr.lincomb_rescale_twin(p, x, w)
        want = fr.lincomb_rescale_reference(p.moduli, x, w)
        assert got.shape == want.shape == (batch, 2, p.n_limbs - 1, p.n)
        assert np.array_equal(got, want), (K, batch, full, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("name", NAMES)
def test_rotate_add_pass_twin_equals_the_integers(name):
    p = CONTEXTS[name](8)
    for i, g in enumerate(ra.elements(p.n)):
        work, in2, plan = ra.pass_inputs(p, 2, 257 + i, g)
        got = ra.reached(p, work, in2, g, plan)
        assert {c[:4] for c in got} == rac.expected_combinations(g, p.n), (name, g)
        assert {c[4] for c in got} == set(fr.P_EDGES)
        out = ra.pass_twin(p, work, in2, g)
        want = ra.pass_reference(p.moduli, work, in2, g)
        assert out.shape == want.shape == (2, 2, p.n_limbs - 1, p.n)
        assert np.array_equal(out, want), (name, g, np.argwhere(out != want)[:4])


@pytest.mark.parametrize("K", (0, 1, 5, 15))
@pytest.mark.parametrize("name", NAMES)
def test_relin_lincomb_pass_twin_equals_the_integers(name, K):
    p = CONTEXTS[name](8)
    Ld, batch = p.n_limbs - 1, 2
    work, in3, terms, w, plan = rl.pass_inputs(p, K, batch, 1000 * K + batch)
    assert [t.shape[2] for t in terms] == rl.term_limbs(K, Ld) and all((t[:, :, Ld:] == rl.NOT_A_RESIDUE).all() for t in terms)
    t = rl.relinearized(p.moduli, work[:1], in3[:1])
    for comp in range(2):
        s_last = rl.sums(p.moduli[:-1], t, [z[:1] for z in terms], w, 0, comp)[-1]
        assert [int(s_last[j]) for j, _, _ in plan] == [tgt for _, _, tgt in plan]
        assert [int(work[0, comp, -1, j]) for j, _, _ in plan] == [wp for _, wp, _ in plan]
    assert len({(wp, tgt) for _, wp, tgt in plan}) == 36
    got = rl.pass_twin(p, work, in3, terms, w)
    want = rl.pass_reference(p.moduli, work, in3, terms, w)
    assert got.shape == want.shape == (batch, 2, p.n_limbs - 2, p.n)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
