"""CPU: the host twin of the fused relinearise + linear combination + rescale (include/dpfhe.h dpfhe_relinearize_lincomb_rescale_pass_host; csrc/fused_rescale.h
(c)) against Python integers (tests/relin_lincomb_ref.py: every value goes through the CRT integer of its coefficient).

Ring N = 256; the pinned 60-bit primes at Ld = 2 (one output limb) and Ld = 4 (FoldArith's folds), the widest generic primes and a mixed-class context (the
128-bit Barrett path); K in {0, 1, 4, 5, 15} - none, below, on and past the four-in-flight loop, the most -; batches 1 and 3; terms at Ld and Ld + 2 limbs mixed
in one call, the limbs that are not read filled with a word that is no residue.  Planted on item 0: the 6 x 6 edges of P on the special limb of the sums and of
the last data prime under s_last, reached by solving a term's word there.  The device kernel shares the per-word function and is held to the oracle by
tests/test_gpu_relin_lincomb.py."""
import ctypes as C

import numpy as np
import pytest

import class_edges
import fused_rescale_ref as fr
import relin_lincomb_ref as rl
from deeppowers_amd import _cabi

CONTEXTS = {
    "pinned_ld2": lambda ln: fr.pinned(ln, 3),
    "pinned_ld4": lambda ln: fr.pinned(ln, 5),
    "shoup": lambda ln: class_edges.edge_moduli("shoup", ln),               # four generic primes, 60 / 60 / 60 / 51 bits
    "f64_under_fold": lambda ln: class_edges.edge_moduli("f64_under_fold", ln),   # narrow data limbs under a fold special prime
}


@pytest.mark.parametrize("batch", (1, 3))
@pytest.mark.parametrize("K", rl.K_CASES)
@pytest.mark.parametrize("name", sorted(CONTEXTS))
def test_pass_twin_equals_the_integers(name, K, batch):
    p = CONTEXTS[name](8)
    Ld = p.n_limbs - 1
    work, in3, terms, w, plan = rl.pass_inputs(p, K, batch, 1000 * K + batch)
    assert [t.shape[2] for t in terms] == rl.term_limbs(K, Ld) and (K < 2 or {t.shape[2] for t in terms} == {Ld, Ld + 2})
    assert all((t[:, :, Ld:] == rl.NOT_A_RESIDUE).all() for t in terms)
    # the planted coefficients do land where they were aimed (a check of the test's own construction)
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


@pytest.mark.parametrize("name", ("pinned_ld2", "pinned_ld4", "shoup"))
def test_fullest_lazy_sum(name):
    """K = 15, the product's word, every term's word and every weight (the constant too) q - 1: 16 products of (q - 1)^2 and q - 1 on a 60-bit prime, the
    largest sum the 128 bits take"""
    p = CONTEXTS[name](8)
    work, in3, terms, w, _ = rl.pass_inputs(p, 15, 1, 0, full=True)
    q = np.array(p.moduli[:-1], np.uint64)
    assert np.array_equal(rl.relinearized(p.moduli, work, in3)[0, 0], np.broadcast_to((q - np.uint64(1))[:, None], (len(q), p.n)))
    assert all(np.array_equal(z[0, 1, :len(q), 7], q - np.uint64(1)) for z in terms) and (w == q - np.uint64(1)).all() and w.shape == (17, len(q))
    assert max(p.moduli[:-1]).bit_length() == 60 and 16 * (max(p.moduli) - 1) ** 2 + max(p.moduli) - 1 < 1 << 125
    assert np.array_equal(rl.pass_twin(p, work, in3, terms, w), rl.pass_reference(p.moduli, work, in3, terms, w))


def test_constant_goes_to_coefficient_0_of_component_0_only():
    p = fr.pinned(8, 3)
    work, in3, terms, w, _ = rl.pass_inputs(p, 2, 2, 3, planted=False)
    base = w.copy()
    base[-1] = 0
    a, b = rl.pass_twin(p, work, in3, terms, w), rl.pass_twin(p, work, in3, terms, base)
    diff = np.argwhere(a != b)
    assert len(diff) and all(c == 0 and k == 0 for _, c, _, k in diff)


@pytest.mark.parametrize("name", sorted(CONTEXTS))
def test_no_terms_weight_one_is_the_relinearised_rescale(name):
    """the first identity of the header: K = 0, w[0] = 1 and a zero constant row give dpfhe_relinearize_rescale_pass_host's words"""
    p = CONTEXTS[name](8)
    work, in3, plan = fr.pass_a_inputs(p, 2, 21)
    w = np.zeros((2, p.n_limbs - 1), np.uint64)
    w[0] = 1
    assert plan and np.array_equal(rl.pass_twin(p, work, in3, [], w), fr.relin_rescale_pass_twin(p, work, in3))


@pytest.mark.parametrize("K", (1, 5, 15))
@pytest.mark.parametrize("name", sorted(CONTEXTS))
def test_equals_relinearise_then_lincomb_rescale(name, K):
    """the second identity: the relinearised words t, then dpfhe_lincomb_rescale_host on the data context over [t, z_0, ...], each z_k cut to its first Ld limbs"""
    p = CONTEXTS[name](8)
    Ld = p.n_limbs - 1
    work, in3, terms, w, _ = rl.pass_inputs(p, K, 2, 50 + K)
    t = rl.relinearized(p.moduli, work, in3)
    x = np.stack([t] + [z[:, :, :Ld] for z in terms])
    assert np.array_equal(rl.pass_twin(p, work, in3, terms, w), fr.lincomb_rescale_twin(rl.data_params(p), x, w))


def test_pass_twin_rejects_bad_arguments():
    lib = _cabi.load()
    p = fr.pinned(8, 4)
    Ld, n = 3, p.n
    work, in3, terms, w, _ = rl.pass_inputs(p, 2, 1, 1, planted=False)
    assert [t.shape[2] for t in terms] == [Ld, Ld + 2]
    out = np.zeros((1, 2, Ld - 1, n), np.uint64)
    rc = lambda **kw: rl.pass_twin_rc(p, **{**dict(out=out, work=work, in3=in3, terms=terms, w=w), **kw})
    assert rc() == 0
    assert rc(batch=0) == 0
    assert rc(out=work) == 2000 and rc(out=in3) == 2000 and rc(out=terms[1]) == 2000                      # out overlaps an input
    wide = np.zeros(4 * Ld + 2 * (Ld - 1) * n, np.uint64)
    assert rc(out=wide[4 * Ld:], w=wide[:4 * Ld].reshape(4, Ld)) == 0 and rc(out=wide[4 * Ld - 1:], w=wide[:4 * Ld].reshape(4, Ld)) == 2000   # ... the weights' last word
    short = [terms[0], np.ascontiguousarray(terms[1][:, :, :Ld - 1])]
    assert rc(terms=short) == 2000 and b"fewer limbs" in lib.dpfhe_last_error()
    for name, at in (("work", (0, 1, 3, 5)), ("work", (0, 0, 0, 0)), ("in3", (0, 1, 2, 7)), ("w", (3, 1)), ("w", (0, 0))):
        bad = dict(work=work, in3=in3, w=w)[name].copy()
        bad[at] = p.moduli[at[-2] if len(at) == 4 else at[-1]]
        assert rc(**{name: bad}) == 2000 and b"canonical" in lib.dpfhe_last_error(), (name, at)
    bad = [terms[0], terms[1].copy()]
    bad[1][0, 1, Ld - 1, 9] = p.moduli[Ld - 1]
    assert rc(terms=bad) == 2000 and b"canonical" in lib.dpfhe_last_error()
    assert (terms[1][:, :, Ld:] >= np.uint64(1 << 60)).all()                                              # ... while the limbs that are not read may hold anything
    other = in3.copy()
    other[:, 2] = rl.NOT_A_RESIDUE                                                                        # component 2 went through the key switch: not read
    assert rc(in3=other) == 0

    f = lib.dpfhe_relinearize_lincomb_rescale_pass_host
    m = (C.c_uint64 * 4)(*p.moduli)
    ptrs, limbs = rl.host_args(terms)
    a = (out.ctypes.data, work.ctypes.data, in3.ctypes.data)
    assert f(m, 4, 8, *a, ptrs, limbs, 2, w.ctypes.data, 1) == 0
    assert f(None, 4, 8, *a, ptrs, limbs, 2, w.ctypes.data, 1) == 2000 and f(m, 4, 8, None, a[1], a[2], ptrs, limbs, 2, w.ctypes.data, 1) == 2000
    assert f(m, 4, 8, *a, None, limbs, 2, w.ctypes.data, 1) == 2000 and f(m, 4, 8, *a, ptrs, None, 2, w.ctypes.data, 1) == 2000
    assert f(m, 4, 8, *a, ptrs, limbs, 2, None, 1) == 2000
    assert f(m, 4, 7, *a, ptrs, limbs, 2, w.ctypes.data, 1) == 2000
    assert f(m, 2, 8, *a, ptrs, limbs, 2, w.ctypes.data, 1) == 2002                                        # Ld < 2: no data limb left to drop
    assert f(m, 4, 8, *a, ptrs, limbs, 16, w.ctypes.data, 1) == 2000 and b"15" in lib.dpfhe_last_error()
    hole = (C.c_void_p * 2)(terms[0].ctypes.data, None)
    assert f(m, 4, 8, *a, hole, limbs, 2, w.ctypes.data, 1) == 2000
    w0 = np.zeros((2, Ld), np.uint64)
    assert f(m, 4, 8, *a, None, None, 0, w0.ctypes.data, 1) == 0                                           # no terms: no arrays
    same = (C.c_uint64 * 4)(p.moduli[0], p.moduli[1], p.moduli[0], p.moduli[3])
    zero = [np.zeros_like(x) for x in (work, in3)]
    assert f(same, 4, 8, out.ctypes.data, zero[0].ctypes.data, zero[1].ctypes.data, None, None, 0, w0.ctypes.data, 1) == 2000 and b"coprime" in lib.dpfhe_last_error()
    # the device entry refuses a null context before anything else
    assert lib.dpfhe_relinearize_lincomb_rescale_hybrid(None, None, None, None, None, None, None, 0, None, 1, None) == 2000
