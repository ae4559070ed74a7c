"""-m gpu: every modular product held to the oracle at the edges of its REMAINDER range, through the C ABI, whole buffers word for word against oracle.c
(threads=0).

The inputs come from tests/remainder_edges.py: operands solved so that the products the kernels take, and the sums they add them into, have their
remainder in T(q) = {0, 1, 2, q - 2, q - 1, h - 1, h, h + 1, h + 2} - where a conditional subtract after a floor quotient, the sign fix after a nearest
quotient and the rounding tie decide.  tests/test_remainder_edges_cpu.py shows against Python integers that the inputs do what they claim, and with the
emulator that they reach every product / reduce primitive of modarith.h with all nine targets.

Contexts: the class_edges.edge_moduli kinds fold, f64, fold_scaled, f64_wide, shoup and mixed, plus FheParams.n4096_l4() (the benchmark's primes), at
the smallest rings at which each kernel family exists: log2 N = 8 (the smallest geometry), 12 (the fused quad, the bit-29 lazy multiply,
relin_shared_kernel) and 13 (the dual form, the halves transforms, the LDS key tiles).  Larger rings - the split transforms from log2 N = 15 and the
quarters form at 14 - are out of scope here: their stage structure differs from the builders' radix-2 model.

A case that could not target its words must not pass quietly: every case asserts its builder's n_untargeted - exactly 0 for the dyadic, tensor,
transform and rescale builders, at most 1 % of the key's words for key material (the digits' transforms can hold zeros)."""
import numpy as np
import pytest

import remainder_edges as re_
from class_edges import CLASSES, Rig, edge_moduli
from deeppowers_amd.params import FheParams
from oracle.cbind import Oracle

pytestmark = pytest.mark.gpu

KINDS = CLASSES + ("mixed",)
CONTEXTS = [(k, ln) for ln in (8, 12, 13) for k in KINDS] + [("bench", 12)]
KEY_CONTEXTS = [(k, ln) for k, ln in CONTEXTS if ln >= 12]
ids = lambda cases: [f"{k}_n{1 << ln}" for k, ln in cases]
HALVES_MIN_POLYS = 2304          # launch.h kHalvesMinPolys


@pytest.fixture
def rig():
    made = []

    def make(kind, log2n):
        r = Rig(FheParams.n4096_l4()) if kind == "bench" else Rig(kind, log2n)
        made.append(r)
        return r
    yield make
    for r in made:
        r.close()


def host(t):
    from deeppowers_amd.evaluator import to_host
    return to_host(t)


# ---- transforms ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,log2n", CONTEXTS, ids=ids(CONTEXTS))
def test_transforms_at_the_remainder_edges(rig, kind, log2n):
    """one item per stage and direction (every butterfly of that stage with its product and its sum leg in T), out of place and in place; at N = 8192 the
    same items tiled past kHalvesMinPolys, where the halves form takes over"""
    r = rig(kind, log2n)
    (f, miss_f), (i, miss_i) = re_.forward_stage_inputs(r.orc, 3), re_.inverse_stage_inputs(r.orc, 4)
    assert miss_f == 0 and miss_i == 0
    want_f, want_i = r.orc.ntt_fwd(f, threads=0), r.orc.ntt_inv(i, threads=0)
    reps = [1] + ([-(-HALVES_MIN_POLYS // (log2n * r.L)) + 1] if log2n == 13 else [])
    for rep in reps:
        assert rep == 1 or rep * log2n * r.L > HALVES_MIN_POLYS
        tile = lambda v: np.tile(v, (rep, 1, 1))
        df, di = r.dev(tile(f)), r.dev(tile(i))
        assert np.array_equal(host(r.ev.ntt_forward(df)), tile(want_f)), rep
        assert np.array_equal(host(r.ev.ntt_inverse(di)), tile(want_i)), rep
        r.ev.ntt_forward_(df)
        assert np.array_equal(host(df), tile(want_f)), rep
        r.ev.ntt_inverse_(di)
        assert np.array_equal(host(di), tile(want_i)), rep


# ---- the fused / composed multiply -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,log2n", CONTEXTS, ids=ids(CONTEXTS))
def test_multiply_at_the_remainder_edges(rig, kind, log2n):
    """the tensor inputs (three of the four products and the middle sum in T) from both input domains into both output domains, and a squaring with
    A0^2 in T; where the context has fold_scaled limbs also the inputs that put s a b on the edges, which is what their lazy products hold; on fold
    contexts at N = 4096 / 8192 every form of the fused multiply"""
    from deeppowers_amd.evaluator import Ciphertext
    r = rig(kind, log2n)
    L, n, orc = r.L, r.n, r.orc
    factors = re_.fold_scaled_factors(r.p.moduli)
    pairs = []
    for fac in [None] + ([factors] if any(v != 1 for v in factors) else []):
        ((a, b), (A, B)), miss = re_.tensor_inputs(orc, 2, 5, fac)
        assert miss == 0
        pairs.append((a, b, A, B))
    (sq, SQ), miss = re_.squaring_inputs(orc, 2, 6)
    assert miss == 0
    pairs.append((sq, sq, SQ, SQ))
    ntt = lambda v: orc.ntt_fwd(v.reshape(-1, L, n), threads=0).reshape(v.shape)
    forms = ["quad", "dual"] if r.ctx.uses_fold and log2n in (12, 13) else [None]
    try:
        for form in forms:
            if form:
                r.ctx.set_ct_mul_variant(form)
            for which, (a, b, A, B) in enumerate(pairs):
                want = orc.ct_mul(a, b, threads=0)
                want_ntt = ntt(want)
                ca, cA = Ciphertext(r.dev(a)), Ciphertext(r.dev(A), is_ntt=True)
                cb, cB = (ca, cA) if a is b else (Ciphertext(r.dev(b)), Ciphertext(r.dev(B), is_ntt=True))
                assert np.array_equal(host(r.ev.multiply(ca, cb).data), want), (form, which)
                assert np.array_equal(host(r.ev.multiply(ca, cb, out_ntt=True).data), want_ntt), (form, which)
                assert np.array_equal(host(r.ev.multiply(cA, cB, out_ntt=False).data), want), (form, which)
                assert np.array_equal(host(r.ev.multiply(cA, cB).data), want_ntt), (form, which)
    finally:
        if forms[0]:
            r.ctx.set_ct_mul_variant("quad" if log2n == 12 else "dual")


# ---- streaming operations --------------------------------------------------------------------------------------------------------------------------------------
def scale_round_integers(p, drop):
    """words [1][L][N] of the integers 0, +-Qd, floor(Qd / 2), floor(Qd / 2) + 1, -floor(Qd / 2) - 1 (Qd the product of the dropped limbs) along the
    coefficient index, and round(X / Qd) for each: 0, 1, -1, 0, 1, -1 (Qd is odd: floor(Qd / 2) / Qd is just below 1 / 2)"""
    Qd = int(np.prod([p.moduli[i] for i in drop], dtype=object))
    vals = [0, Qd, -Qd, Qd // 2, Qd // 2 + 1, -(Qd // 2) - 1]
    x = np.array([[vals[k % 6] % q for k in range(p.n)] for q in p.moduli], np.uint64)[None]
    return np.ascontiguousarray(x), [0, 1, -1, 0, 1, -1]


@pytest.mark.parametrize("kind,log2n", CONTEXTS, ids=ids(CONTEXTS))
def test_streaming_operations_at_the_remainder_edges(rig, kind, log2n):
    """dyadic_mul, dyadic_mul_add_ (product and sum in T), multiply_plain, matvec_scalar / matvec_plain with 5 rows on both sides of kDot30Period = 8
    (and, at the smallest ring, of the generic 128-column fold), matvec_plain_multi with three right-hand sides at (8 x 16) and (5 x 9), rescale_words
    with the quotient product in T on both sides of the rounding's wrap, scale_round on the integers at its rounding boundaries"""
    from deeppowers_amd.evaluator import Ciphertext, Plaintext
    r = rig(kind, log2n)
    L, n, orc = r.L, r.n, r.orc
    (a, b, acc), miss = re_.dyadic_inputs(orc, (3,), 2)
    assert miss == 0
    assert np.array_equal(host(r.ev.dyadic_mul(r.dev(a), r.dev(b))), orc.dyadic("mul", a, b, threads=0))
    dacc = r.dev(acc)
    r.ev.dyadic_mul_add_(dacc, r.dev(a), r.dev(b))
    assert np.array_equal(host(dacc), orc.dyadic("mul_add", a, b, acc=acc, threads=0))
    (ct, pt), miss = re_.plain_product_inputs(orc, 2, 3)
    assert miss == 0
    got = r.ev.multiply_plain(Ciphertext(r.dev(ct), True), Plaintext(r.dev(pt), True))
    assert np.array_equal(host(got.data), orc.dyadic("mul", ct, np.ascontiguousarray(np.broadcast_to(pt, ct.shape)), threads=0))
    rows = 5
    for cols in (1, 8, 9) + ((129,) if log2n == 8 else ()):
        (W, x), miss = re_.matvec_plain_inputs(orc, rows, cols, 2, 10 + cols)
        assert miss == 0
        got = r.ev.matvec_plain(Plaintext(r.dev(W), True), Ciphertext(r.dev(x), True))
        assert np.array_equal(host(got.data), orc.matvec_plain(W.ravel(), x.ravel(), rows, cols, threads=0)), ("plain", cols)
        (w, x), miss = re_.matvec_scalar_inputs(orc, rows, cols, 2, 20 + cols)
        assert miss == 0
        got = r.ev.matvec_scalar(r.dev(w), Ciphertext(r.dev(x), True))
        assert np.array_equal(host(got.data), orc.matvec_scalar(w, x, rows, cols, threads=0)), ("scalar", cols)
    n_rhs = 3
    for rows, cols in ((8, 16), (5, 9)):
        (W, x), miss = re_.matvec_plain_inputs(orc, rows, cols, 2 * n_rhs, 30 + cols)
        assert miss == 0
        x = np.ascontiguousarray(x.reshape(cols, n_rhs, 2, L, n))
        got = host(r.ev.matvec_plain_multi(Plaintext(r.dev(W), True), r.dev(x), n_rhs))
        for t in range(n_rhs):
            want = orc.matvec_plain(W.ravel(), np.ascontiguousarray(x[:, t]).ravel(), rows, cols, threads=0)
            assert np.array_equal(got[:, t], want), ("multi", rows, cols, t)
    z, miss = re_.rescale_inputs(orc, (3, 2), 5)
    assert miss == 0
    assert np.array_equal(host(r.ev.rescale_words(r.dev(z))), orc.rescale(z))
    for drop0, ndrop, keep0, nkeep in ((L - 1, 1, 0, L - 1), (0, 2, 2, L - 2)):
        x, rounded = scale_round_integers(r.p, range(drop0, drop0 + ndrop))
        want = orc.scale_round(x, drop0, ndrop, keep0, nkeep, 1)
        for j in range(nkeep):
            q = r.p.moduli[keep0 + j]
            assert [int(v) for v in want[0, j, :6]] == [v % q for v in rounded]
        assert np.array_equal(host(r.ev.scale_round(r.dev(x), drop0, ndrop, keep0, nkeep, 1)), want), (drop0, ndrop)


# ---- key switching ---------------------------------------------------------------------------------------------------------------------------------------------
def under_cap(miss, key):
    assert miss * 100 <= key.size, (miss, key.size)


@pytest.mark.parametrize("kind,log2n", KEY_CONTEXTS, ids=ids(KEY_CONTEXTS))
def test_key_switching_at_the_remainder_edges(rig, kind, log2n):
    """relinearize, switch_key, keyswitch_hybrid (2 and 3 components) and rotate_hybrid_hoisted (3, 3^9, 2N - 1) under keys solved against item 0's
    digits: every product NTT(digit) (.) key in T, and the sum over the digits in T"""
    from deeppowers_amd.evaluator import Ciphertext
    r = rig(kind, log2n)
    L, n, orc = r.L, r.n, r.orc
    (c3, evk), miss = re_.relin_inputs(orc, 2, 700)
    under_cap(miss, evk)
    dk = r.dev(evk)
    got = r.ev.relinearize(Ciphertext(r.dev(c3)), dk)
    assert np.array_equal(host(got.data), orc.relinearize(c3, evk, threads=0))
    a = np.ascontiguousarray(c3[:, 1:])
    got = r.ev.apply_galois(Ciphertext(r.dev(a)), 1, dk)            # dpfhe_switch_key on the same digits
    assert np.array_equal(host(got.data), orc.switch_key(a, evk, threads=0))
    data = Oracle(log2n, r.p.moduli[:-1], r.p.psi[:-1])
    (cts, key), miss = re_.hybrid_inputs(orc, data, 2, 710)
    under_cap(miss, key)
    dkey = r.dev(key)
    for comps in (2, 3):
        got = r.ev.keyswitch_hybrid(Ciphertext(r.dev(cts[comps])), dkey)
        assert np.array_equal(host(got.data), orc.keyswitch_hybrid(cts[comps], key, comps, threads=0)), comps
    elts = re_.rotation_elements(n)
    T = 2
    (cts, keys), miss = re_.hoisted_inputs(orc, data, elts, T, 720)
    under_cap(miss, keys)
    got = host(r.ev.rotate_hybrid_hoisted(Ciphertext(r.dev(cts)), list(elts), r.dev(keys)).data).reshape(len(elts), T, 2, L - 1, n)
    for t in range(T):
        assert np.array_equal(got[:, t], orc.rotate_hoisted(cts[t], elts, keys, threads=0)), t
