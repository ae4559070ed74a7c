"""-m gpu: every per-limb arithmetic class at the edge of its prime range (tests/class_edges.py) through the C ABI against oracle.c.

The suite's other class tests take primes far inside each class's range; the lazy arithmetic's margin is smallest at the edge of the rule that admits
a prime.  Here every context is built from catalogue primes nearest a bound - the special prime of key switching and the last limb of a rescale
included - and every comparison is a whole buffer, word for word, against the oracle (threads=0), whose exactness at these primes
tests/test_class_edges_cpu.py shows against direct evaluation.  Inputs carry worst_case stripes in item 0 and q - 1 in every word of item 1, in the
ciphertexts and in the key material.  Each context first asserts the classes its limbs run on, so that a change to the rule cannot move a case to
another class unseen."""
import numpy as np
import pytest

from class_edges import CLASSES, Rig
from oracle.cbind import Oracle

pytestmark = pytest.mark.gpu

@pytest.fixture
def rig(request):
    made = []

    def make(kind, log2n):
        r = Rig(kind, log2n)
        made.append(r)
        return r
    yield make
    for r in made:
        r.close()


def host(t):
    from deeppowers_amd.evaluator import to_host
    return to_host(t)


UNIFORM_AND_MIXED = [(k, ln) for ln in (12, 13) for k in CLASSES + ("mixed",)] + [(k, 14) for k in CLASSES]
IDS = [f"{k}_n{1 << ln}" for k, ln in UNIFORM_AND_MIXED]


# ---- transforms -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,log2n", UNIFORM_AND_MIXED + [(k, 16) for k in CLASSES], ids=IDS + [f"{k}_n65536" for k in CLASSES])
def test_transforms_at_the_class_edges(rig, kind, log2n):
    """ntt_forward / ntt_inverse out of place and in place, both directions on non-image data; at N = 8192 and 16384 also a batch past
    kHalvesMinPolys (2304 residue polynomials) / kQuartersMinPolys (768), where those forms of the transform take over"""
    import torch
    r = rig(kind, log2n)
    thresholds = {13: 2304, 14: 768}
    batches = [3] if log2n > 14 else [5]
    if log2n in thresholds:
        batches.append(-(-thresholds[log2n] // r.L) + 1)
    for batch in batches:
        x = r.words(r.orc, (batch,), 100 + batch)
        want_f, want_i = r.orc.ntt_fwd(x, threads=0), r.orc.ntt_inv(x, threads=0)
        d = r.dev(x)
        X = r.ev.ntt_forward(d)
        assert np.array_equal(host(X), want_f), batch
        assert np.array_equal(host(r.ev.ntt_inverse(d)), want_i), batch
        assert torch.equal(r.ev.ntt_inverse(X), d), batch
        y = d.clone()
        r.ev.ntt_forward_(y)
        assert np.array_equal(host(y), want_f), batch
        y = d.clone()
        r.ev.ntt_inverse_(y)
        assert np.array_equal(host(y), want_i), batch


# ---- the fused / composed multiply ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,log2n", UNIFORM_AND_MIXED + [(k, 16) for k in CLASSES], ids=IDS + [f"{k}_n65536" for k in CLASSES])
def test_multiply_at_the_class_edges(rig, kind, log2n):
    """multiply in both output domains from both input domains, squaring included; on fold contexts at N = 4096 / 8192 every form of the fused
    multiply (quad, dual)"""
    from deeppowers_amd.evaluator import Ciphertext
    r = rig(kind, log2n)
    L, n = r.L, r.n
    batch = 2 if log2n >= 14 else 3
    a = r.words(r.orc, (batch, 2), 200)
    b = r.words(r.orc, (batch, 2), 201)
    b[0] = np.roll(b[0], n // 16, axis=-1)   # b's stripes overlap a's only in part
    want = r.orc.ct_mul(a, b, threads=0)
    want_sq = r.orc.ct_mul(a, a, threads=0)
    ntt = lambda v: r.orc.ntt_fwd(v.reshape(-1, L, n), threads=0).reshape(v.shape)
    want_ntt, want_sq_ntt = ntt(want), ntt(want_sq)
    A, B = Ciphertext(r.dev(a)), Ciphertext(r.dev(b))
    An = Ciphertext(r.ev.ntt_forward(A.data.view(-1, L, n)).view(batch, 2, L, n), is_ntt=True)
    Bn = Ciphertext(r.ev.ntt_forward(B.data.view(-1, L, n)).view(batch, 2, L, n), is_ntt=True)
    forms = [None]
    if r.ctx.uses_fold and log2n in (12, 13):
        forms = ["quad", "dual"]
    try:
        for form in forms:
            if form:
                r.ctx.set_ct_mul_variant(form)
            assert np.array_equal(host(r.ev.multiply(A, B).data), want), form
            assert np.array_equal(host(r.ev.multiply(A, B, out_ntt=True).data), want_ntt), form
            assert np.array_equal(host(r.ev.multiply(An, Bn, out_ntt=False).data), want), form
            assert np.array_equal(host(r.ev.multiply(An, Bn).data), want_ntt), form
            assert np.array_equal(host(r.ev.multiply(A, A).data), want_sq), form
            assert np.array_equal(host(r.ev.multiply(An, An).data), want_sq_ntt), form
    finally:
        if forms[0]:
            r.ctx.set_ct_mul_variant("quad" if log2n == 12 else "dual")


# ---- key switching ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,log2n", UNIFORM_AND_MIXED, ids=IDS)
def test_key_switching_at_the_class_edges(rig, kind, log2n):
    """relinearize, apply_galois (+ switch_key), keyswitch_hybrid with 2 and 3 components, rotate_hybrid_batch / _hoisted / _grouped - on a uniform
    context the class's own key-switching kernels (k_relin_{f64,f64w,fscaled}.hip; fold / generic), on the mixture one launch per class; the last
    limb (the special prime) is an edge prime; worst-case words in the ciphertexts and in the keys"""
    from deeppowers_amd.evaluator import Ciphertext
    r = rig(kind, log2n)
    L, n, orc = r.L, r.n, r.orc
    big = log2n >= 14
    batch = 2 if big else 3
    a = r.words(orc, (batch, 2), 300)
    b = r.words(orc, (batch, 2), 301)
    c3 = orc.ct_mul(a, b, threads=0)
    evk = r.words(orc, (L, 2), 302)
    dk = r.dev(evk)
    got = r.ev.relinearize(Ciphertext(r.dev(c3)), dk)
    assert np.array_equal(host(got.data), orc.relinearize(c3, evk, threads=0))
    for g in (5, 2 * n - 1):
        got = r.ev.apply_galois(Ciphertext(r.dev(a)), g, dk)
        assert np.array_equal(host(got.data), orc.switch_key(orc.apply_galois(a, g), evk, threads=0)), g
    Ld = L - 1
    data = Oracle(log2n, r.p.moduli[:-1], r.p.psi[:-1])
    key = r.words(orc, (Ld, 2), 303)
    dkey = r.dev(key)
    for comps in (2, 3):
        ct = r.words(data, (batch, comps), 310 + comps)
        got = r.ev.keyswitch_hybrid(Ciphertext(r.dev(ct)), dkey)
        assert np.array_equal(host(got.data), orc.keyswitch_hybrid(ct, key, comps, threads=0)), comps
    # rotations: 66 keys cross the 64-rotation launch groups of the hoisted form (a few at N = 16384 and on the 8-limb mixture)
    k = 3 if big else (5 if L > 4 else 66)
    T = 2
    elts = [pow(3, i + 1, 2 * n) for i in range(k)]
    elts[-1] = 2 * n - 1
    keys = orc.fill(k * Ld * 2, 320).reshape(k, Ld, 2, L, n)
    for i in (0, k - 1):
        keys[i] = r.words(orc, (Ld, 2), 321 + i)
    dks = r.dev(keys)
    check = sorted({0, 1, k - 1} | ({63, 64} if k > 64 else set()))
    cts = r.words(data, (T, 2), 330)
    got = host(r.ev.rotate_hybrid_batch(Ciphertext(r.dev(cts[:1])), elts, dks).data)
    for i in check:
        assert np.array_equal(got[i], orc.keyswitch_hybrid(data.apply_galois(cts[:1], elts[i]), keys[i], 2, threads=0)[0]), ("batch", i)
    got = host(r.ev.rotate_hybrid_hoisted(Ciphertext(r.dev(cts)), elts, dks).data).reshape(k, T, 2, Ld, n)
    for i in check:
        for t in range(T):
            assert np.array_equal(got[i, t], orc.rotate_hoisted(cts[t], [elts[i]], keys[i][None], threads=0)[0]), ("hoisted", i, t)
    items = r.words(data, (k * T, 2), 340)
    got = host(r.ev.rotate_hybrid_grouped(Ciphertext(r.dev(items)), elts, T, dks).data)
    for i in sorted({j * T + t for j in check for t in range(T)}):
        assert np.array_equal(got[i], orc.keyswitch_hybrid(data.apply_galois(items[i][None], elts[i // T]), keys[i // T], 2, threads=0)[0]), ("grouped", i)


# ---- streaming operations: dyadic, plaintext products, sums, rescale, base extension -----------------------------------------------------------------------
@pytest.mark.parametrize("kind,log2n", UNIFORM_AND_MIXED, ids=IDS)
def test_streaming_operations_at_the_class_edges(rig, kind, log2n):
    """dyadic_mul, dyadic_mul_add_, multiply_plain, reduce_sum past 512 items (all 15 batch splits, the capped grid), rescale_words with an edge
    prime as the dropped last limb, base_extend / scale_round between edge primes (k_bx_fold on the fold context, k_bx_shoup otherwise)"""
    from deeppowers_amd.evaluator import Ciphertext, Plaintext
    r = rig(kind, log2n)
    L, n, orc = r.L, r.n, r.orc
    x = r.words(orc, (3,), 400)
    y = r.words(orc, (3,), 401)
    acc = r.words(orc, (3,), 402)
    y[0] = y[0][:, ::-1]
    assert np.array_equal(host(r.ev.dyadic_mul(r.dev(x), r.dev(y))), orc.dyadic("mul", x, y))
    dacc = r.dev(acc)
    r.ev.dyadic_mul_add_(dacc, r.dev(x), r.dev(y))
    assert np.array_equal(host(dacc), orc.dyadic("mul_add", x, y, acc=acc))
    ct = r.words(orc, (2, 2), 403)
    pt = r.words(orc, (2,), 404)[1]          # q - 1 in every word
    got = r.ev.multiply_plain(Ciphertext(r.dev(ct), True), Plaintext(r.dev(pt), True))
    assert np.array_equal(host(got.data), orc.dyadic("mul", ct, np.ascontiguousarray(np.broadcast_to(pt, ct.shape))))
    count = 520 if L * n <= 16384 else 130   # both past 8 items for each of the 15 splits
    cts = orc.fill(count * 2, 405).reshape(count, 2, L, n)
    cts[:, :, :, : n // 2] = r.qcol - np.uint64(1)
    got = r.ev.reduce_sum(Ciphertext(r.dev(cts)))
    assert np.array_equal(host(got.data), orc.reduce_sum(cts.ravel(), 2)), count
    # rescale: round(x / q_last) on the first L - 1 limbs
    z = r.words(orc, (3, 2), 406)
    assert np.array_equal(host(r.ev.rescale_words(r.dev(z))), orc.rescale(z))
    # exact base extension and scale-and-round between edge primes (at most 8 source limbs on the generic path)
    w = r.words(orc, (2,), 407)
    for src0, ns, dst0, nd in ((0, 2, 0, L), (L - 2, 2, 0, L - 2), (0, L - 1, L - 1, 1)):
        xs = np.ascontiguousarray(w[:, src0:src0 + ns])
        got = host(r.ev.base_extend(r.dev(xs), src0, dst0, nd))
        assert np.array_equal(got, orc.base_extend(xs, src0, dst0, nd)), (src0, ns, dst0, nd)
    for drop0, ndrop, keep0, nkeep, mul in ((L - 1, 1, 0, L - 1, 65537), (0, 2, 2, L - 2, 1), (0, 1, 1, L - 1, (1 << 20) + 7)):
        got = host(r.ev.scale_round(r.dev(w), drop0, ndrop, keep0, nkeep, mul))
        assert np.array_equal(got, orc.scale_round(w, drop0, ndrop, keep0, nkeep, mul)), (drop0, ndrop, keep0, nkeep, mul)


# ---- matvec accumulation periods ------------------------------------------------------------------------------------------------------------------------------
MATVEC_COLS = (127, 128, 129, 256, 257)


@pytest.mark.parametrize("kind", ["shoup60", "fold2"], ids=["shoup60", "fold_edge"])
@pytest.mark.parametrize("cols", MATVEC_COLS)
def test_matvec_accumulation_periods_at_the_class_edges(rig, kind, cols):
    """matvec_plain and matvec_scalar with q - 1 in every word of W and of half of x, rows a multiple of the row tile (8) and not (5).

    The generic matvec (kernels_linalg.h matvec_kernel / matvec_scalar_kernel / matvec_multi_kernel) adds 128-bit products and folds its accumulators
    every 128 columns.  That 128 is conservative: with q < 2^60 - 2^24 (shoup60), 256 products of (q - 1)^2 next to a reduced value still stay below
    2^128, but 257 do not.  So this test guards the real limit - a fold period past 256 columns fails at cols = 257 - and does not pin the number 128:
    a period as wrong as 136 would not overflow here.  The fold matvec folds its split-at-bit-30 columns every FoldArith::kDot30Period = 8 terms; on
    the fold_edge context (d close to 2^24, the largest fold constant) the same shapes cross that period many times over."""
    from deeppowers_amd.evaluator import Ciphertext, Plaintext
    r = rig(kind, 12)
    L, n, orc = r.L, r.n, r.orc
    qm1 = r.qcol - np.uint64(1)
    rng = np.random.default_rng(cols)
    x = orc.fill(cols * 2, 500 + cols).reshape(cols, 2, L, n)
    x[..., : n // 2] = qm1
    dx = r.dev(x)
    for rows in (8, 5):
        W = np.empty((rows, cols, L, n), np.uint64)
        W[...] = qm1
        got = r.ev.matvec_plain(Plaintext(r.dev(W), True), Ciphertext(dx, True))
        assert np.array_equal(host(got.data), orc.matvec_plain(W.ravel(), x.ravel(), rows, cols, threads=0)), ("plain", rows)
        w = (rng.integers(0, 1 << 62, (rows, cols, L), dtype=np.uint64) % np.array(r.p.moduli, np.uint64)).astype(np.uint64)
        w[: rows - 1] = np.array(r.p.moduli, np.uint64) - np.uint64(1)
        got = r.ev.matvec_scalar(r.dev(w), Ciphertext(dx, True))
        assert np.array_equal(host(got.data), orc.matvec_scalar(w, x, rows, cols, threads=0)), ("scalar", rows)


@pytest.mark.parametrize("kind", ["shoup60", "fold2"], ids=["shoup60", "fold_edge"])
def test_matvec_plain_multi_at_the_class_edges(rig, kind):
    """matvec_plain_multi at a shape that takes the branch-free FULL form of the fold kernel (rows % 4 == 0, cols % 8 == 0) and a ragged one, past the
    generic kernel's 256-column limit, three right-hand sides (one pair and an odd one), q - 1 in W and in half of x"""
    from deeppowers_amd.evaluator import Plaintext
    r = rig(kind, 12)
    L, n, orc = r.L, r.n, r.orc
    qm1 = r.qcol - np.uint64(1)
    n_rhs = 3
    for rows, cols in ((8, 264), (5, 257)):
        W = orc.fill(rows * cols, 600 + cols).reshape(rows, cols, L, n)
        W[:, :, :, : n // 2] = qm1
        W[0] = qm1
        x = orc.fill(cols * n_rhs * 2, 601 + cols).reshape(cols, n_rhs, 2, L, n)
        x[..., : n // 2] = qm1
        x[:, 1] = qm1
        got = host(r.ev.matvec_plain_multi(Plaintext(r.dev(W), True), r.dev(x), n_rhs))
        for t in range(n_rhs):
            want = orc.matvec_plain(W.ravel(), np.ascontiguousarray(x[:, t]).ravel(), rows, cols, threads=0)
            assert np.array_equal(got[:, t], want), (rows, cols, t)
