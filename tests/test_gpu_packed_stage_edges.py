"""-m gpu: the stages the packed encrypted layers run on - the baby-step / giant-step sums with the division by P deferred (include/dpfhe.h "N3, round
3"), the multi-right-hand-side plaintext product and the exact multiply - at the edges of the per-limb arithmetic classes, through the C ABI against
oracle.c.

tests/test_gpu_class_edges.py holds the transforms, the multiply and the non-deferred key switches to the oracle at the edge primes;
tests/test_gpu_bsgs_qp.py runs the deferred stages on the pinned fold primes and one small context of fold_scaled and f64 primes.  Here every context
is an edge context (tests/class_edges.py): the uniform context of each class at N = 4096, 8192 and 16384 (where the stages are composed from the batched
transforms), the all-class mixture, and the deployable hybrid shape - data limbs of one class under a special prime P of another (class_edges.MIXED_P),
where the key-switching kernels launch once per class, the transform of the data limbs sees one class among a truncated limb count, and the one-pass
kernels reduce P, or a residue mod P, into a much narrower (or wider) limb.  Every comparison is a whole buffer, or the stated set of blocks, word for
word against the oracle (threads=0), whose exactness for these functions at these primes tests/test_packed_stage_edges_cpu.py shows against Python
integers.  Inputs come from Rig.words: worst_case stripes in item 0 and q - 1 in every word of item 1, in the ciphertexts and in the keys.  Every rig
first asserts the classes its limbs run on."""
import numpy as np
import pytest

from class_edges import (CLASSES, FSCALED_ORDER, MIXED_P, Rig, catalogue, edge_moduli, expected_class, neighbour, reported_classes,
                         rescale_bsgs_reference)
from deeppowers_amd.params import FheParams, min_primitive_2n_root
from oracle import pyoracle as po
from oracle.cbind import Oracle

pytestmark = pytest.mark.gpu

# the second ring degree of each hybrid shape (the first is N = 4096)
MIXED_P_SECOND = {"f64_under_fold": 14, "fold_scaled_under_shoup": 14, "f64_wide_under_fold_scaled": 13, "shoup_under_f64": 13, "fold_under_smallest": 13}
CONTEXTS = ([(k, ln) for ln in (12, 13) for k in CLASSES + ("mixed",)] + [(k, 14) for k in CLASSES]
            + [(k, 12) for k in MIXED_P] + [(k, MIXED_P_SECOND[k]) for k in MIXED_P])
IDS = [f"{k}_n{1 << ln}" for k, ln in CONTEXTS]


@pytest.fixture
def rig():
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


def data_oracle(r):
    """the oracle of the data limbs (the extended context without its special prime)"""
    return Oracle(r.p.log2_n, r.p.moduli[:-1], r.p.psi[:-1])


# ---- dpfhe_rotate_hoisted_qp ------------------------------------------------------------------------------------------------------------------------------
# k = 66 crosses the 64-rotation launch group (kMaxGaloisBatch) and four 16-rotation blocks (kQpRotGroup): every launch group and every rotation-group
# boundary has a compared member on both sides
CHECKED_OF_66 = (0, 1, 15, 16, 63, 64, 65)


def _rotate_hoisted_qp(r, k, T, seed):
    from deeppowers_amd.evaluator import Ciphertext
    L, Ld, n, orc = r.L, r.L - 1, r.n, r.orc
    data = data_oracle(r)
    elts = [pow(3, i + 1, 2 * n) for i in range(k)]
    if k:
        elts[-1] = 2 * n - 1
    keys = r.words(orc, (max(k, 2), Ld, 2), seed)[:k]        # stripes in key 0, q - 1 in every word of key 1
    if k > 2:
        keys[k - 1] = keys[0]                                  # ... and the stripes again under g = 2N - 1, the last rotation
    cts = r.words(data, (max(T, 2), 2), seed + 1)[:T]
    if T == 1:
        cts[0, 1] = (r.qcol - np.uint64(1))[:Ld]               # one token: stripes in c0, every digit word q - 1
    got = host(r.ev.rotate_hoisted_qp(Ciphertext(r.dev(cts)), elts, r.dev(keys) if k else None))
    assert got.shape == (k + 1, T, 2, L, n)
    idx = list(range(k)) if k <= 8 else list(CHECKED_OF_66)
    for t in range(T):
        want = orc.rotate_hoisted_qp(cts[t], [elts[i] for i in idx], keys[idx], threads=0)
        assert np.array_equal(got[0, t], want[0]), (k, t, "identity block")
        for w, i in zip(want[1:], idx):
            assert np.array_equal(got[1 + i, t], w), (k, t, i)


@pytest.mark.parametrize("kind,log2n", CONTEXTS, ids=IDS)
def test_rotate_hoisted_qp_at_the_class_edges(rig, kind, log2n):
    """(k rotations, T tokens) = (5, 1) and (0, 2), every block compared: the transform of the data limbs alone (one class among a truncated limb
    count on the hybrid shapes), lift_qp_kernel's P mod q_i and hoisted_qp_stream_kernel's key products on every limb"""
    r = rig(kind, log2n)
    for k, T in ((5, 1), (0, 2)):
        _rotate_hoisted_qp(r, k, T, 700 + k)


@pytest.mark.parametrize("kind", CLASSES)
def test_rotate_hoisted_qp_across_the_launch_groups_at_the_class_edges(rig, kind):
    """66 rotations of 3 tokens at N = 4096: the identity block and rotations {0, 1, 15, 16, 63, 64, 65} of every token"""
    assert len(CHECKED_OF_66) == 7 and {15, 16, 63, 64} <= set(CHECKED_OF_66)
    _rotate_hoisted_qp(rig(kind, 12), 66, 3, 710)


# ---- dpfhe_ntt_inv_galois ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,log2n", CONTEXTS, ids=IDS)
def test_ntt_inverse_galois_at_the_class_edges(rig, kind, log2n):
    """sigma_g(INTT(x)) with the automorphism as a gather in the NTT domain: 70 elements (two launch groups), 3 RNS polynomials per element, out of
    place and in place, g = 1 and g = 2N - 1 included; the stripes and the all-(q - 1) polynomials also under g = 2N - 1 and in the second launch group"""
    r = rig(kind, log2n)
    n, orc = r.n, r.orc
    k, per = 70, 3
    elts = [pow(3, 5 * i, 2 * n) for i in range(k)]
    assert elts[0] == 1
    elts[2] = elts[k - 1] = 2 * n - 1
    x = r.words(orc, (k, per), 720)
    x[2], x[3], x[65], x[k - 1] = x[0], x[1], x[0], x[1]
    inv = orc.ntt_inv(x, threads=0)
    want = np.stack([orc.apply_galois(inv[e], elts[e]) for e in range(k)])
    d = r.dev(x)
    assert np.array_equal(host(r.ev.ntt_inverse_galois(d, elts)), want)
    r.ev.ntt_inverse_galois(d, elts, out=d)
    assert np.array_equal(host(d), want)


# ---- dpfhe_switch_key_qp ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,log2n", CONTEXTS + [("fold_scaled6", 13)], ids=IDS + ["fold_scaled6_n8192"])
def test_switch_key_qp_at_the_class_edges(rig, kind, log2n):
    """(keys, items per key) = (1, 3), (5, 1), (9, 4), every item compared: relin_kernel MODE 4 on the class's own policy (uniform contexts), once per
    class (the mixture and the hybrid shapes), key_products_composed at N = 16384; fold_scaled6: five digits and P, all fold_scaled edge primes"""
    from deeppowers_amd.evaluator import Ciphertext
    r = rig(kind, log2n)
    L, Ld, n, orc = r.L, r.L - 1, r.n, r.orc
    data = data_oracle(r)
    for k, group in ((1, 3), (5, 1), (9, 4)):
        keys = r.words(orc, (max(k, 2), Ld, 2), 730 + k)[:k]
        items = r.words(data, (k * group, 2), 740 + k)
        if k > 1:
            items[k * group - 1] = items[0]                    # the stripes under the last key as well
        got = host(r.ev.switch_key_qp(Ciphertext(r.dev(items)), r.dev(keys), group))
        assert got.shape == (k * group, 2, L, n)
        for i in range(k):
            want = orc.switch_key_qp(items[i * group:(i + 1) * group], keys[i], threads=0)
            assert np.array_equal(got[i * group:(i + 1) * group], want), (k, group, i)


# ---- dpfhe_rescale_bsgs and the whole deferred sum -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,log2n", CONTEXTS, ids=IDS)
def test_rescale_bsgs_and_the_whole_deferred_sum_at_the_class_edges(rig, kind, log2n):
    """dpfhe_rescale_bsgs with 0, 1 and 6 addends == round(x / P) + addends (oracle composition); then the deferred giant-step sum
         rescale_bsgs(INTT(reduce_sum_i switch_key_qp(rot_i)), rot)
    against the oracle run in the same order, bit for bit; against the per-term path (one rounding per term) it differs by at most the number of
    terms in every coefficient."""
    import torch
    from deeppowers_amd import _cabi
    from deeppowers_amd.evaluator import Ciphertext
    r = rig(kind, log2n)
    L, Ld, n, orc = r.L, r.L - 1, r.n, r.orc
    data = data_oracle(r)
    n2, T = 6, 3
    rot = r.words(data, (n2, T, 2), 750)                       # [n2][T][2][Ld][N]: stripes in addend 0, q - 1 in every word of addend 1
    t_qp = r.words(orc, (T, 2), 751)
    d_rot, d_t = r.dev(rot), r.dev(t_qp)
    for count in (0, 1, n2):
        got = host(r.ev.rescale_bsgs(d_t, d_rot[:count]))
        assert np.array_equal(got, rescale_bsgs_reference(orc, data, t_qp, rot[:count])), count
    # the whole deferred sum on the GPU
    keys = r.words(orc, (n2 - 1, Ld, 2), 752)
    terms = r.ev.switch_key_qp(Ciphertext(d_rot[1:].reshape((n2 - 1) * T, 2, Ld, n)), r.dev(keys), T)      # [(n2-1) T][2][L][N]
    summed = torch.empty((T, 2, L, n), dtype=torch.int64, device=r.ctx.device)
    _cabi.check(r.ctx._lib.dpfhe_reduce_sum(r.ctx.handle, summed.data_ptr(), terms.data_ptr(), n2 - 1, T * 2, None), "dpfhe_reduce_sum")
    r.ev.ntt_inverse_(summed)
    got = host(r.ev.rescale_bsgs(summed, d_rot))
    # the oracle, same order of operations (bit exact) ...
    acc = np.zeros((T, 2, L, n), np.uint64)
    for i in range(1, n2):
        acc = orc.dyadic("add", acc, orc.switch_key_qp(rot[i], keys[i - 1], threads=0))
    want = rescale_bsgs_reference(orc, data, orc.ntt_inv(acc, threads=0), rot)
    assert np.array_equal(got, want)
    # ... and against the per-term path: the sums differ by the roundings only
    per_term = rot[0].copy()
    for i in range(1, n2):
        per_term = data.dyadic("add", per_term, orc.keyswitch_hybrid(rot[i], keys[i - 1], 2, threads=0))
    q = np.array(r.p.moduli[:-1], np.uint64)[None, None, :, None]
    diff = (got.astype(object) - per_term.astype(object)) % q.astype(object)
    diff = np.minimum(diff, q.astype(object) - diff)
    assert int(diff.max()) <= n2


# ---- dpfhe_matvec_plain_multi -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f64", "fold_scaled", "f64_wide", "fold_scaled_under_shoup"])
def test_matvec_plain_multi_at_the_class_edges(rig, kind):
    """(tests/test_gpu_class_edges.py has shoup60 and fold_edge) the generic multi-right-hand-side product on f64, fold_scaled and f64_wide edge primes
    and on a hybrid shape: a full shape and a ragged one past the generic kernel's 256-column limit, three right-hand sides, q - 1 in W and in half of x"""
    from deeppowers_amd.evaluator import Plaintext
    r = rig(kind, 12)
    L, n, orc = r.L, r.n, r.orc
    qm1 = r.qcol - np.uint64(1)
    n_rhs = 3
    for rows, cols in ((8, 264), (5, 257)):
        W = orc.fill(rows * cols, 760 + cols).reshape(rows, cols, L, n)
        W[:, :, :, : n // 2] = qm1
        W[0] = qm1
        x = orc.fill(cols * n_rhs * 2, 761 + cols).reshape(cols, n_rhs, 2, L, n)
        x[..., : n // 2] = qm1
        x[:, 1] = qm1
        got = host(r.ev.matvec_plain_multi(Plaintext(r.dev(W), True), r.dev(x), n_rhs))
        for t in range(n_rhs):
            want = orc.matvec_plain(W.ravel(), np.ascontiguousarray(x[:, t]).ravel(), rows, cols, threads=0)
            assert np.array_equal(got[:, t], want), (rows, cols, t)


# ---- Evaluator.multiply_exact -----------------------------------------------------------------------------------------------------------------------------
LEVEL_LIMBS = 2


def exact_moduli(kind, log2n, level_limbs=LEVEL_LIMBS):
    """a context for the exact multiply at the edge of one class: level_limbs data primes and level_limbs + 1 auxiliary primes, all of that class - the
    catalogue's edge primes, then the next primes of the class inward (class_edges.neighbour); 'mixed': the all-class mixture as it stands"""
    if kind == "mixed":
        return edge_moduli("mixed", log2n)
    need = 2 * level_limbs + 1
    cat = catalogue(log2n)
    if kind == "fold_scaled":     # the edge primes of several shifts, then the second prime of each shift
        qs = [e[i][0] for i in range(4) for k in FSCALED_ORDER for e in [cat.get(f"fscaled_edge_{k}", ())] if len(e) > i][:need]
    else:
        entry = {"f64": "f64_edge", "f64_wide": "f64_wide_edge", "shoup": "shoup60"}[kind]
        qs = [q for q, _ in cat[entry]][:need]
        q = qs[-1]
        while len(qs) < need:
            q = neighbour(q, log2n, -1)
            if expected_class(q) == kind:
                qs.append(q)
    assert len(qs) == need and len(set(qs)) == need and all(expected_class(q) == kind for q in qs), (kind, log2n)
    return FheParams(log2n, tuple(qs), tuple(min_primitive_2n_root(1 << log2n, q) for q in qs))


class ExactRig(Rig):
    def __init__(self, kind, log2n):
        from deeppowers_amd.evaluator import Context, Evaluator
        self.kind, self.p = kind, exact_moduli(kind, log2n)
        self.L, self.n = self.p.n_limbs, self.p.n
        self.orc = Oracle.from_params(self.p)
        self.ctx = Context(self.p, 0)
        self.ev = Evaluator(self.ctx)
        self.qcol = np.array(self.p.moduli, np.uint64)[:, None]
        assert self.ctx.limb_classes == reported_classes(self.p), (kind, log2n, self.ctx.limb_classes, [hex(q) for q in self.p.moduli])
        assert set(self.ctx.limb_classes) == (set(CLASSES) if kind == "mixed" else {kind})


EXACT = [(k, 12) for k in CLASSES[1:] + ("mixed",)] + [("f64", 14), ("fold_scaled", 14)]


@pytest.mark.parametrize("kind,log2n", EXACT, ids=[f"{k}_n{1 << ln}" for k, ln in EXACT])
def test_multiply_exact_at_the_class_edges(kind, log2n):
    """Evaluator.multiply_exact == the oracle's pipeline base_extend -> ct_mul -> scale_round -> base_extend (tests/test_gpu_exact_multiply.py composes it
    this way on fold primes), word for word, squaring included: the per-class fused multiply (the composed one at N = 16384) between the exact base
    extensions, on level_limbs edge primes of one class with level_limbs + 1 auxiliary primes of the same class, and on the all-class mixture"""
    r = ExactRig(kind, log2n)
    try:
        orc, L, ll, t, n = r.orc, r.L, LEVEL_LIMBS, 65537, r.n
        level = Oracle(log2n, r.p.moduli[:ll], r.p.psi[:ll])
        a = r.words(level, (3, 2), 770)
        b = r.words(level, (3, 2), 771)
        b[0] = np.roll(b[0], n // 16, axis=-1)
        A, B = orc.base_extend(a, 0, 0, L), orc.base_extend(b, 0, 0, L)
        for x, y, X, Y in ((a, b, A, B), (a, a, A, A)):
            T = orc.ct_mul(np.ascontiguousarray(X), np.ascontiguousarray(Y), threads=0)
            want = orc.base_extend(orc.scale_round(T, 0, ll, ll, L - ll, t), ll, 0, ll)
            dx = r.dev(x)
            got = host(r.ev.multiply_exact(dx, dx if y is x else r.dev(y), ll, t))
            assert got.shape == (3, 3, ll, n) and np.array_equal(got, want), "squaring" if y is x else "product"
    finally:
        r.close()


def test_multiply_exact_on_the_mixture_decrypts_to_the_product():
    """the decryption-level check of tests/test_gpu_exact_multiply.py on the all-class mixture (a fold and an f64 edge prime as the level, six limbs of
    the other classes as the workspace), on a small ring: the result decrypts to m1 * m2 mod (X^N + 1, t) under a toy BFV scheme in Python integers"""
    r = ExactRig("mixed", 8)
    try:
        p, ll, t, n = r.p, LEVEL_LIMBS, 65537, r.n
        rng = np.random.default_rng(13)
        q = p.moduli[0] * p.moduli[1]
        delta = q // t
        s = rng.integers(-1, 2, n)

        def encrypt(m):
            e = rng.integers(-8, 9, n)
            ct = np.zeros((2, ll, n), np.uint64)
            for i, qi in enumerate(p.moduli[:ll]):
                a_ = [int(rng.integers(0, 2**62)) % qi for _ in range(n)]
                a_s = po.negacyclic_schoolbook(a_, [int(v) % qi for v in s], qi)
                ct[0, i] = [(-a_s[k] + int(e[k]) + delta * int(m[k])) % qi for k in range(n)]
                ct[1, i] = a_
            return ct
        m1, m2 = rng.integers(0, t, n), rng.integers(0, t, n)
        m1[: n // 8], m2[: n // 8] = t - 1, t - 1
        c1, c2 = encrypt(m1), encrypt(m2)
        c3 = host(r.ev.multiply_exact(r.dev(c1[None]), r.dev(c2[None]), ll, t))[0]    # [3][ll][N]
        ph = []
        for i, qi in enumerate(p.moduli[:ll]):          # phase = c0 + c1 s + c2 s^2 per limb, then CRT
            sq = [int(v) % qi for v in s]
            s2 = po.negacyclic_schoolbook(sq, sq, qi)
            ph.append(po.poly_add(po.poly_add([int(v) for v in c3[0, i]], po.negacyclic_schoolbook([int(v) for v in c3[1, i]], sq, qi), qi),
                                  po.negacyclic_schoolbook([int(v) for v in c3[2, i]], s2, qi), qi))
        want_m = po.negacyclic_schoolbook([int(v) for v in m1], [int(v) for v in m2], t)
        for k in range(n):
            x = po.crt_centered([ph[i][k] for i in range(ll)], p.moduli[:ll])
            assert ((2 * t * x + q) // (2 * q)) % t == want_m[k], k
    finally:
        r.close()
