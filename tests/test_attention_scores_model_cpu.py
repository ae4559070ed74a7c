"""CPU: the big-integer model of ApproxAttentionScores on a transparent input (tests/attention_scores_model.py), both packings at N = 256 and N = 1024:
* against the ORACLE limb by limb: ct_mul of the pair lists, the hybrid key switch (its digits are zero: the key's words do not matter, a random key is used),
  the rescale, then per ladder step acc + apply_galois(acc) on the next level;
* against the float64 scores, every slot of every pair, within the header's bound evaluated at zero input noise (recomputed here term by term);
* the seeded inputs' distinct expected scores differ by at least four times that bound - at the noise of a fresh encryption too, which is what the encrypted
  GPU test runs at - so a transposed or mis-indexed pair cannot pass there."""
import numpy as np
import pytest

import attention_scores_model as am
from oracle.cbind import Oracle

CASES = [(log2n, T, pk, causal) for log2n in (8, 10) for pk in ("one", "heads") for T, causal in ((3, True), (2, False))]


@pytest.fixture(scope="module")
def runs():
    made = {}

    def get(log2n, T, pk, causal):
        key = (log2n, T, pk, causal)
        if key not in made:
            c = am.Case(log2n, T, pk, causal)
            qp, kp = c.polynomials(c.q), c.polynomials(c.k)
            made[key] = (c, qp, kp) + am.model(c, qp, kp)
        return made[key]
    return get


@pytest.mark.parametrize("log2n,T,pk,causal", CASES)
def test_model_equals_the_oracle_limb_by_limb(runs, log2n, T, pk, causal):
    c, qp, kp, prods, scores = runs(log2n, T, pk, causal)
    d = c.data
    data = Oracle(log2n, d.moduli, d.psi)
    ext = Oracle(log2n, tuple(d.moduli) + (c.special,), tuple(d.psi) + (c.special_psi,))
    nxt = Oracle(log2n, d.moduli[:-1], d.psi[:-1])
    qa, kb = am.words(qp, d.moduli), am.words(kp, d.moduli)
    la, lb = np.stack([qa[i] for i, _ in c.pairs]), np.stack([kb[j] for _, j in c.pairs])
    ct3 = data.ct_mul(la, lb, threads=0)
    assert not ct3[:, 1:].any()                                                        # (a0 b0, 0, 0)
    key = ext.fill(len(d.moduli) * 2, 77).reshape(len(d.moduli), 2, len(d.moduli) + 1, c.n)
    step = data.rescale(ext.keyswitch_hybrid(ct3, key, 3, threads=0))
    assert np.array_equal(step, am.words(prods, d.moduli[:-1]))                        # c1 stays 0, c0 = round(a0 b0 / q_last)
    acc = step
    qcol = np.array(d.moduli[:-1], dtype=np.uint64)[:, None]
    for g in am.elements(c.pk["block"], c.pk["stride"], c.n):
        acc = (acc + nxt.apply_galois(acc, g)) % qcol
    assert np.array_equal(acc, am.words(scores, d.moduli[:-1]))


@pytest.mark.parametrize("log2n,T,pk,causal", CASES)
def test_model_is_within_the_bound_of_float64_and_pairs_are_told_apart(runs, log2n, T, pk, causal):
    c, _, _, _, scores = runs(log2n, T, pk, causal)
    want = c.scores()
    A, B = float(np.abs(c.q).max()), float(np.abs(c.k).max())
    bound0 = am.error_bound(c, A, B, 0.5, 0.5)                                         # a transparent input: the encoder's rounding alone
    s = np.arange(c.n // 2) % c.pk["stride"]
    worst = 0.0
    for a in range(len(c.pairs)):
        z = am.decode(c, scores[a])
        expect = np.where(s < c.pk["heads"], want[a][np.minimum(s, c.pk["heads"] - 1)], 0.0)
        worst = max(worst, float(np.abs(z.real - expect).max()), float(np.abs(z.imag).max()))
    print(f"N = {c.n} {pk} T = {T}: model within 2^{np.log2(worst):.2f} of float64, bound 2^{np.log2(bound0):.2f}")
    assert worst <= bound0
    fresh = 21.5 + 8.0 * log2n * am.U * am.SCALE * max(A, B)
    bound = am.error_bound(c, A, B, fresh, fresh)
    gaps = [abs(want[a][h] - want[b][h]) for a in range(len(c.pairs)) for b in range(a) for h in range(c.pk["heads"])]
    assert bound0 <= bound and min(gaps) >= 4 * bound, (min(gaps), bound)
