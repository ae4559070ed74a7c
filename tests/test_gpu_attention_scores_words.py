"""-m gpu: the attention-scores step on TRANSPARENT inputs, word for word against the big-integer model (tests/attention_scores_model.py): the three entries
ApproxAttentionScores::apply chains - dpfhe_ct_mul_outer on the input level, dpfhe_relinearize_rescale_hybrid over all pairs, dpfhe_rotate_add_hybrid with
SlotSum's elements on the next level - through the Python mirror, with RANDOM keys (every key-switch digit of a transparent input is zero: the keys cannot
matter, and a kernel that let them would show).  tests/cpp/attention/test_attention_api.cpp holds apply() itself to the same chain on encrypted inputs.
Both packings, full and causal, T in {1, 3, 5} at N = 1024; one case at N = 32768 with T = 2."""
import numpy as np
import pytest

import attention_scores_model as am
from deeppowers_amd.evaluator import Ciphertext, Context, Evaluator, to_device, to_host
from deeppowers_amd.params import FheParams
from oracle.cbind import Oracle

pytestmark = pytest.mark.gpu

CASES = [(10, T, pk, causal) for pk in ("one", "heads") for causal in (False, True) for T in (1, 3, 5)] + [(15, 2, "heads", True)]


@pytest.mark.parametrize("log2n,T,pk,causal", CASES)
def test_device_words_equal_the_integer_model(log2n, T, pk, causal):
    import torch
    c = am.Case(log2n, T, pk, causal)
    qp, kp = c.polynomials(c.q), c.polynomials(c.k)
    _, scores = am.model(c, qp, kp)
    d = c.data
    ext_p = FheParams(log2n, tuple(d.moduli) + (c.special,), tuple(d.psi) + (c.special_psi,))
    ext2_p = FheParams(log2n, tuple(d.moduli[:-1]) + (c.special,), tuple(d.psi[:-1]) + (c.special_psi,))
    ctxs = [Context(p, 0) for p in (d, ext_p, ext2_p)]
    try:
        data, ext, ext2 = ctxs
        dev = data.device
        Ld, n = len(d.moduli), c.n
        key = Oracle.from_params(ext_p).fill(Ld * 2, 81).reshape(Ld, 2, Ld + 1, n)
        elts = am.elements(c.pk["block"], c.pk["stride"], n)
        lkeys = Oracle.from_params(ext2_p).fill(len(elts) * (Ld - 1) * 2, 82).reshape(len(elts), Ld - 1, 2, Ld, n)
        cq, ck = (Ciphertext(to_device(am.words(p, d.moduli), dev)) for p in (qp, kp))
        prod = Evaluator(data).multiply_outer(cq, ck, causal=causal)
        step = Evaluator(ext).relinearize_rescale_hybrid(prod, to_device(key, dev))
        got = Evaluator(ext2).rotate_add_hybrid(step, elts, to_device(lkeys, dev))
        torch.cuda.synchronize()
        got, want = to_host(got.data), am.words(scores, d.moduli[:-1])
        assert got.shape == want.shape == (len(c.pairs), 2, Ld - 1, n)
        assert not got[:, 1].any()                                                     # c1 stays zero: no key word reached the result
        assert np.array_equal(got, want), (log2n, T, pk, causal, np.argwhere(got != want)[:4])
    finally:
        for x in ctxs:
            x.close()
