"""GPU (-m gpu): dpfhe_ct_mul at N = 4096 on fold contexts - ct_mul_quad_kernel's lazy transforms (twiddles split at bit 29, unreduced butterfly
products) - every output word against the oracle: 1, 2 and 4 limbs of the bench primes and of the fold edge primes, 3 pairs of all-(q - 1), all-zero,
random and alternating 0 / q - 1 inputs, coefficient-domain and DPFHE_OUT_NTT output; and 520 pairs whose products the thin reduce sums."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import class_edges  # noqa: E402
from deeppowers_amd.evaluator import Ciphertext, Context, Evaluator, to_device, to_host  # noqa: E402
from deeppowers_amd.params import FheParams  # noqa: E402
from oracle.cbind import Oracle  # noqa: E402

N, PAIRS = 4096, 3
SOURCES = {"bench": FheParams.n4096_l4(), "edge": class_edges.edge_moduli("fold", 12)}


class Rig:
    def __init__(self, kind, limbs):
        src = SOURCES[kind]
        self.p = FheParams(12, tuple(src.moduli[:limbs]), tuple(src.psi[:limbs]))
        self.orc = Oracle.from_params(self.p)
        self.ctx = Context(self.p, 0)
        self.ev = Evaluator(self.ctx)


@pytest.fixture(scope="module")
def rigs():
    cache = {}

    def get(kind, limbs):
        if (kind, limbs) not in cache:
            cache[kind, limbs] = Rig(kind, limbs)
        return cache[kind, limbs]

    yield get
    for r in cache.values():
        r.ctx.close()


def patterns(r, seed):
    L = r.p.n_limbs
    qm1 = (np.array(r.p.moduli, np.uint64) - np.uint64(1))[None, None, :, None]
    shape = (PAIRS, 2, L, N)
    even = (np.arange(N) % 2 == 0)[None, None, None, :]
    alt_a = np.where(even, np.uint64(0), np.broadcast_to(qm1, shape)).astype(np.uint64)
    alt_b = np.where(even, np.broadcast_to(qm1, shape), np.uint64(0)).astype(np.uint64)
    alt_b[1] = alt_a[1]                                   # pair 1: both operands on the same phase
    return {
        "max": (np.broadcast_to(qm1, shape).copy(), np.broadcast_to(qm1, shape).copy()),
        "zero": (np.zeros(shape, np.uint64), np.zeros(shape, np.uint64)),
        "random": (r.orc.fill(PAIRS * 2, seed).reshape(shape), r.orc.fill(PAIRS * 2, seed + 1).reshape(shape)),
        "alternating": (alt_a, alt_b),
    }


@pytest.mark.parametrize("limbs", [1, 2, 4])
@pytest.mark.parametrize("kind", ["bench", "edge"])
def test_lazy_multiply_matches_oracle_word_for_word(rigs, kind, limbs):
    r = rigs(kind, limbs)
    assert r.ctx.uses_fold
    for pat, (a, b) in patterns(r, 2900 + limbs).items():
        want = r.orc.ct_mul(np.ascontiguousarray(a), np.ascontiguousarray(b), threads=0)
        A, B = Ciphertext(to_device(a, r.ctx.device)), Ciphertext(to_device(b, r.ctx.device))
        c = r.ev.multiply(A, B)
        assert not c.is_ntt and np.array_equal(to_host(c.data), want), pat
        want_ntt = r.orc.ntt_fwd(want.reshape(-1, limbs, N), threads=0).reshape(want.shape)
        c2 = r.ev.multiply(A, B, out_ntt=True)
        assert c2.is_ntt and np.array_equal(to_host(c2.data), want_ntt), pat


def test_thin_reduce_of_520_lazy_products_equals_the_oracles_sum(rigs):
    r = rigs("bench", 4)
    count, L = 520, 4
    a = r.orc.fill(count * 2, 3100).reshape(count, 2, L, N)
    b = r.orc.fill(count * 2, 3101).reshape(count, 2, L, N)
    qm1 = (np.array(r.p.moduli, np.uint64) - np.uint64(1))[None, :, None]
    a[0, :, :, : N // 4] = qm1
    b[0, :, :, : N // 4] = qm1
    prods = r.ev.multiply(Ciphertext(to_device(a, r.ctx.device)), Ciphertext(to_device(b, r.ctx.device)))
    total = to_host(r.ev.reduce_sum(prods).data)
    want = r.orc.ct_mul(np.ascontiguousarray(a), np.ascontiguousarray(b), threads=0)
    assert np.array_equal(to_host(prods.data), want)
    assert np.array_equal(total.ravel(), r.orc.reduce_sum(np.ascontiguousarray(want).ravel(), 3).ravel())
