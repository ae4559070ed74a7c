"""GPU (-m gpu): dpfhe_ct_mul at N = 4096 on the pinned primes after the inverse butterflies' multiples of q moved (scalar pairs, and the product chains'
addends where the bound plan has room): 1 and 4 limbs, 1, 3 and 17 pairs, stripes of q - 1 in random words, as a plain product, as a squaring (both
operands the same buffer) and through the traced form of the kernel - every output word against the oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from deeppowers_amd import _cabi  # noqa: E402
from deeppowers_amd.evaluator import Ciphertext, Context, Evaluator, to_device, to_host  # noqa: E402
from deeppowers_amd.params import FheParams  # noqa: E402
from oracle.cbind import Oracle  # noqa: E402

N = 4096
BENCH = FheParams.n4096_l4()
MAX_PAIRS = 17


class Rig:
    def __init__(self, limbs):
        self.p = FheParams(12, tuple(BENCH.moduli[:limbs]), tuple(BENCH.psi[:limbs]))
        self.orc = Oracle.from_params(self.p)
        self.ctx = Context(self.p, 0)
        self.ctx.set_ct_mul_variant("quad")
        self.ev = Evaluator(self.ctx)
        # 17 pairs once; the smaller batches are their first items.  Stripes: pair 0 is all q - 1; elsewhere runs of 64 words alternate between q - 1 and
        # random words, on opposite phases in the two operands of odd pairs
        shape = (MAX_PAIRS, 2, limbs, N)
        qm1 = np.broadcast_to((np.array(self.p.moduli, np.uint64) - np.uint64(1))[None, None, :, None], shape)
        run = ((np.arange(N) // 64) % 2 == 0)[None, None, None, :]
        odd = (np.arange(MAX_PAIRS) % 2 == 1)[:, None, None, None]
        self.a = np.where(run, qm1, self.orc.fill(MAX_PAIRS * 2, 5100 + limbs).reshape(shape)).astype(np.uint64)
        self.b = np.where(run ^ odd, qm1, self.orc.fill(MAX_PAIRS * 2, 5200 + limbs).reshape(shape)).astype(np.uint64)
        self.a[0], self.b[0] = qm1[0], qm1[0]
        self.want = self.orc.ct_mul(np.ascontiguousarray(self.a), np.ascontiguousarray(self.b), threads=0)
        self.want_sq = self.orc.ct_mul(np.ascontiguousarray(self.a), np.ascontiguousarray(self.a), threads=0)


@pytest.fixture(scope="module")
def rigs():
    cache = {}

    def get(limbs):
        if limbs not in cache:
            cache[limbs] = Rig(limbs)
        return cache[limbs]

    yield get
    for r in cache.values():
        r.ctx.close()


@pytest.mark.parametrize("pairs", [1, 3, 17])
@pytest.mark.parametrize("limbs", [1, 4])
def test_product_squaring_and_traced_form_match_the_oracle_word_for_word(rigs, limbs, pairs):
    r = rigs(limbs)
    assert r.ctx.uses_fold
    A, B = Ciphertext(to_device(r.a[:pairs], r.ctx.device)), Ciphertext(to_device(r.b[:pairs], r.ctx.device))
    c = r.ev.multiply(A, B)
    assert not c.is_ntt and np.array_equal(to_host(c.data), r.want[:pairs]), "product"
    sq = r.ev.multiply(A, A)
    assert np.array_equal(to_host(sq.data), r.want_sq[:pairs]), "squaring"
    out = r.ctx.empty(pairs, components=3)
    trace = torch.zeros(pairs * limbs * 12, dtype=torch.int64, device=r.ctx.device)
    stream = torch.cuda.current_stream(r.ctx.device).cuda_stream
    _cabi.check(r.ctx._lib.dpfhe_debug_ct_mul_trace(r.ctx.handle, out.data_ptr(), A.data.data_ptr(), B.data.data_ptr(), pairs, trace.data_ptr(), stream), "dpfhe_debug_ct_mul_trace")
    torch.cuda.synchronize()
    assert np.array_equal(to_host(out), r.want[:pairs]), "traced form"
