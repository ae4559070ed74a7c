"""CPU: FheParams.n32768 - the N = 32768 chain the packed layers, blocks and stacks are built on at the one ring with room for more than one activated
block inside the 128-bit budget (881 bits): the first primes of ntt_primes(15, n); the first 8 are fold primes (2^60 - d, d < 2^24), the rest generic."""
import pytest

import class_edges
from deeppowers_amd.params import FheParams, ntt_primes


def test_n32768_is_the_head_of_the_generated_chain():
    chain = ntt_primes(15, 14)
    for k in range(1, 15):
        p = FheParams.n32768(k)
        assert p.log2_n == 15 and p.moduli == chain.moduli[:k] and p.psi == chain.psi[:k]
        assert p == ntt_primes(15, k)
    assert all(q % 65536 == 1 for q in chain.moduli)
    assert [class_edges.expected_class(q) == "fold" for q in chain.moduli] == [True] * 8 + [False] * 6
    assert {class_edges.expected_class(q) for q in chain.moduli[8:]} == {"shoup"}


@pytest.mark.parametrize("k", [0, 15])
def test_n32768_rejects_counts_outside_the_chain(k):
    with pytest.raises(ValueError):
        FheParams.n32768(k)
