"""GPU (-m gpu): dpfhe_reduce_sum against the oracle where it picks reduce_thin_kernel (all-fold limbs, count > 512) and right below that threshold:
all-(q - 1) inputs (every lazy sum at its bound), the benchmark's shard (8192 x 3 x 4 x 4096 random words), both sides of count = 512 at several
ring degrees (N = 256 runs half-filled chunks), and a generic-prime context above the threshold (the other kernel).  Bit-exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from deeppowers_amd.evaluator import Ciphertext, to_host  # noqa: E402
from test_gpu_parity import rigs  # noqa: E402,F401  (the module-scoped contexts of the parity suite)


def _oracle_sum(r, x, comps):
    """the oracle's modular sum of x: [count][comps][L][N] on the host, 1024 items at a time (the sum is associative and exact)"""
    parts = [r.orc.reduce_sum(np.ascontiguousarray(x[lo:lo + 1024]).ravel(), comps) for lo in range(0, x.shape[0], 1024)]
    return parts[0] if len(parts) == 1 else r.orc.reduce_sum(np.concatenate([p.ravel() for p in parts]), comps)


@pytest.mark.parametrize("name,count,comps", [("n4096", 1000, 3), ("n4096", 513, 2), ("fold8", 8192, 3), ("n8192", 600, 2)])
def test_all_q_minus_one_inputs(rigs, name, count, comps):
    r = rigs(name)
    assert r.ctx.uses_fold
    L, n = r.p.n_limbs, r.p.n
    x = np.empty((count, comps, L, n), np.uint64)
    x[:] = (np.array(r.p.moduli, np.uint64) - np.uint64(1))[None, None, :, None]
    got = to_host(r.ev.reduce_sum(Ciphertext(r.dev(x))).data)
    want = np.array([(count * (q - 1)) % q for q in r.p.moduli], np.uint64)
    assert np.array_equal(got, np.broadcast_to(want[None, :, None], got.shape))   # closed form
    assert np.array_equal(got.ravel(), _oracle_sum(r, x, comps).ravel())          # and the oracle


def test_the_benchmark_shard_random_words(rigs):
    """8192 x 3 x 4 x 4096 random canonical words (3 GiB), every output word against the oracle"""
    r = rigs("n4096")
    L, n, count = 4, 4096, 8192
    dev = r.ctx.device
    g = torch.Generator(device=dev).manual_seed(1013)
    q = torch.tensor(r.p.moduli, dtype=torch.int64, device=dev).view(1, 1, L, 1)
    x = torch.randint(0, 2**62, (count, 3, L, n), generator=g, dtype=torch.int64, device=dev) % q
    got = to_host(r.ev.reduce_sum(Ciphertext(x)).data)
    parts = [r.orc.reduce_sum(to_host(x[lo:lo + 1024]).ravel(), 3) for lo in range(0, count, 1024)]
    want = r.orc.reduce_sum(np.concatenate([p.ravel() for p in parts]), 3)
    assert np.array_equal(got.ravel(), want.ravel())
    # and on a second stream, twice into the same buffer (the call zeroes its output itself)
    side = torch.cuda.Stream(device=dev)
    out = r.ctx.empty(components=3)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            r.ev.reduce_sum(Ciphertext(x), out=out, stream=side)
    side.synchronize()
    assert np.array_equal(to_host(out).ravel(), want.ravel())


@pytest.mark.parametrize("name", ["n4096", "fold8", "fold9", "fold11", "shoup10"])
@pytest.mark.parametrize("count", [511, 512, 513, 527, 1031])
def test_both_sides_of_the_threshold(rigs, name, count):
    r = rigs(name)
    comps = 2
    L, n = r.p.n_limbs, r.p.n
    x = r.orc.fill(count * comps, 7 + count).reshape(count, comps, L, n)
    x[::3, :, :, :8] = (np.array(r.p.moduli, np.uint64) - np.uint64(1))[None, None, :, None]
    got = to_host(r.ev.reduce_sum(Ciphertext(r.dev(x))).data)
    assert np.array_equal(got.ravel(), _oracle_sum(r, x, comps).ravel())
