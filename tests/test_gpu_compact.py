"""-m gpu: compact result ciphertexts on the device (include/dpfhe.h dpfhe_compact, csrc/k_compact.hip).

The kernel must give the host twin's bytes (tests/test_compact_cpu.py holds the host twin to the definition) on every ring degree, limb count and
limb class, for odd batches, without writing past the records or touching the input.  Through the C++ facade (tests/cpp/test_compact_api.cpp):
a fresh ciphertext, a biased 768 x 768 PackedLinear at N = 8192 and an activated FFN at N = 16384 decrypt exactly from compact form."""
import subprocess

import numpy as np
import pytest

import cpp_build
from deeppowers_amd import _cabi
from deeppowers_amd.params import FheParams, ntt_primes
from test_compact_cpu import WIDTHS, plant_edges, random_words, twin
from test_seeded_cpu import mixed_params
SENTINEL = 0xA5

pytestmark = pytest.mark.gpu


def _device_vs_twin(p: FheParams, batch, bits0, bits1, seed=1):
    import torch
    from deeppowers_amd.evaluator import Context, Evaluator, to_device, to_host
    rng = np.random.default_rng(seed)
    words = random_words(rng, p, batch)
    plant_edges(p, words, bits0, bits1)
    want = twin(p, words, bits0, bits1)
    ctx = Context(p, 0)
    try:
        ev = Evaluator(ctx)
        d_in = to_device(words, ctx.device)
        # the Python mirror
        got = ev.compact(d_in, bits0, bits1)
        # the C ABI into a sentinel-filled buffer with a tail of 4 KiB after the records
        out = torch.full((want.size + 4096,), SENTINEL, dtype=torch.uint8, device=ctx.device)
        _cabi.check(ctx._lib.dpfhe_compact(ctx.handle, out.data_ptr(), d_in.data_ptr(), batch, bits0, bits1, None), "dpfhe_compact")
        torch.cuda.synchronize()
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy(), want), (p.log2_n, p.moduli, batch, bits0, bits1)
        host = out.cpu().numpy()
        assert np.array_equal(host[: want.size], want.reshape(-1))
        assert (host[want.size :] == SENTINEL).all()                       # nothing written past the records
        assert np.array_equal(to_host(d_in), words)                          # the input is untouched
    finally:
        ctx.close()


@pytest.mark.parametrize("log2n", range(8, 17))
def test_device_matches_host_twin_every_ring_degree(log2n):
    p = ntt_primes(log2n, 3, 60)
    _device_vs_twin(p, 3, 19, 28)
    _device_vs_twin(p, 1, 13, 41, seed=2)


@pytest.mark.parametrize("L", [1, 2, 4, 6, 10])
@pytest.mark.parametrize("bits", WIDTHS)
def test_device_matches_host_twin_limb_counts(L, bits):
    _device_vs_twin(ntt_primes(12, L, 60), 5, *bits, seed=L)


@pytest.mark.parametrize("name", ["f64", "f64_wide", "fold_scaled", "shoup", "mixed", "config1"])
def test_device_matches_host_twin_limb_classes(name):
    from test_plain_add_cpu import shoup55
    p = {"f64": lambda: ntt_primes(12, 4, 40), "f64_wide": lambda: ntt_primes(12, 4, 49), "fold_scaled": lambda: ntt_primes(12, 4, 59),
         "shoup": lambda: shoup55(12, 4), "mixed": lambda: mixed_params(12), "config1": FheParams.config1}[name]()
    for i, (b0, b1) in enumerate(WIDTHS):
        _device_vs_twin(p, 3, b0, b1, seed=20 + i)


@pytest.mark.parametrize("kind,log2n", [(k, ln) for k in ("mixed", "smallest") for ln in (12, 13)])
def test_device_matches_host_twin_at_the_catalogue_extremes(kind, log2n):
    """the all-class edge mixture (tests/class_edges.py: one edge prime of every class and the smallest prime) and a context of smallest primes only
    (Q below 2^52, narrower than the widest record), with the rounding boundaries planted"""
    from class_edges import edge_moduli
    p = edge_moduli(kind, log2n)
    for i, (b0, b1) in enumerate(WIDTHS):
        _device_vs_twin(p, 3, b0, b1, seed=40 + i)


def test_device_entry_rejects_bad_arguments():
    import torch
    from deeppowers_amd.evaluator import Context, Evaluator
    p = FheParams.n4096_l4()
    ctx = Context(p, 0)
    try:
        ev = Evaluator(ctx)
        lib = ctx._lib
        ct = torch.zeros((4, 2, p.n_limbs, p.n), dtype=torch.int64, device=ctx.device)
        out = torch.full((4 * p.n * 60 // 8 + 64,), SENTINEL, dtype=torch.uint8, device=ctx.device)
        c, o = ct.data_ptr(), out.data_ptr()
        assert lib.dpfhe_compact(None, o, c, 4, 19, 28, None) == 2000
        for args in ((None, c, 4, 19, 28), (o, None, 4, 19, 28), (o, c, 0, 19, 28), (o, c, 4, 7, 28), (o, c, 4, 19, 61), (o + 8, c, 4, 19, 28),
                     (o, c + 8, 4, 19, 28), (c + 64, c, 4, 19, 28)):
            assert lib.dpfhe_compact(ctx.handle, *args, None) == 2000, args
        with pytest.raises(_cabi.DpfheError):
            ev.compact(ct[:, :1].contiguous(), 19, 28)
        with pytest.raises(_cabi.DpfheError):
            ev.compact(ct, 19, 64)
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == SENTINEL).all() and int(ct.abs().sum()) == 0
    finally:
        ctx.close()
    # eleven limbs: rescale first
    p11 = ntt_primes(8, 11, 60)
    ctx = Context(p11, 0)
    try:
        ct = torch.zeros((1, 2, 11, p11.n), dtype=torch.int64, device=ctx.device)
        out = torch.zeros((p11.n * 60 // 8,), dtype=torch.uint8, device=ctx.device)
        assert ctx._lib.dpfhe_compact(ctx.handle, out.data_ptr(), ct.data_ptr(), 1, 19, 28, None) == 2000
    finally:
        ctx.close()


def test_cpp_compact_facade():
    exe = cpp_build.build_program("test_compact_api")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=1500)
    print(out.stdout)
    assert out.returncode == 0 and "compact C++ facade OK" in out.stdout, out.stdout + out.stderr
