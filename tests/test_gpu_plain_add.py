"""-m gpu: exact plaintext addition on the device (include/dpfhe.h dpfhe_add_plain_scaled, csrc/k_plain_add.hip).

The kernel must give the host twin's words (tests/test_plain_add_cpu.py holds the host twin to the definition) on every ring degree and limb
class, in place and out of place, with components >= 1 untouched or copied.  Through the C++ facade (tests/cpp/test_affine_api.cpp): decryption
of ciphertexts plus plaintexts, 3-component products plus plaintexts, biased PackedLinear layers, the biased transformer block and the activated
FFN with biases."""
import subprocess

import numpy as np
import pytest

import cpp_build
from deeppowers_amd import _cabi
from deeppowers_amd.params import FheParams, ntt_primes
from test_plain_add_cpu import PARAMS, T_PRIME_BIG, T_VALUES, random_ct, random_plain, twin
from test_seeded_cpu import SENTINEL

pytestmark = pytest.mark.gpu


def _device_vs_twin(p: FheParams, batch, comps, items, t, negate, seed=1):
    import torch
    from deeppowers_amd.evaluator import Context, Evaluator, to_device, to_host
    rng = np.random.default_rng(seed)
    ct = random_ct(rng, p, batch, comps)
    plain = random_plain(rng, items, p.n, t)
    want = twin(p, ct, plain, t, negate)
    ctx = Context(p, 0)
    try:
        ev = Evaluator(ctx)
        d_ct, d_plain = to_device(ct, ctx.device), to_device(plain, ctx.device)
        # in place (the Python mirror)
        ev.add_plain_scaled_(d_ct, d_plain, t, negate)
        # out of place into a sentinel-filled buffer: component 0 computed, the others copied
        d_in = to_device(ct, ctx.device)
        d_out = torch.full_like(d_in, int(SENTINEL.view(np.int64)))
        _cabi.check(ctx._lib.dpfhe_add_plain_scaled(ctx.handle, d_out.data_ptr(), d_in.data_ptr(), d_plain.data_ptr(), batch, comps, items, t,
                                                    1 if negate else 0, None), "dpfhe_add_plain_scaled")
        torch.cuda.synchronize()
        got_ip, got_oop = to_host(d_ct), to_host(d_out)
        assert np.array_equal(got_ip, want), (p.log2_n, p.moduli, batch, comps, items, t, negate)
        assert np.array_equal(got_oop, want)
        assert np.array_equal(to_host(d_in), ct)                           # the input of the out-of-place call is untouched
    finally:
        ctx.close()


@pytest.mark.parametrize("log2n", range(8, 17))
def test_device_matches_host_twin_every_ring_degree(log2n):
    p = ntt_primes(log2n, 3 if log2n <= 14 else 2, 60)
    _device_vs_twin(p, 3, 2, 1, 65537, False)
    _device_vs_twin(p, 4, 3, 2, T_PRIME_BIG, True, seed=2)


@pytest.mark.parametrize("name", list(PARAMS) + ["config1", "limbs40"])
def test_device_matches_host_twin_limb_classes(name):
    p = {"config1": FheParams.config1, "limbs40": lambda: ntt_primes(10, 40, 31)}.get(name, PARAMS.get(name))()
    for i, t in enumerate(T_VALUES):
        _device_vs_twin(p, 6, 2 + i % 2, (1, 6, 3)[i], t, bool(i % 2), seed=10 + i)


def _device_and_twin_refuse(p: FheParams, t):
    """t shares a factor with a modulus: the host twin and the device entry both refuse (DPFHE_INVALID_ARGUMENT) and the ciphertext keeps its words"""
    from deeppowers_amd.evaluator import Context, Evaluator, to_device, to_host
    rng = np.random.default_rng(t)
    ct, plain = random_ct(rng, p, 2, 2), random_plain(rng, 1, p.n, t)
    with pytest.raises(_cabi.DpfheError) as e:
        twin(p, ct, plain, t)
    assert e.value.code == 2000
    ctx = Context(p, 0)
    try:
        d_ct, d_plain = to_device(ct, ctx.device), to_device(plain, ctx.device)
        assert ctx._lib.dpfhe_add_plain_scaled(ctx.handle, d_ct.data_ptr(), d_ct.data_ptr(), d_plain.data_ptr(), 2, 2, 1, t, 0, None) == 2000
        with pytest.raises(_cabi.DpfheError):
            Evaluator(ctx).add_plain_scaled_(d_ct, d_plain, t)
        assert np.array_equal(to_host(d_ct), ct)
    finally:
        ctx.close()


@pytest.mark.parametrize("kind,log2n", [(k, ln) for k in ("mixed", "smallest") for ln in (12, 13)])
def test_device_matches_host_twin_at_the_catalogue_extremes(kind, log2n):
    """the all-class edge mixture (tests/class_edges.py) and a context of smallest primes only (every q far below 2^32), with t just below 2^32 and
    t = 65537.  At N = 8192 the smallest prime = 1 mod 2N is 65537 itself and the mixture holds it as a limb: there t = 65537 must be refused by the
    twin and by the device, and the neighbouring 65539 is added instead."""
    from class_edges import edge_moduli
    p = edge_moduli(kind, log2n)
    assert (65537 in p.moduli) == (kind == "mixed" and log2n == 13)
    for i, t in enumerate((T_PRIME_BIG, 65537)):
        assert t > (1 << 32) - (1 << 20) or t == 65537
        if t in p.moduli:
            _device_and_twin_refuse(p, t)
            t = 65539
        assert all(t % q for q in p.moduli)
        _device_vs_twin(p, 4, 2 + i, (1, 2)[i], t, bool(i), seed=30 + i)


def test_full_size_in_place():
    """8192 items x N = 4096 x L = 4, broadcast plaintext, in place: the first and last 64 items and three zero items in between == host twin"""
    import torch
    from deeppowers_amd.evaluator import Context, Evaluator, to_device, to_host
    p = FheParams.n4096_l4()
    rng = np.random.default_rng(3)
    ctx = Context(p, 0)
    try:
        ev = Evaluator(ctx)
        head = random_ct(rng, p, 64, 2)
        d = torch.zeros((8192, 2, p.n_limbs, p.n), dtype=torch.int64, device=ctx.device)
        d[:64] = to_device(head, ctx.device)
        d[-64:] = to_device(head, ctx.device)
        plain = random_plain(rng, 1, p.n, 65537)
        ev.add_plain_scaled_(d, to_device(plain, ctx.device), 65537)
        torch.cuda.synchronize()
        want = twin(p, head, plain, 65537)
        assert np.array_equal(to_host(d[:64]), want) and np.array_equal(to_host(d[-64:]), want)
        assert int(d[64:-64, 1].abs().sum()) == 0                          # component 1 of the zero items stays zero
        zero = twin(p, np.zeros((1, 2, p.n_limbs, p.n), dtype=np.uint64), plain, 65537)
        assert all(np.array_equal(to_host(d[i:i + 1]), zero) for i in (64, 4095, 8192 - 65))
        del d
    finally:
        ctx.close()


def test_device_entry_rejects_bad_arguments():
    import torch
    from deeppowers_amd.evaluator import Context, Evaluator
    p = FheParams.n4096_l4()
    ctx = Context(p, 0)
    try:
        ev = Evaluator(ctx)
        lib = ctx._lib
        ct = torch.zeros((4, 2, p.n_limbs, p.n), dtype=torch.int64, device=ctx.device)
        pl = torch.ones((2, p.n), dtype=torch.int64, device=ctx.device)
        c, q = ct.data_ptr(), pl.data_ptr()
        assert lib.dpfhe_add_plain_scaled(None, c, c, q, 4, 2, 2, 65537, 0, None) == 2000
        for args in ((None, c, q, 4, 2, 2, 65537), (c, None, q, 4, 2, 2, 65537), (c, c, None, 4, 2, 2, 65537), (c, c, q, 4, 1, 2, 65537),
                     (c, c, q, 4, 4, 2, 65537), (c, c, q, 3, 2, 2, 65537), (c, c, q, 4, 2, 0, 65537), (c, c, q, 4, 2, 2, 65536),
                     (c, c, q, 4, 2, 2, 1), (c, c, q, 4, 2, 2, (1 << 32) + 1), (c + 8, c + 8, q, 4, 2, 2, 65537)):
            assert lib.dpfhe_add_plain_scaled(ctx.handle, *args, 0, None) == 2000, args
        with pytest.raises(_cabi.DpfheError):
            ev.add_plain_scaled_(ct, pl[:, :16].contiguous(), 65537)
        torch.cuda.synchronize()
        assert int(ct.abs().sum()) == 0
    finally:
        ctx.close()
    # t sharing a factor with a modulus
    p31 = ntt_primes(8, 2, 31)
    ctx = Context(p31, 0)
    try:
        ct = torch.zeros((1, 2, 2, p31.n), dtype=torch.int64, device=ctx.device)
        pl = torch.zeros((1, p31.n), dtype=torch.int64, device=ctx.device)
        assert ctx._lib.dpfhe_add_plain_scaled(ctx.handle, ct.data_ptr(), ct.data_ptr(), pl.data_ptr(), 1, 2, 1, p31.moduli[0], 0, None) == 2000
    finally:
        ctx.close()


def test_cpp_affine_facade():
    exe = cpp_build.build_program("test_affine_api")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=1500)
    print(out.stdout)
    assert out.returncode == 0 and "affine C++ facade OK" in out.stdout, out.stdout + out.stderr
