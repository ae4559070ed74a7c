"""-m gpu: slot encoding on the device (include/dpfhe.h dpfhe_encode_slots, csrc/k_encode.hip).

The kernels must give the host twin's words (tests/test_encode_cpu.py holds the host twin to the definition) at every ring degree, for the
smallest usable t, 65537 and a t just under 2^32, in the plain, residue and transformed forms and on every limb class; at full size (the 1024
diagonals of a 768 -> 3072 layer at N = 8192 over six limbs) every word is compared, and a call on a second stream leaves the words past its
output alone.  Through the C++ facade (tests/cpp/test_encode_api.cpp): BatchEncoder::encode_device equals encode + lift + upload word for word
on the data and the extended context, and device-encoded operands multiply and add correctly under encryption."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import cpp_build
from deeppowers_amd import _cabi
from deeppowers_amd.params import FheParams, min_primitive_2n_root, ntt_primes
from encode_ref import extreme_slot_vectors, largest_t, slot_vectors, t_values, twin, zeta_of
from test_plain_add_cpu import PARAMS, big_prime_t
from test_seeded_cpu import SENTINEL
T_BIG = big_prime_t()

pytestmark = pytest.mark.gpu


def _to_dev32(slots, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(slots, dtype=np.uint32).view(np.int32)).to(device)


def _device_vs_twin(p: FheParams, t, seed, slots=None, orc=None):
    """slots: the vectors to encode (default: slot_vectors); orc: also hold the transformed output to this oracle's forward transform of the residues"""
    import torch
    from deeppowers_amd.evaluator import Context, Evaluator, to_host
    if slots is None:
        slots = slot_vectors(np.random.default_rng(seed), p.n, t)
    want_plain, want_res = twin(p.moduli, p.log2_n, t, slots, plain=True), twin(p.moduli, p.log2_n, t, slots)
    ctx = Context(p, 0)
    try:
        ev = Evaluator(ctx)
        assert ctx._lib.dpfhe_encoder_root(ctx.encoder(t)) == zeta_of(p.log2_n, t)
        d_slots = _to_dev32(slots, ctx.device)
        got_plain = ev.encode_slots(d_slots, t, plain=True)
        got_res = ev.encode_slots(d_slots, t)
        got_ntt = ev.encode_slots(d_slots, t, to_ntt=True)
        from_i64 = ev.encode_slots(d_slots.to(torch.int64) & 0xFFFFFFFF, t)
        fwd = got_res.clone()
        _cabi.check(ctx._lib.dpfhe_ntt_fwd(ctx.handle, fwd.data_ptr(), fwd.shape[0], None), "dpfhe_ntt_fwd")
        torch.cuda.synchronize()
        assert np.array_equal(to_host(got_plain), want_plain), (p.log2_n, t, "plain")
        assert np.array_equal(to_host(got_res), want_res), (p.log2_n, t, "residues")
        assert np.array_equal(to_host(from_i64), want_res)
        assert torch.equal(got_ntt, fwd), (p.log2_n, t, "ntt")
        if orc is not None:
            assert np.array_equal(to_host(got_ntt), orc.ntt_fwd(want_res, threads=0)), (p.log2_n, t, "ntt against the oracle")
        assert np.array_equal(to_host(d_slots).view(np.uint32).reshape(slots.shape), slots)      # the input is untouched
    finally:
        ctx.close()


@pytest.mark.parametrize("log2n", range(8, 17))
def test_device_matches_host_twin_every_ring_degree(log2n):
    p = ntt_primes(log2n, 3 if log2n <= 14 else 2, 60)
    for i, t in enumerate(t_values(log2n, T_BIG)):
        _device_vs_twin(p, t, seed=100 * log2n + i)


@pytest.mark.parametrize("name", list(PARAMS) + ["config1", "limbs40", "below_t"])
def test_device_matches_host_twin_limb_classes(name):
    if name == "below_t":
        p = FheParams(8, (7681, 12289), (min_primitive_2n_root(256, 7681), min_primitive_2n_root(256, 12289)))   # every limb below t
        ts = (T_BIG,)
    else:
        p = {"config1": FheParams.config1, "limbs40": lambda: ntt_primes(10, 40, 31)}.get(name, PARAMS.get(name))()
        ts = (65537, T_BIG)
    for i, t in enumerate(ts):
        _device_vs_twin(p, t, seed=7 + i)


@pytest.mark.parametrize("kind,log2n", [(k, ln) for k in ("mixed", "smallest") for ln in (12, 13)])
def test_device_matches_host_twin_at_the_catalogue_extremes(kind, log2n):
    """the all-class edge mixture (tests/class_edges.py) and a context of smallest primes only (every q far below t), t the largest prime below 2^32
    that is 1 mod 2N, slots at 0, t - 1, (t - 1) / 2 and (t + 1) / 2 (the sign change of the centred lift): plain, residue and transformed output, the
    last also against the oracle's forward transform of the twin's residues"""
    from class_edges import edge_moduli
    from oracle.cbind import Oracle
    p = edge_moduli(kind, log2n)
    t = largest_t(log2n)
    assert t > (1 << 32) - (1 << 20) and (t - 1) % (2 * p.n) == 0
    _device_vs_twin(p, t, seed=log2n, slots=extreme_slot_vectors(np.random.default_rng(log2n), p.n, t), orc=Oracle.from_params(p))


def test_full_size_layer_and_second_stream():
    """1024 slot vectors (the diagonals of 768 -> 3072) at N = 8192 over six limbs, 403 MB out in one call: every word against the twin; then 64 of
    them on a non-default stream into the middle of a sentinel-filled buffer"""
    import torch
    from deeppowers_amd.evaluator import Context, Evaluator, to_host
    p = FheParams.n8192_l6()
    t, items = 65537, 1024
    rng = np.random.default_rng(768 * 3072)
    slots = rng.integers(0, t, (items, p.n), dtype=np.uint64).astype(np.uint32)
    slots[::7] &= 0xFF                                   # quantised weights among them
    want = twin(p.moduli, p.log2_n, t, slots)
    ctx = Context(p, 0)
    try:
        ev = Evaluator(ctx)
        d_slots = _to_dev32(slots, ctx.device)
        got = ev.encode_slots(d_slots, t)
        torch.cuda.synchronize()
        assert got.shape == (items, 6, p.n) and got.numel() * 8 == 402653184
        assert np.array_equal(to_host(got), want)
        del got
        side = torch.cuda.Stream(device=ctx.device)
        per = 6 * p.n
        buf = torch.full((66 * per,), int(SENTINEL.view(np.int64)), dtype=torch.int64, device=ctx.device)
        torch.cuda.synchronize()
        _cabi.check(ctx._lib.dpfhe_encode_slots(ctx.encoder(t), buf.data_ptr() + 8 * per, d_slots.data_ptr(), 64, 0, C.c_void_p(side.cuda_stream)),
                    "dpfhe_encode_slots")
        side.synchronize()
        h = to_host(buf)
        assert (h[:per] == SENTINEL).all() and (h[65 * per:] == SENTINEL).all()      # the words before and just past the end
        assert np.array_equal(h[per:65 * per].reshape(64, 6, p.n), want[:64])
    finally:
        ctx.close()


def test_device_entry_rejects_bad_arguments():
    import torch
    from deeppowers_amd.evaluator import Context, Evaluator
    p = FheParams.n4096_l4()
    ctx = Context(p, 0)
    try:
        lib = ctx._lib
        enc = C.c_void_p()
        for t in (65536, 8193 * 3, (1 << 32) + 8192 * 3 + 1, 12289, 0):        # even, composite, >= 2^32, prime but not 1 mod 2N, zero
            assert lib.dpfhe_encoder_create(C.byref(enc), ctx.handle, t) == 2000 and not enc.value, t
        e = ctx.encoder(65537)
        out = torch.zeros((2, p.n_limbs, p.n), dtype=torch.int64, device=ctx.device)
        sl = torch.ones((2, p.n), dtype=torch.int32, device=ctx.device)
        o, s = out.data_ptr(), sl.data_ptr()
        for args in ((None, o, s, 2, 0), (e, None, s, 2, 0), (e, o, None, 2, 0), (e, o, s, 0, 0), (e, o, s, 2, 3), (e, o, s, 2, 4), (e, o + 8, s, 2, 0),
                     (e, o, s + 4, 2, 0), (e, o, o, 2, 0), (e, o, s, 1 << 20, 0)):
            assert lib.dpfhe_encode_slots(*args, None) == 2000, args
        torch.cuda.synchronize()
        assert int(out.abs().sum()) == 0
        with pytest.raises(_cabi.DpfheError):
            Evaluator(ctx).encode_slots(sl[:, :16].contiguous(), 65537)
        # a slot value >= t is reduced, never a fault
        big = torch.full((1, p.n), 65537 + 5, dtype=torch.int32, device=ctx.device)
        five = torch.full((1, p.n), 5, dtype=torch.int32, device=ctx.device)
        ev = Evaluator(ctx)
        assert torch.equal(ev.encode_slots(big, 65537, plain=True), ev.encode_slots(five, 65537, plain=True))
    finally:
        ctx.close()


def test_cpp_encode_facade():
    exe = cpp_build.build_program("test_encode_api")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=1500)
    print(out.stdout)
    assert out.returncode == 0 and "encode C++ facade OK" in out.stdout, out.stdout + out.stderr
