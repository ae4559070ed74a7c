"""-m gpu: noise polynomials and re-randomisation on the device (include/dpfhe.h dpfhe_sample_noise, dpfhe_rerandomize; csrc/k_noise.hip).

The sampler must give the host twin's words (tests/test_rerandomize_cpu.py holds the host twin to the definition) on every ring degree, limb count
and limb class, for odd batches, with and without DPFHE_NOISE_ADD, without touching another component or a word past the buffer.
dpfhe_rerandomize must equal its definition composed from the host twin and the CPU oracle's transforms and products.  Through the C++ facade
(tests/cpp/test_rerandomize_api.cpp): message kept, c1 replaced, the derived budget, a biased 768 x 768 PackedLinear re-randomised and compacted."""
import subprocess

import numpy as np
import pytest

import cpp_build
from deeppowers_amd import _cabi, wire
from deeppowers_amd.params import FheParams, ntt_primes
from test_rerandomize_cpu import CBD21, FLOOD, FLOOD_BITS, TERNARY
from test_seeded_cpu import SEED, mixed_params
SENTINEL = 0x5A5A5A5A5A5A5A5A
TAIL = 512

pytestmark = pytest.mark.gpu


def _random_words(rng, p: FheParams, batch, comps):
    q = np.array(p.moduli, dtype=np.uint64)[None, None, :, None]
    return (rng.integers(0, 1 << 63, (batch, comps, p.n_limbs, p.n), dtype=np.uint64) % q).astype(np.uint64)


def _device_vs_twin(ctx, p: FheParams, cases, seed=SEED):
    """cases: (batch, comps, comp, kind, param, stream_id, first_item, add); one context serves all of them"""
    import torch
    from deeppowers_amd.evaluator import to_device
    rng = np.random.default_rng(p.log2_n * 100 + p.n_limbs)
    for batch, comps, comp, kind, param, stream_id, first_item, add in cases:
        start = _random_words(rng, p, batch, comps)
        if add and batch > 1:
            start[-1] = (np.array(p.moduli, dtype=np.uint64) - np.uint64(1))[None, :, None]      # q - 1 everywhere in the last item
        want = wire.noise_host(p, batch, comps, comp, kind, param, stream_id, seed, first_item, add=add, out=start.copy())
        buf = torch.full((start.size + TAIL,), SENTINEL, dtype=torch.int64, device=ctx.device)
        buf[: start.size] = to_device(start, ctx.device).reshape(-1)
        _cabi.check(ctx._lib.dpfhe_sample_noise(ctx.handle, buf.data_ptr(), batch, comps, comp, kind, param, stream_id, seed, first_item,
                                                _cabi.NOISE_ADD if add else 0, None), "dpfhe_sample_noise")
        torch.cuda.synchronize()
        host = buf.cpu().numpy().view(np.uint64)
        got = host[: start.size].reshape(start.shape)
        what = (p.log2_n, p.moduli, batch, comps, comp, kind, param, first_item, add)
        assert np.array_equal(got[:, comp], want[:, comp]), what
        others = [c for c in range(comps) if c != comp]
        assert np.array_equal(got[:, others], start[:, others]), what       # other components untouched
        assert (host[start.size:] == np.uint64(SENTINEL)).all(), what       # nothing written past the buffer


def _all_kinds(batch, first_item):
    cases = []
    for add in (False, True):
        cases.append((batch, 2, 1, TERNARY, 0, 0, first_item, add))
        cases.append((batch, 3, 0, CBD21, 0, 1, first_item, add))
        for i, f in enumerate(FLOOD_BITS):
            cases.append((batch, 2 + i % 2, i % 2, FLOOD, f, 2, first_item, add))
    return cases


def _with_ctx(p, fn):
    from deeppowers_amd.evaluator import Context
    ctx = Context(p, 0)
    try:
        return fn(ctx)
    finally:
        ctx.close()


# ---- 6: device sampler == host twin ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2n", range(8, 17))
def test_device_matches_host_twin_every_ring_degree(log2n):
    p = ntt_primes(log2n, 2, 60)
    _with_ctx(p, lambda ctx: _device_vs_twin(ctx, p, _all_kinds(3 if log2n <= 13 else 1, (1 << 31) + 5 if log2n % 2 else 0)))


@pytest.mark.parametrize("L", [1, 2, 4, 6, 10])
def test_device_matches_host_twin_limb_counts(L):
    p = ntt_primes(12, L, 60)
    _with_ctx(p, lambda ctx: _device_vs_twin(ctx, p, _all_kinds(5, 7 * L)))


@pytest.mark.parametrize("name", ["f64", "f64_wide", "fold_scaled", "shoup", "mixed", "config1"])
def test_device_matches_host_twin_limb_classes(name):
    from test_plain_add_cpu import shoup55
    p = {"f64": lambda: ntt_primes(12, 4, 40), "f64_wide": lambda: ntt_primes(12, 4, 49), "fold_scaled": lambda: ntt_primes(12, 4, 59),
         "shoup": lambda: shoup55(12, 4), "mixed": lambda: mixed_params(12), "config1": FheParams.config1}[name]()
    _with_ctx(p, lambda ctx: _device_vs_twin(ctx, p, _all_kinds(3, 0)))


@pytest.mark.parametrize("kind,log2n", [(k, ln) for k in ("mixed", "smallest") for ln in (12, 13)])
def test_device_matches_host_twin_at_the_catalogue_extremes(kind, log2n):
    """the all-class edge mixture (tests/class_edges.py) and a context of smallest primes only (every q below 2^18, far below a flood value): ternary,
    centred binomial, and flood at 1, 64 and 250 bits, set and added (q - 1 in every word of the last item)"""
    from class_edges import edge_moduli
    p = edge_moduli(kind, log2n)
    cases = []
    for add in (False, True):
        cases.append((3, 2, 1, TERNARY, 0, 0, 5, add))
        cases.append((3, 3, 0, CBD21, 0, 1, 5, add))
        for i, f in enumerate((1, 64, 250)):
            cases.append((3, 2 + i % 2, i % 2, FLOOD, f, 2, 5, add))
    _with_ctx(p, lambda ctx: _device_vs_twin(ctx, p, cases))


def test_more_limbs_than_one_launch_group():
    p = ntt_primes(8, 19, 60)
    _with_ctx(p, lambda ctx: _device_vs_twin(ctx, p, [(3, 2, 1, FLOOD, 200, 2, 3, False), (3, 2, 0, CBD21, 0, 1, 0, True), (1, 1, 0, TERNARY, 0, 0, 9, False)]))


# ---- 7: dpfhe_rerandomize == its definition ----------------------------------------------------------------------------------------
def _rerandomize_ref(p: FheParams, ct, pk, flood_bits, seed, first_item):
    """the composition of include/dpfhe.h from the host twin and the CPU oracle's transforms and products"""
    from oracle.cbind import Oracle
    orc = Oracle.from_params(p)
    batch = ct.shape[0]
    u = wire.noise_host(p, batch, 1, 0, TERNARY, 0, 0, seed, first_item)[:, 0]                # [batch][L][N]
    u_hat = orc.ntt_fwd(np.ascontiguousarray(u))
    out = ct.copy()
    q = np.array(p.moduli, dtype=np.uint64)[None, :, None]
    for c in range(2):
        pkc = np.ascontiguousarray(np.broadcast_to(pk[c][None], u_hat.shape))
        prod = orc.ntt_inv(orc.dyadic("mul", u_hat, pkc))
        out[:, c] = (out[:, c] + prod) % q
    wire.noise_host(p, batch, 2, 0, FLOOD, flood_bits, 2, seed, first_item, add=True, out=out)
    wire.noise_host(p, batch, 2, 1, CBD21, 0, 1, seed, first_item, add=True, out=out)
    return out


@pytest.mark.parametrize("log2n", [8, 12, 13, 14, 16])
@pytest.mark.parametrize("name", ["pinned60", "mixed", "primes31"])
def test_rerandomize_equals_its_definition(name, log2n):
    p = {"pinned60": lambda: ntt_primes(log2n, 4, 60), "mixed": lambda: mixed_params(log2n), "primes31": lambda: ntt_primes(log2n, 3, 31)}[name]()
    _rerandomize_vs_definition(p, {"pinned60": 200, "mixed": 130, "primes31": 64}[name], (name, log2n))


@pytest.mark.parametrize("kind,log2n", [(k, ln) for k in ("mixed", "smallest") for ln in (12, 13)])
def test_rerandomize_equals_its_definition_at_the_catalogue_extremes(kind, log2n):
    """the all-class edge mixture (tests/class_edges.py) with the widest flood, 250 bits, and a context of smallest primes only with the widest flood
    its Q admits (floor(log2 Q) - 3 bits, far above every q): the ciphertext and the key carry q - 1 in every word of one item / component"""
    import math
    from class_edges import edge_moduli
    p = edge_moduli(kind, log2n)
    flood_bits = min(250, math.prod(p.moduli).bit_length() - 1 - 3)
    assert flood_bits == 250 or (kind == "smallest" and flood_bits > 40)
    _rerandomize_vs_definition(p, flood_bits, (kind, log2n), extreme=True)


def _rerandomize_vs_definition(p, flood_bits, what, extreme=False):
    import torch
    from deeppowers_amd.evaluator import Evaluator, to_device, to_host
    name, log2n = what
    batch, first_item = 3, 11
    rng = np.random.default_rng(log2n)
    ct = _random_words(rng, p, batch, 2)
    pk = _random_words(rng, p, 1, 2)[0]
    if extreme:
        ct[1] = pk[1] = (np.array(p.moduli, dtype=np.uint64) - np.uint64(1))[:, None]
    want = _rerandomize_ref(p, ct, pk, flood_bits, SEED, first_item)

    def run(ctx):
        d_ct, d_pk = to_device(ct, ctx.device), to_device(pk, ctx.device)
        words = 3 * batch * p.n_limbs * p.n
        work = torch.full((words + TAIL,), SENTINEL, dtype=torch.int64, device=ctx.device)
        _cabi.check(ctx._lib.dpfhe_rerandomize(ctx.handle, d_ct.data_ptr(), d_pk.data_ptr(), batch, flood_bits, SEED, first_item, work.data_ptr(), None),
                    "dpfhe_rerandomize")
        torch.cuda.synchronize()
        assert np.array_equal(to_host(d_ct), want), (name, log2n)
        assert (work[words:].cpu().numpy().view(np.uint64) == np.uint64(SENTINEL)).all()         # the work buffer is 3 batch L N words, no more
        assert np.array_equal(to_host(d_pk), pk)
        # 9: the Python mirror gives the C ABI's words
        d2 = to_device(ct, ctx.device)
        Evaluator(ctx).rerandomize_(d2, d_pk, flood_bits, SEED, first_item)
        torch.cuda.synchronize()
        assert np.array_equal(to_host(d2), want)
    _with_ctx(p, run)


def test_python_mirror_sample_noise():
    import torch
    from deeppowers_amd.evaluator import Evaluator, to_device, to_host
    p = FheParams.n4096_l4()

    def run(ctx):
        ev = Evaluator(ctx)
        start = _random_words(np.random.default_rng(5), p, 3, 2)
        t = to_device(start, ctx.device)
        ev.sample_noise_(t, _cabi.NOISE_FLOOD, 100, 2, SEED, 0, first_item=4)
        ev.sample_noise_(t, _cabi.NOISE_CBD21, 0, 1, SEED, 1, first_item=4, add=True)
        torch.cuda.synchronize()
        want = wire.noise_host(p, 3, 2, 0, FLOOD, 100, 2, SEED, 4, out=start.copy())
        wire.noise_host(p, 3, 2, 1, CBD21, 0, 1, SEED, 4, add=True, out=want)
        assert np.array_equal(to_host(t), want)
        with pytest.raises(_cabi.DpfheError):
            ev.sample_noise_(t, 3, 0, 0, SEED, 0)
        with pytest.raises(_cabi.DpfheError):
            ev.sample_noise_(t, _cabi.NOISE_FLOOD, 251, 0, SEED, 0)
        with pytest.raises(_cabi.DpfheError):
            ev.sample_noise_(t, _cabi.NOISE_TERNARY, 0, 0, b"short", 0)
    _with_ctx(p, run)


# ---- 5, device side: the entries refuse bad arguments and write nothing ---------------------------------------------------------------
def test_device_entries_reject_bad_arguments():
    import torch
    p = FheParams.n4096_l4()                                                # floor(log2 Q) = 239

    def run(ctx):
        lib, h = ctx._lib, ctx.handle
        poly = p.n_limbs * p.n
        ct = torch.full((2 * 2 * poly,), SENTINEL, dtype=torch.int64, device=ctx.device)
        pk = torch.full((2 * poly,), SENTINEL, dtype=torch.int64, device=ctx.device)
        work = torch.full((3 * 2 * poly,), SENTINEL, dtype=torch.int64, device=ctx.device)
        c, k, w = ct.data_ptr(), pk.data_ptr(), work.data_ptr()
        ok = (c, 2, 2, 1, FLOOD, 20, 0, SEED, 0, 0)
        assert lib.dpfhe_sample_noise(None, *ok, None) == 2000
        for why, args in {"null buffer": (None,) + ok[1:], "batch 0": ok[:1] + (0,) + ok[2:], "comp >= comps": ok[:3] + (2,) + ok[4:],
                          "kind 3": ok[:4] + (3,) + ok[5:], "f 0": ok[:5] + (0,) + ok[6:], "f 251": ok[:5] + (251,) + ok[6:],
                          "null seed": ok[:7] + (None,) + ok[8:], "first_item + batch": ok[:8] + (0xFFFFFFFF,) + ok[9:],
                          "unknown flag": ok[:9] + (2,), "misaligned": (c + 8,) + ok[1:]}.items():
            assert lib.dpfhe_sample_noise(h, *args, None) == 2000, why
        okr = (c, k, 2, 100, SEED, 0, w)
        assert lib.dpfhe_rerandomize(None, *okr, None) == 2000
        for why, args in {"null ct": (None,) + okr[1:], "null pk": okr[:1] + (None,) + okr[2:], "batch 0": okr[:2] + (0,) + okr[3:],
                          "flood_bits 0": okr[:3] + (0,) + okr[4:], "flood_bits > floor(log2 Q) - 3": okr[:3] + (237,) + okr[4:],
                          "null seed": okr[:4] + (None,) + okr[5:], "first_item + batch": okr[:5] + (0xFFFFFFFF,) + okr[6:],
                          "null work": okr[:6] + (None,), "misaligned ct": (c + 8,) + okr[1:], "misaligned pk": okr[:1] + (k + 8,) + okr[2:],
                          "misaligned work": okr[:6] + (w + 8,), "work overlaps the ciphertexts": okr[:6] + (c + 64,),
                          "work overlaps the key": okr[:6] + (k,), "key inside the ciphertexts": okr[:1] + (c + 16,) + okr[2:]}.items():
            assert lib.dpfhe_rerandomize(h, *args, None) == 2000, why
        torch.cuda.synchronize()
        for t in (ct, pk, work):
            assert bool((t == SENTINEL).all())
    _with_ctx(p, run)


# ---- 8: the C++ facade -------------------------------------------------------------------------------------------------------------
def test_cpp_rerandomize_facade():
    exe = cpp_build.build_program("test_rerandomize_api")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    print(out.stdout)
    assert out.returncode == 0 and "rerandomize C++ facade OK" in out.stdout, out.stdout + out.stderr
