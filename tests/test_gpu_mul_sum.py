"""-m gpu: sums of ciphertext tensor products on the device (include/dpfhe.h dpfhe_ct_mul_sum; csrc/mul_sum.h, tensor3_sum_kernel in csrc/kernels_mul.h), word for
word, on the contexts of tests/test_gpu_fused_rescale.py's rig (the pinned fold primes on 3 and 5 limbs, f64 limbs under a fold prime, generic primes).

* flags 0 against sum_k orc.ct_mul(a_k, b_k) taken mod q_l in Python integers: N = 256 (one partial chunk) and N = 1024, terms in {1, 2, 9, 17}, groups in
  {1, 3}, the second operand per group, shared, and the first operand itself (a sum of squares); one case each at N = 4096 and N = 16384;
* DPFHE_IN_NTT | DPFHE_OUT_NTT - the streaming kernel with no transform in between - against Python integers alone, on the planted columns of
  tests/test_emulated_mul_sum.py (tests/mul_sum_ref.py: the largest products, sums solved to land on 0, 1, q - 1 and either side of q / 2);
* terms = 1 against the device's own dpfhe_ct_mul, and the three-call composition (multiply into the NTT domain, reduce_sum, ntt_inverse) against the entry;
* a scratch limit of 1 MiB at N = 4096, L = 4, terms = 5, groups = 2 (a term's transformed operands are 512 KiB: every group is cut into ranges of 2, 2 and 1
  terms that accumulate) and of 3 MiB (one whole group per slice): the words of the default limit;
* the header's rejections, before the device is touched.
arena_cases() is the footprint case, and - run again by tests/test_gpu_stream_contract_mul_sum.py with Case.gate set - the stream-contract case."""
import numpy as np
import pytest

import fused_rescale_ref as fr
import mul_sum_ref as ms
import test_gpu_footprint as fp
import test_gpu_fused_rescale as fu
from deeppowers_amd import _cabi
from deeppowers_amd.evaluator import Ciphertext, to_host

pytestmark = pytest.mark.gpu

rig = fu.rig
RIGS = ("pinned_ld2", "pinned_ld4", "f64_under_fold", "shoup")
TERMS, GROUPS = (1, 2, 9, 17), (1, 3)
IN_NTT, OUT_NTT = _cabi.IN_NTT, _cabi.OUT_NTT


def sum_mod(r, prods):
    """prods uint64 [G][K][3][L][N] -> sum over K mod q_l, in Python integers -> uint64 [G][3][L][N]"""
    q = np.array([int(v) for v in r.p.moduli], dtype=object)[:, None]
    return (prods.astype(object).sum(axis=1) % q).astype(np.uint64)


def reference(r, a, b):
    """a [G][K][2][L][N], b the same or [1][K][2][L][N] (shared): the oracle's tensor product of every pair, summed in Python integers"""
    G, K = a.shape[:2]
    bb = np.ascontiguousarray(np.broadcast_to(b, a.shape))
    prods = r.orc.ct_mul(np.ascontiguousarray(a).reshape(G * K, 2, r.L, r.n), bb.reshape(G * K, 2, r.L, r.n), threads=0)
    return sum_mod(r, prods.reshape(G, K, 3, r.L, r.n))


def device(r, a, b, shared=False, square=False, in_ntt=False, out_ntt=None):
    import torch
    G, K = a.shape[:2]
    da = Ciphertext(r.dev(a.reshape(G * K, 2, r.L, r.n)), in_ntt)
    db = da if square else Ciphertext(r.dev(b.reshape(-1, 2, r.L, r.n)), in_ntt)
    out = r.ev.multiply_sum(da, db, K, b_shared=shared, out_ntt=out_ntt)
    torch.cuda.synchronize()
    return to_host(out.data)


@pytest.mark.parametrize("log2n", (8, 10))
@pytest.mark.parametrize("name", RIGS)
def test_coefficient_domain_equals_the_oracles_products_summed_in_integers(rig, name, log2n):
    r = rig(name, log2n)
    assert r.ctx.uses_fold == name.startswith("pinned")
    Gm, Km = max(GROUPS), max(TERMS)
    a = r.words(r.orc, (Gm, Km, 2), 500 + log2n)
    b = r.words(r.orc, (Gm, Km, 2), 510 + log2n)
    b[0] = np.roll(b[0], r.n // 16, axis=-1)
    every = lambda x, y: r.orc.ct_mul(np.ascontiguousarray(x).reshape(-1, 2, r.L, r.n), np.ascontiguousarray(np.broadcast_to(y, x.shape)).reshape(-1, 2, r.L, r.n),
                                      threads=0).reshape(Gm, Km, 3, r.L, r.n)
    prods = {"own": every(a, b), "shared": every(a, b[:1]), "square": every(a, a)}     # every pair's product once; the cases below sum slices of them
    for G in GROUPS:
        for K in TERMS:
            ag, bg = np.ascontiguousarray(a[:G, :K]), np.ascontiguousarray(b[:G, :K])
            for form in ("own", "shared", "square"):
                got = device(r, ag, bg[:1] if form == "shared" else bg, shared=form == "shared", square=form == "square")
                want = sum_mod(r, prods[form][:G, :K])
                assert got.shape == want.shape == (G, 3, r.L, r.n)
                assert np.array_equal(got, want), (name, log2n, G, K, form, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("name,log2n", [("pinned_ld4", 12), ("fold_ld2", 14)])
def test_coefficient_domain_at_the_larger_rings(rig, name, log2n):
    r = rig(name, log2n)
    a, b = r.words(r.orc, (1, 3, 2), 520), r.words(r.orc, (1, 3, 2), 530)
    got, want = device(r, a, b), reference(r, a, b)
    assert np.array_equal(got, want), (name, log2n, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("name", RIGS)
def test_ntt_domain_equals_python_integers_on_the_planted_columns(rig, name):
    """no transform on either side: the streaming kernel alone.  Group 1 is group 0 rolled by one column kind, so that every lane sees every kind."""
    r = rig(name, 8)
    for K in (1, 4, 9, 17, 64):
        a0, b0, w0 = ms.planted_operands(r.p.moduli, r.n, K, 40 + K)
        a = np.stack([a0, np.roll(a0, 1, axis=-1)])
        b = np.stack([b0, np.roll(b0, 1, axis=-1)])
        want = np.stack([w0, np.roll(w0, 1, axis=-1)])
        got = device(r, a, b, in_ntt=True, out_ntt=True)
        assert np.array_equal(got, want), (name, K, np.argwhere(got != want)[:4])
        got = device(r, a, b[:1], shared=True, in_ntt=True, out_ntt=True)
        assert np.array_equal(got[0], want[0])


@pytest.mark.parametrize("log2n", (8, 10))
@pytest.mark.parametrize("name", RIGS)
def test_one_term_is_the_devices_ct_mul_and_the_three_calls_are_the_entry(rig, name, log2n):
    import torch
    r = rig(name, log2n)
    a, b = r.words(r.orc, (3, 2), 540), r.words(r.orc, (3, 2), 550)
    ca, cb = Ciphertext(r.dev(a)), Ciphertext(r.dev(b))
    for out_ntt in (False, True):
        one = r.ev.multiply_sum(ca, cb, 1, out_ntt=out_ntt)
        mul = r.ev.multiply(ca, cb, out_ntt=out_ntt)
        torch.cuda.synchronize()
        assert one.is_ntt == mul.is_ntt == out_ntt and np.array_equal(to_host(one.data), to_host(mul.data)), (name, log2n, out_ntt)
    # what the entry replaces: every pair's product in the NTT domain, the modular sum over them, the inverse transforms
    summed = r.ev.reduce_sum(r.ev.multiply(ca, cb, out_ntt=True))
    three = r.ev.ntt_inverse(summed.data)
    entry = r.ev.multiply_sum(ca, cb, 3)
    torch.cuda.synchronize()
    assert np.array_equal(to_host(three).reshape(1, 3, r.L, r.n), to_host(entry.data)), (name, log2n)


def test_scratch_limit_cuts_groups_and_terms_without_changing_a_word(rig):
    r = fp.ParamsRig("pinned_l4", fr.pinned(12, 4))
    try:
        assert r.L == 4 and r.n == 4096
        a, b = r.words(r.orc, (2, 5, 2), 560), r.words(r.orc, (2, 5, 2), 570)
        forms = {"own": dict(b=b), "shared": dict(b=b[:1], shared=True), "square": dict(b=b, square=True)}
        default = {k: device(r, a, **kw) for k, kw in forms.items()}
        assert np.array_equal(default["own"], reference(r, a, b))
        try:
            for mib in (1, 3):          # 1: a term's transformed operands are 512 KiB, a group is cut into 2 + 2 + 1 terms; 3: one whole group (2.5 MiB) per slice
                r.ctx.set_scratch_limit(mib)
                for k, kw in forms.items():
                    got = device(r, a, **kw)
                    assert np.array_equal(got, default[k]), (mib, k, np.argwhere(got != default[k])[:4])
                ntt = device(r, a, b, out_ntt=True)
                assert np.array_equal(r.orc.ntt_inv(ntt.reshape(-1, r.L, r.n), threads=0).reshape(ntt.shape), default["own"])
        finally:
            r.ctx.set_scratch_limit(1024)
    finally:
        r.close()


def arena_cases(r):
    """the entry with every buffer carved out of one arena at 16-byte (not 32-byte) alignment between guard bands of a whole item: per-group, shared and squared
    second operands in the coefficient domain, and the NTT-domain form that takes no scratch"""
    lib, h, L, n, orc = r.ctx._lib, r.ctx.handle, r.L, r.n, r.orc
    poly = L * n
    ntt = lambda v: orc.ntt_fwd(v.reshape(-1, L, n), threads=0).reshape(v.shape)
    for G, K, form, flags in ((2, 3, "own", 0), (3, 2, "shared", 0), (1, 5, "square", 0), (2, 5, "own", IN_NTT | OUT_NTT)):
        a = r.words(orc, (G, K, 2), 600 + K)
        b = a if form == "square" else r.words(orc, (1 if form == "shared" else G, K, 2), 610 + K)
        want = reference(r, a, b)
        if flags:
            a, b, want = ntt(a), ntt(b), ntt(want)
        c = fp.Case(r)
        c.inp("a", a, 2 * poly)
        if form != "square":
            c.inp("b", b, 2 * poly)
        c.out("out3", G * 3 * poly, 3 * poly, want)

        def call(at, G=G, K=K, form=form, flags=flags):
            return lib.dpfhe_ct_mul_sum(h, at("out3"), at("a"), at("a" if form == "square" else "b"), G, K, 1 if form == "shared" else G, flags, at.stream)
        c.run(f"dpfhe_ct_mul_sum {G} x {K} {form} flags {flags}", call)


ARENA = [("pinned_ld4", 8), ("f64_under_fold", 12)]
ARENA_CASES = 4


@pytest.mark.parametrize("name,log2n", ARENA)
def test_footprint(rig, name, log2n):
    assert fp.Case.gate is None
    arena_cases(rig(name, log2n))


def test_device_entry_rejects_bad_arguments(rig):
    import torch
    r = rig("pinned_ld2", 8)
    lib, h, L, n = r.ctx._lib, r.ctx.handle, r.L, r.n
    z = lambda *s: torch.zeros(s, dtype=torch.int64, device=r.ctx.device)
    G, K = 2, 3
    out, a, b, bs = z(G, 3, L, n), z(G, K, 2, L, n), z(G, K, 2, L, n), z(1, K, 2, L, n)
    f = lib.dpfhe_ct_mul_sum
    p = lambda t: t.data_ptr()
    assert f(h, p(out), p(a), p(b), G, K, G, 0, None) == 0
    assert f(h, p(out), p(a), p(bs), G, K, 1, 0, None) == 0
    for flags in (IN_NTT, OUT_NTT, IN_NTT | OUT_NTT):
        assert f(h, p(out), p(a), p(b), G, K, G, flags, None) == 0
    assert f(h, p(out), p(a), p(b), 0, K, 0, 0, None) == 0 and f(h, None, None, None, 0, K, 1, 0, None) == 0          # no groups: nothing to do
    assert f(None, p(out), p(a), p(b), G, K, G, 0, None) == 2000
    for args in ((None, p(a), p(b)), (p(out), None, p(b)), (p(out), p(a), None), (p(out) + 8, p(a), p(b)), (p(out), p(a) + 8, p(b)), (p(out), p(a), p(b) + 8)):
        assert f(h, *args, G, K, G, 0, None) == 2000 and b"null or misaligned" in lib.dpfhe_last_error(), args
    assert f(h, p(out), p(a), p(b), G, 0, G, 0, None) == 2000 and b"terms" in lib.dpfhe_last_error()
    assert f(h, p(out), p(a), p(b), 3, K, 2, 0, None) == 2000 and b"b_groups" in lib.dpfhe_last_error()
    assert f(h, p(out), p(a), p(b), G, K, 0, 0, None) == 2000
    assert f(h, p(out), p(a), p(b), G, K, G, 4, None) == 2000 and b"unknown flag" in lib.dpfhe_last_error()
    assert f(h, p(a), p(a), p(b), G, K, G, 0, None) == 2000 and b"overlaps" in lib.dpfhe_last_error()                # out on the first operand
    assert f(h, p(b), p(a), p(b), G, K, G, 0, None) == 2000
    assert f(h, p(a) + 16 * L * n, p(a), p(b), 1, K, 1, 0, None) == 2000                                              # ... inside it
    assert f(h, p(bs), p(a), p(bs), G, K, 1, 0, None) == 2000                                                         # ... on the shared operand
    assert f(h, p(out), p(a), p(b), 1 << 31, K, 1 << 31, 0, None) == 2000 and b"too large" in lib.dpfhe_last_error()
    assert f(h, p(out), p(a), p(b), 1 << 20, 1 << 20, 1, 0, None) == 2000 and b"too large" in lib.dpfhe_last_error()
    assert f(h, p(out), p(a), p(a), G, K, G, 0, None) == 0 and f(h, p(out), p(a), p(a), G, K, 1, 0, None) == 0        # read-only operands may alias each other
    assert f(h, p(out), p(a) + 16 * L * n, p(a), 1, K - 1, 1, 0, None) == 0                                           # ... also partly
    torch.cuda.synchronize()
    with pytest.raises(_cabi.DpfheError):
        r.ev.multiply_sum(Ciphertext(a.view(G * K, 2, L, n)), Ciphertext(b.view(G * K, 2, L, n)), 4)                  # 6 items are no multiple of 4 terms
    with pytest.raises(_cabi.DpfheError):
        r.ev.multiply_sum(Ciphertext(a.view(G * K, 2, L, n)), Ciphertext(b.view(G * K, 2, L, n)), K, b_shared=True)   # shared: b holds `terms` items
