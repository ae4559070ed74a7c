"""-m gpu: products with a shared complement factor on the device (include/dpfhe.h dpfhe_ct_mul_complement; csrc/mul_complement.h, tensor3_complement_kernel in
csrc/kernels_mul.h), word for word, on the contexts of tests/test_gpu_fused_rescale.py's rig (the pinned fold primes on 3 and 5 limbs, f64 limbs under a fold
prime, generic primes).

* flags 0 against the oracle's ct_mul(a, F) with F = kappa X^0 - b built on the host in integers: N = 256 (one partial chunk) and N = 1024, terms in
  {0 (with self), 1, 3, 4, 5, 9}, groups in {1, 3}, with and without the self product, kappa a 61-bit integer (its residues differ per limb); one case each at
  N = 4096, N = 16384 and N = 32768;
* DPFHE_IN_NTT | DPFHE_OUT_NTT - the streaming kernel with no transform in between - against Python integers alone, on the planted columns of
  tests/test_emulated_mul_complement.py (tests/mul_complement_ref.py: the factor on its edges, products solved to land on 0, 1, q - 1 and either side of q / 2);
* terms = 1 without the self product against the device's own dpfhe_negate + dpfhe_add_plain + dpfhe_ct_mul;
* scratch limits at N = 4096, L = 4, terms = 5, groups = 2 (an item's transform is 256 KiB, a group's 1.5 MiB): 1 MiB cuts every group into b and ranges of 3
  and 2 numerators, 2 MiB takes one whole group per slice, 3 MiB both: the words of the default limit;
* the header's rejections, before the device is touched.
arena_cases() is the footprint case, and - run again by tests/test_gpu_stream_contract_mul_complement.py with Case.gate set - the stream-contract case."""
import numpy as np
import pytest

import fused_rescale_ref as fr
import mul_complement_ref as mc
import test_gpu_footprint as fp
import test_gpu_fused_rescale as fu
from deeppowers_amd import _cabi
from deeppowers_amd.evaluator import Ciphertext, to_host

pytestmark = pytest.mark.gpu

rig = fu.rig
RIGS = ("pinned_ld2", "pinned_ld4", "f64_under_fold", "shoup")
TERMS, GROUPS = (0, 1, 3, 4, 5, 9), (1, 3)
IN_NTT, OUT_NTT = _cabi.IN_NTT, _cabi.OUT_NTT
KAPPA = (1 << 60) + 0x0123456789ABCDE            # 61 bits: another residue on every limb


def residues(r, kappa=KAPPA):
    return np.array([kappa % int(q) for q in r.p.moduli], dtype=np.uint64)


def host_factor(r, b, kap):
    """b [G][2][L][N] coefficient domain -> kappa X^0 - b: every word negated mod q_l (0 stays 0), kappa_l added to coefficient 0 of component 0"""
    q = r.qcol
    f = (q - b) % q
    f[:, 0, :, 0] = (f[:, 0, :, 0] + kap) % q[:, 0]
    return f


def reference(r, a, b, kap):
    """a [G][K][2][L][N], b [G][2][L][N] -> the oracle's a[g][k] (x) F_g as [G][K][3][L][N] and b[g] (x) F_g as [G][3][L][N]"""
    G, K = a.shape[:2]
    f = host_factor(r, b, kap)
    if K == 0:
        return np.zeros((G, 0, 3, r.L, r.n), dtype=np.uint64), r.orc.ct_mul(np.ascontiguousarray(b), f, threads=0)
    fk =np.ascontiguousarray(np.broadcast_to(f[:, None], a.shape)).reshape(G * K, 2, r.L, r.n)
    prods = r.orc.ct_mul(np.ascontiguousarray(a).reshape(G * K, 2, r.L, r.n), fk, threads=0).reshape(G, K, 3, r.L, r.n)
    return prods, r.orc.ct_mul(np.ascontiguousarray(b), f, threads=0)


def layout(prods, selfs, with_self):
    """the entry's output: the products group-major, then the self products"""
    flat = prods.reshape((-1,) + prods.shape[2:])
    return np.concatenate([flat, selfs]) if with_self else flat


def device(r, a, b, kap, with_self=True, in_ntt=False, out_ntt=None):
    import torch
    G, K = a.shape[:2]
    da = Ciphertext(r.dev(a.reshape(G * K, 2, r.L, r.n)), in_ntt) if K else None
    out = r.ev.multiply_complement(da, Ciphertext(r.dev(b), in_ntt), r.dev(kap), K, with_self=with_self, out_ntt=out_ntt)
    torch.cuda.synchronize()
    return to_host(out.data)


@pytest.mark.parametrize("log2n", (8, 10))
@pytest.mark.parametrize("name", RIGS)
def test_coefficient_domain_equals_the_oracles_products_with_the_host_factor(rig, name, log2n):
    r = rig(name, log2n)
    assert r.ctx.uses_fold == name.startswith("pinned")
    kap = residues(r)
    assert len(set(int(v) for v in kap)) == r.L
    Gm, Km = max(GROUPS), max(TERMS)
    a, b = r.words(r.orc, (Gm, Km, 2), 800 + log2n), r.words(r.orc, (Gm, 2), 810 + log2n)
    prods, selfs = reference(r, a, b, kap)                      # every product once; the cases below take slices of them
    for G in GROUPS:
        for K in TERMS:
            for with_self in (False, True):
                if K == 0 and not with_self:
                    continue
                got = device(r, np.ascontiguousarray(a[:G, :K]), np.ascontiguousarray(b[:G]), kap, with_self=with_self)
                want = layout(prods[:G, :K], selfs[:G], with_self)
                assert got.shape == want.shape == (G * K + (G if with_self else 0), 3, r.L, r.n)
                assert np.array_equal(got, want), (name, log2n, G, K, with_self, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("name,log2n", [("pinned_ld4", 12), ("fold_ld2", 14), ("fold_ld2", 15)])
def test_coefficient_domain_at_the_larger_rings(rig, name, log2n):
    r = rig(name, log2n)
    kap = residues(r)
    a, b = r.words(r.orc, (1, 1, 2), 820), r.words(r.orc, (1, 2), 830)
    got, want = device(r, a, b, kap), layout(*reference(r, a, b, kap), True)
    assert np.array_equal(got, want), (name, log2n, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("name", RIGS)
def test_ntt_domain_equals_python_integers_on_the_planted_columns(rig, name):
    """no transform on either side: the streaming kernel alone.  Group 1 is group 0 rolled by one column, so that every lane sees other kinds; the limbs' kappa
    kinds rotate with the case."""
    r = rig(name, 8)
    rng = np.random.default_rng(7)
    for case, K in enumerate((0, 1, 4, 5, 9)):
        kappas = [mc.kappa_of(int(q), mc.KAPPA_KINDS[(l + case) % len(mc.KAPPA_KINDS)], rng) for l, q in enumerate(r.p.moduli)]
        a0, b0, w0 = mc.planted_operands([int(q) for q in r.p.moduli], r.n, K, kappas, 60 + K)
        a = np.stack([a0, np.roll(a0, 1, axis=-1)])
        b = np.stack([b0, np.roll(b0, 1, axis=-1)])
        w = np.stack([w0, np.roll(w0, 1, axis=-1)])
        kap = np.array(kappas, dtype=np.uint64)
        got = device(r, a, b, kap, in_ntt=True, out_ntt=True)
        want = layout(w[:, :K], w[:, K], True)
        assert np.array_equal(got, want), (name, K, np.argwhere(got != want)[:4])
        if K:
            got = device(r, a, b, kap, with_self=False, in_ntt=True, out_ntt=True)
            assert np.array_equal(got, want[:2 * K]), (name, K)


@pytest.mark.parametrize("log2n", (8, 10))
@pytest.mark.parametrize("name", RIGS)
def test_one_term_is_the_devices_negate_add_plain_and_ct_mul(rig, name, log2n):
    import torch
    r = rig(name, log2n)
    kap = residues(r)
    a, b = r.words(r.orc, (3, 2), 840), r.words(r.orc, (3, 2), 850)
    plain = np.zeros((1, r.L, r.n), dtype=np.uint64)
    plain[0, :, 0] = kap
    ca, cb = Ciphertext(r.dev(a)), Ciphertext(r.dev(b))
    f = r.ev.negate(cb)
    r.ev.add_plain_(f.data, r.dev(plain))
    for out_ntt in (False, True):
        one = r.ev.multiply_complement(ca, cb, r.dev(kap), 1, with_self=False, out_ntt=out_ntt)
        mul = r.ev.multiply(ca, f, out_ntt=out_ntt)
        torch.cuda.synchronize()
        assert one.is_ntt == mul.is_ntt == out_ntt and np.array_equal(to_host(one.data), to_host(mul.data)), (name, log2n, out_ntt)


def test_scratch_limit_cuts_groups_and_terms_without_changing_a_word(rig):
    r = fp.ParamsRig("pinned_l4", fr.pinned(12, 4))
    try:
        assert r.L == 4 and r.n == 4096
        kap = residues(r)
        a, b = r.words(r.orc, (2, 5, 2), 860), r.words(r.orc, (2, 2), 870)
        default = {ws: device(r, a, b, kap, with_self=ws) for ws in (False, True)}
        assert np.array_equal(default[True], layout(*reference(r, a, b, kap), True))
        assert np.array_equal(default[False], default[True][:10])
        try:
            for mib in (1, 2, 3):       # 1: b[g] and ranges of 3 + 2 numerators per group; 2: one whole group (1.5 MiB) per slice; 3: both groups
                r.ctx.set_scratch_limit(mib)
                for ws in (False, True):
                    got = device(r, a, b, kap, with_self=ws)
                    assert np.array_equal(got, default[ws]), (mib, ws, np.argwhere(got != default[ws])[:4])
                ntt = device(r, a, b, kap, out_ntt=True)
                assert np.array_equal(r.orc.ntt_inv(ntt.reshape(-1, r.L, r.n), threads=0).reshape(ntt.shape), default[True])
                only_self = device(r, a[:, :0], b, kap)
                assert np.array_equal(only_self, default[True][10:])
        finally:
            r.ctx.set_scratch_limit(1024)
    finally:
        r.close()


def arena_cases(r):
    """the entry with every buffer carved out of one arena at 16-byte (not 32-byte) alignment between guard bands of a whole item: with and without the self
    product in the coefficient domain, a aliasing b, the self products alone, and the NTT-domain form that takes no scratch"""
    lib, h, L, n, orc = r.ctx._lib, r.ctx.handle, r.L, r.n, r.orc
    poly = L * n
    kap = residues(r)
    ntt = lambda v: orc.ntt_fwd(v.reshape(-1, L, n), threads=0).reshape(v.shape)
    for G, K, form, flags in ((2, 3, "self", 0), (3, 2, "no_self", 0), (2, 1, "a_is_b", 0), (2, 0, "self", 0), (2, 5, "self", IN_NTT | OUT_NTT)):
        b = r.words(orc, (G, 2), 910 + K)
        a = b.reshape(G, 1, 2, L, n) if form == "a_is_b" else r.words(orc, (G, max(K, 1), 2), 900 + K)[:, :K]
        with_self = form != "no_self"
        want = layout(*reference(r, a, b, kap), with_self)
        if flags:      # the constant is kappa in every word there: the transform of kappa X^0
            a, b, want = ntt(np.ascontiguousarray(a)), ntt(b), ntt(want)
        c = fp.Case(r)
        if K and form != "a_is_b":
            c.inp("a", np.ascontiguousarray(a), 2 * poly)
        c.inp("b", b, 2 * poly)
        c.inp("kappa", kap, L)
        c.out("out3", want.size, 3 * poly, want)

        def call(at, G=G, K=K, form=form, flags=flags, with_self=with_self):
            pa = at("b") if form == "a_is_b" else at("a") if K else None
            return lib.dpfhe_ct_mul_complement(h, at("out3"), pa, at("b"), at("kappa"), G, K, int(with_self), flags, at.stream)
        c.run(f"dpfhe_ct_mul_complement {G} x {K} {form} flags {flags}", call)


ARENA = [("pinned_ld4", 8), ("f64_under_fold", 12)]
ARENA_CASES = 5


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
    out, a, b, kap = z(G * (K + 1), 3, L, n), z(G, K, 2, L, n), z(G, 2, L, n), z(4 * L)
    f = lib.dpfhe_ct_mul_complement
    p = lambda t: t.data_ptr()
    for ws in (0, 1):
        for flags in (0, IN_NTT, OUT_NTT, IN_NTT | OUT_NTT):
            assert f(h, p(out), p(a), p(b), p(kap), G, K, ws, flags, None) == 0
    assert f(h, p(out), None, p(b), p(kap), G, 0, 1, 0, None) == 0                                                      # no numerators: the self products alone
    assert f(h, p(out), p(a), p(b), p(kap), 0, K, 1, 0, None) == 0 and f(h, None, None, None, None, 0, K, 0, 0, None) == 0    # no groups: nothing to do
    assert f(None, p(out), p(a), p(b), p(kap), G, K, 1, 0, None) == 2000
    for args in ((None, p(a), p(b), p(kap)), (p(out), None, p(b), p(kap)), (p(out), p(a), None, p(kap)), (p(out), p(a), p(b), None),
                 (p(out) + 8, p(a), p(b), p(kap)), (p(out), p(a) + 8, p(b), p(kap)), (p(out), p(a), p(b) + 8, p(kap)), (p(out), p(a), p(b), p(kap) + 8)):
        assert f(h, *args, G, K, 1, 0, None) == 2000 and b"null or misaligned" in lib.dpfhe_last_error(), args
    assert f(h, p(out), p(a), p(b), p(kap), G, 0, 0, 0, None) == 2000 and b"terms" in lib.dpfhe_last_error()
    assert f(h, p(out), p(a), p(b), p(kap), G, K, 1, 4, None) == 2000 and b"unknown flag" in lib.dpfhe_last_error()
    assert f(h, p(a), p(a), p(b), p(kap), G, K, 0, 0, None) == 2000 and b"overlaps" in lib.dpfhe_last_error()           # out on the numerators
    assert f(h, p(b), p(a), p(b), p(kap), G, K, 1, 0, None) == 2000                                                     # ... on the denominators
    assert f(h, p(a) + 16 * L * n, p(a), p(b), p(kap), 1, K, 0, 0, None) == 2000                                        # ... inside the numerators
    assert f(h, p(kap), p(a), p(b), p(kap), G, K, 1, 0, None) == 2000 and b"overlaps" in lib.dpfhe_last_error()         # ... on kappa
    assert f(h, p(out), p(a), p(b), p(out) + 8 * (G * K * 3 + 1) * L * n, G, K, 1, 0, None) == 2000                     # kappa inside the self products
    assert f(h, p(out), p(a), p(b), p(out) + 8 * (G * K * 3 + 1) * L * n, G, K, 0, 0, None) == 0                        # ... which are not written without with_self
    assert f(h, p(out), p(a), p(b), p(kap), 1 << 31, K, 1, 0, None) == 2000 and b"too large" in lib.dpfhe_last_error()
    assert f(h, p(out), p(a), p(b), p(kap), 1 << 20, 1 << 20, 1, 0, None) == 2000 and b"too large" in lib.dpfhe_last_error()
    assert f(h, p(out), p(b), p(b), p(kap), G, 1, 1, 0, None) == 0                                                      # read-only operands may alias each other
    assert f(h, p(out), p(a) + 16 * L * n, p(a), p(kap), 1, 1, 1, 0, None) == 0                                         # ... also partly
    torch.cuda.synchronize()
    ca, cb = Ciphertext(a.view(G * K, 2, L, n)), Ciphertext(b)
    with pytest.raises(_cabi.DpfheError):
        r.ev.multiply_complement(ca, cb, kap[:L].contiguous(), 2)                       # 6 items are not 2 groups of 2
    with pytest.raises(_cabi.DpfheError):
        r.ev.multiply_complement(None, cb, kap[:L].contiguous(), 0, with_self=False)    # nothing to compute
    with pytest.raises(_cabi.DpfheError):
        r.ev.multiply_complement(ca, cb, kap, K)                                        # kappa holds one word per limb
