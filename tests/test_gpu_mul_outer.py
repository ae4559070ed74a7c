"""-m gpu: the all-pairs tensor product on the device (include/dpfhe.h dpfhe_ct_mul_outer; csrc/mul_outer.h, tensor3_outer_kernel in csrc/kernels_mul.h), word
for word, on the contexts of tests/test_gpu_fused_rescale.py's rig (the pinned fold primes on 3 and 5 limbs, f64 limbs under a fold prime, generic primes).

* flags 0 against the oracle's ct_mul on the pair lists: N = 256 (one partial chunk) and N = 1024, the oracle's 9 x 9 products computed once per rig and
  compared in slices for A, B in {1, 3, 4, 5, 9} (below, at and past the tile of 4 queries and the load-ahead depth of 4 keys) and causal T in {1, 2, 4, 5, 9};
  one case each at N = 4096, N = 16384 and N = 32768 at 2 x 3; a squaring, d_a2 == d_b2;
* DPFHE_IN_NTT | DPFHE_OUT_NTT - the streaming kernel with no transform in between - against Python integers alone, on the planted columns of
  tests/test_emulated_mul_outer.py (tests/mul_outer_ref.py);
* against the device's own dpfhe_ct_mul on materialised pair lists at N = 4096, 5 x 5 causal;
* scratch limits at N = 4096, L = 4, 5 x 5 causal (an item's transform is 256 KiB): 1 MiB (4 items) is below the entry's floor of one query tile and 2 keys - 6 items, 1.5 MiB, which the header states it then takes: one query tile, key
  ranges of 2 -, 2 MiB holds a whole
  (1.25 MiB) and b in ranges of 3, the default holds both: the same words;
* every output is sentinel-filled beforehand with one item of tail: no word outside the A B (or T (T + 1) / 2) items changes, and every word inside does;
* the header's rejections, before the device is touched.
arena_cases() is the footprint case, and - run again by tests/test_gpu_stream_contract_mul_outer.py with Case.gate set - the stream-contract case."""
import numpy as np
import pytest

import fused_rescale_ref as fr
import mul_outer_ref as mo
import test_gpu_footprint as fp
import test_gpu_fused_rescale as fu
from deeppowers_amd import _cabi
from deeppowers_amd.evaluator import Ciphertext, to_host

pytestmark = pytest.mark.gpu

rig = fu.rig
RIGS = ("pinned_ld2", "pinned_ld4", "f64_under_fold", "shoup")
SIZES, CAUSAL_T = (1, 3, 4, 5, 9), (1, 2, 4, 5, 9)
IN_NTT, OUT_NTT, CAUSAL = _cabi.IN_NTT, _cabi.OUT_NTT, _cabi.OUTER_CAUSAL
SENTINEL = 0xDEADBEEFCAFEF00D - (1 << 64)          # >= 2^60 as a word: no residue


def reference(r, a, b):
    """a [A][2][L][N], b [B][2][L][N] -> the oracle's products of the materialised pair lists as [A][B][3][L][N]"""
    A, B = a.shape[0], b.shape[0]
    pa = np.ascontiguousarray(np.broadcast_to(a[:, None], (A, B) + a.shape[1:])).reshape(A * B, 2, r.L, r.n)
    pb = np.ascontiguousarray(np.broadcast_to(b[None], (A, B) + b.shape[1:])).reshape(A * B, 2, r.L, r.n)
    return r.orc.ct_mul(pa, pb, threads=0).reshape(A, B, 3, r.L, r.n)


def device(r, a, b, causal=False, in_ntt=False, out_ntt=None, same=False):
    """the entry on a sentinel-filled output with one item of tail: every item written, the tail untouched"""
    import torch
    A, B = a.shape[0], b.shape[0]
    pairs = A * (A + 1) // 2 if causal else A * B
    ca = Ciphertext(r.dev(a), in_ntt)
    cb = ca if same else Ciphertext(r.dev(b), in_ntt)
    buf = torch.full((pairs + 1, 3, r.L, r.n), SENTINEL, dtype=torch.int64, device=r.ctx.device)
    out = r.ev.multiply_outer(ca, cb, causal=causal, out_ntt=out_ntt, out=buf[:pairs])
    torch.cuda.synchronize()
    assert out.is_ntt == (in_ntt if out_ntt is None else out_ntt)
    assert bool((buf[pairs] == SENTINEL).all()), "the item behind the output changed"
    got = to_host(buf[:pairs])
    assert int(got.max()) < 1 << 60, "a word of the output still holds the sentinel"
    return got


@pytest.mark.parametrize("log2n", (8, 10))
@pytest.mark.parametrize("name", RIGS)
def test_coefficient_domain_equals_the_oracles_products_of_the_pair_lists(rig, name, log2n):
    r = rig(name, log2n)
    assert r.ctx.uses_fold == name.startswith("pinned")
    M = max(SIZES)
    a, b = r.words(r.orc, (M, 2), 1100 + log2n), r.words(r.orc, (M, 2), 1110 + log2n)
    prods = reference(r, a, b)                                  # every product once; the cases below take slices of them
    for A in SIZES:
        for B in SIZES:
            got, want = device(r, a[:A], b[:B]), mo.full_layout(np.ascontiguousarray(prods[:A, :B]))
            assert got.shape == want.shape == (A * B, 3, r.L, r.n)
            assert np.array_equal(got, want), (name, log2n, A, B, np.argwhere(got != want)[:4])
    for T in CAUSAL_T:
        got, want = device(r, a[:T], b[:T], causal=True), mo.causal_layout(prods[:T, :T])
        assert got.shape == want.shape == (T * (T + 1) // 2, 3, r.L, r.n)
        assert np.array_equal(got, want), (name, log2n, T, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("name,log2n", [("pinned_ld4", 12), ("fold_ld2", 14), ("fold_ld2", 15)])
def test_coefficient_domain_at_the_larger_rings(rig, name, log2n):
    r = rig(name, log2n)
    a, b = r.words(r.orc, (2, 2), 1120), r.words(r.orc, (3, 2), 1130)
    got, want = device(r, a, b), mo.full_layout(reference(r, a, b))
    assert np.array_equal(got, want), (name, log2n, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("name,log2n", [("pinned_ld2", 8), ("shoup", 10), ("pinned_ld4", 12)])
def test_squaring_reads_one_buffer(rig, name, log2n):
    """d_a2 == d_b2 with equal counts: every product of a list with itself, one forward transform per item"""
    r = rig(name, log2n)
    a = r.words(r.orc, (5, 2), 1140)
    prods = reference(r, a, a)
    for causal, want in ((False, mo.full_layout(prods)), (True, mo.causal_layout(prods))):
        got = device(r, a, a, causal=causal, same=True)
        assert np.array_equal(got, want), (name, log2n, causal, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("name", RIGS)
def test_ntt_domain_equals_python_integers_on_the_planted_columns(rig, name):
    """no transform on either side: the streaming kernel alone, full and causal, on every size around the tile and the depth"""
    r = rig(name, 8)
    M = max(SIZES)
    a, b, w = mo.planted_operands([int(q) for q in r.p.moduli], r.n, M, M, 70)
    for A, B in ((1, 1), (3, 9), (4, 4), (5, 3), (9, 5), (9, 9)):
        got, want = device(r, a[:A], b[:B], in_ntt=True, out_ntt=True), mo.full_layout(np.ascontiguousarray(w[:A, :B]))
        assert np.array_equal(got, want), (name, A, B, np.argwhere(got != want)[:4])
    for T in CAUSAL_T:
        got, want = device(r, a[:T], b[:T], causal=True, in_ntt=True, out_ntt=True), mo.causal_layout(w[:T, :T])
        assert np.array_equal(got, want), (name, T, np.argwhere(got != want)[:4])


def pair_lists(a, b, causal):
    idx = [(i, j) for i in range(a.shape[0]) for j in range(b.shape[0]) if not causal or j <= i]
    return np.stack([a[i] for i, _ in idx]), np.stack([b[j] for _, j in idx])


def test_equals_the_devices_own_ct_mul_on_materialised_pair_lists(rig):
    import torch
    r = rig("pinned_ld4", 12)
    a, b = r.words(r.orc, (5, 2), 1150), r.words(r.orc, (5, 2), 1160)
    pa, pb = pair_lists(a, b, True)
    for out_ntt in (False, True):
        mul = r.ev.multiply(Ciphertext(r.dev(pa)), Ciphertext(r.dev(pb)), out_ntt=out_ntt)
        torch.cuda.synchronize()
        got = device(r, a, b, causal=True, out_ntt=out_ntt)
        assert np.array_equal(got, to_host(mul.data)), (out_ntt, np.argwhere(got != to_host(mul.data))[:4])


def test_scratch_limit_cuts_queries_and_keys_without_changing_a_word(rig):
    r = fp.ParamsRig("pinned_l4", fr.pinned(12, 4))
    try:
        assert r.L == 4 and r.n == 4096                        # an item's transform: 2 * 4 * 4096 * 8 bytes = 256 KiB
        a, b = r.words(r.orc, (5, 2), 1170), r.words(r.orc, (5, 2), 1180)
        prods = reference(r, a, b)
        default = {c: device(r, a, b, causal=c) for c in (False, True)}
        assert np.array_equal(default[True], mo.causal_layout(prods)) and np.array_equal(default[False], mo.full_layout(prods))
        try:
            for mib in (1, 2, 3):       # 1: fit = 4 items, below the floor of 6 the entry then takes - one tile of 4 queries, keys in ranges of 2; 2: fit = 8 - a whole (5), keys in ranges of 3; 3: all 10
                r.ctx.set_scratch_limit(mib)
                for c in (False, True):
                    got = device(r, a, b, causal=c)
                    assert np.array_equal(got, default[c]), (mib, c, np.argwhere(got != default[c])[:4])
                ntt = device(r, a, b, causal=True, out_ntt=True)
                assert np.array_equal(r.orc.ntt_inv(ntt.reshape(-1, r.L, r.n), threads=0).reshape(ntt.shape), default[True]), mib
                sq = device(r, a, a, causal=True, same=True)
                assert np.array_equal(sq, mo.causal_layout(reference(r, a, a))), mib
        finally:
            r.ctx.set_scratch_limit(1024)
    finally:
        r.close()


def arena_cases(r):
    """the entry with every buffer carved out of one arena at 16-byte (not 32-byte) alignment between guard bands of a whole item: full and causal in the
    coefficient domain (a ragged tile and a ragged end of the key loop), a aliasing b, and the NTT-domain form that takes no scratch"""
    lib, h, L, n, orc = r.ctx._lib, r.ctx.handle, r.L, r.n, r.orc
    poly = L * n
    ntt = lambda v: orc.ntt_fwd(np.ascontiguousarray(v).reshape(-1, L, n), threads=0).reshape(v.shape)
    for A, B, form, flags in ((5, 6, "full", 0), (5, 5, "causal", CAUSAL), (3, 3, "a_is_b", 0), (6, 5, "full", IN_NTT | OUT_NTT), (5, 5, "causal", IN_NTT | OUT_NTT | CAUSAL)):
        a = r.words(orc, (A, 2), 1200 + A)
        b = a if form == "a_is_b" else r.words(orc, (B, 2), 1210 + B)
        prods = reference(r, a, b)
        want = mo.causal_layout(prods) if flags & CAUSAL else mo.full_layout(prods)
        if flags & IN_NTT:
            a, b, want = ntt(a), ntt(b), ntt(want)
        c = fp.Case(r)
        c.inp("a", np.ascontiguousarray(a), 2 * poly)
        if form != "a_is_b":
            c.inp("b", np.ascontiguousarray(b), 2 * poly)
        c.out("out3", want.size, 3 * poly, want)

        def call(at, A=A, B=B, form=form, flags=flags):
            return lib.dpfhe_ct_mul_outer(h, at("out3"), at("a"), at("a") if form == "a_is_b" else at("b"), A, B, flags, at.stream)
        c.run(f"dpfhe_ct_mul_outer {A} x {B} {form} flags {flags}", call)


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
    A, B = 3, 4
    out, a, b = z(A * B, 3, L, n), z(4, 2, L, n), z(4, 2, L, n)
    f = lib.dpfhe_ct_mul_outer
    p = lambda t: t.data_ptr()
    for flags in (0, IN_NTT, OUT_NTT, IN_NTT | OUT_NTT):
        assert f(h, p(out), p(a), p(b), A, B, flags, None) == 0
        assert f(h, p(out), p(a), p(b), 4, 4, flags | CAUSAL, None) == 0                                     # 10 pairs
    assert f(h, p(out), p(a), p(b), 0, B, 0, None) == 0 and f(h, None, None, None, A, 0, 0, None) == 0         # nothing to do
    assert f(None, p(out), p(a), p(b), A, B, 0, None) == 2000
    for args in ((None, p(a), p(b)), (p(out), None, p(b)), (p(out), p(a), None), (p(out) + 8, p(a), p(b)), (p(out), p(a) + 8, p(b)), (p(out), p(a), p(b) + 8)):
        assert f(h, *args, A, B, 0, None) == 2000 and b"null or misaligned" in lib.dpfhe_last_error(), args
    assert f(h, p(out), p(a), p(b), A, B, 8, None) == 2000 and b"unknown flag" in lib.dpfhe_last_error()
    assert f(h, p(out), p(a), p(b), A, B, CAUSAL, None) == 2000 and b"causal" in lib.dpfhe_last_error()
    assert f(h, p(a), p(a), p(b), 1, 1, 0, None) == 2000 and b"overlaps" in lib.dpfhe_last_error()             # out on the queries
    assert f(h, p(b), p(a), p(b), 1, 1, 0, None) == 2000                                                       # ... on the keys
    assert f(h, p(a) + 16 * L * n, p(a), p(b), 2, 1, 0, None) == 2000                                          # ... inside the queries
    assert f(h, p(out), p(out) + 24 * 9 * L * n, p(b), 1, 4, 0, None) == 0                                     # the operand behind the 4 pairs written: no overlap
    assert f(h, p(out), p(out) + 24 * 9 * L * n, p(b), 4, 4, CAUSAL, None) == 2000                             # ... inside the 10 pairs of the causal form
    assert f(h, p(out), p(a), p(b), 1 << 31, 1, 0, None) == 2000 and b"too large" in lib.dpfhe_last_error()
    assert f(h, p(out), p(a), p(b), 1 << 20, 1 << 20, 0, None) == 2000 and b"too large" in lib.dpfhe_last_error()
    assert f(h, p(out), p(a), p(b), 1 << 40, 1 << 40, 0, None) == 2000 and b"too large" in lib.dpfhe_last_error()
    assert f(h, p(out), p(b), p(b), 3, 3, 0, None) == 0                                                        # read-only operands may alias each other
    assert f(h, p(out), p(a) + 16 * L * n, p(a), 3, 3, 0, None) == 0                                           # ... also partly
    torch.cuda.synchronize()
    ca, cb = Ciphertext(a[:3]), Ciphertext(b)
    with pytest.raises(_cabi.DpfheError):
        r.ev.multiply_outer(ca, cb, causal=True)                                        # 3 queries, 4 keys
    with pytest.raises(_cabi.DpfheError):
        r.ev.multiply_outer(ca, Ciphertext(b, True))                                    # different domains
    with pytest.raises(_cabi.DpfheError):
        r.ev.multiply_outer(ca, cb, out=out[:5])                                        # 12 pairs do not fit 5 items
