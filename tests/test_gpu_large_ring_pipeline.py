"""GPU: the packed layers' stages at N = 32768 and 65536, where the transforms are split in two kernels (csrc/ntt_top.h): dpfhe_ntt_inv_galois
(the Galois form of the split inverse: every sub-transform gathers from ONE other sub-block, in place through the stream's scratch arena),
dpfhe_rotate_hoisted_qp and dpfhe_rotate_hybrid_hoisted (its composed, deferred-division path), bit for bit against the oracle, on a context of
fold primes and on one of generic primes; and the three entries held to their declared footprint at N = 32768.  The comparisons are those of
tests/test_gpu_bsgs_qp.py, tests/test_rlwe_semantics.py and tests/test_gpu_footprint.py at the smaller rings."""
import ctypes as C

import numpy as np
import pytest

from class_edges import Rig, expected_class
from deeppowers_amd import _cabi
from deeppowers_amd.params import ntt_primes
from oracle.cbind import Oracle

pytestmark = pytest.mark.gpu

CONTEXTS = [("fold", 15), ("generic", 15), ("fold", 16), ("generic", 16)]
IDS = [f"{k}_n{1 << ln}" for k, ln in CONTEXTS]
N32768 = [c for c in CONTEXTS if c[1] == 15]
_PARAMS = {}


def params(kind, ln):
    """fold: the three largest primes below 2^60 that are 1 mod 2N (2 data limbs + P, all 2^60 - d); generic: the three below 2^55 (all shoup)"""
    if (kind, ln) not in _PARAMS:
        p = ntt_primes(ln, 3) if kind == "fold" else ntt_primes(ln, 3, 55)
        assert {expected_class(q) for q in p.moduli} == ({"fold"} if kind == "fold" else {"shoup"})
        _PARAMS[(kind, ln)] = p
    return _PARAMS[(kind, ln)]


@pytest.fixture
def rig():
    made = []

    def make(kind, ln):
        r = Rig(params(kind, ln))
        r.kind = f"{kind}{ln}"
        assert r.ctx.uses_fold == (kind == "fold")
        made.append(r)
        return r
    yield make
    for r in made:
        r.close()


def galois_elements(ln):
    """the identity, 3 and its inverse, -1, an element that is 1 mod 2 N1 (every sub-block its own source, at a non-zero offset), a far power of 3"""
    two_n, n1 = 2 << ln, 1 << (ln - 12)
    return [1, 3, pow(3, -1, two_n), two_n - 1, 2 * n1 + 1, pow(3, 77, two_n)]


@pytest.mark.parametrize("kind,ln", CONTEXTS, ids=IDS)
def test_ntt_inverse_galois_bit_exact(rig, kind, ln):
    """out of place, in place, in place again (the arena must not grow), and in place in at least 3 slices under a 1 MiB scratch limit: the same words"""
    from deeppowers_amd.evaluator import to_host
    r = rig(kind, ln)
    orc, L, n, ctx, ev = r.orc, r.L, r.n, r.ctx, r.ev
    for k, per in ((1, 1), (6, 3), (70, 1)):
        if k == 6:
            elts = galois_elements(ln)
        else:
            elts = [pow(3, 5 * i, 2 * n) for i in range(k)]     # (k = 1: the identity)
            if k > 2:
                elts[2] = 2 * n - 1
        x = orc.fill(k * per, 811 + k).reshape(k, per, L, n)
        inv = orc.ntt_inv(x, threads=0)
        want = np.stack([orc.apply_galois(inv[e], elts[e]) for e in range(k)])
        d = r.dev(x)
        got = to_host(ev.ntt_inverse_galois(d, elts))
        assert np.array_equal(got, want), (k, per, "out of place")
        assert np.array_equal(to_host(d), x), (k, per, "the input of an out-of-place call changed")
        ev.ntt_inverse_galois(d, elts, out=d)
        assert np.array_equal(to_host(d), want), (k, per, "in place")
        held = ctx.scratch_bytes
        assert held >= min(k, 64) * per * L * n * 8                # one 64-element launch group is staged at a time
        d = r.dev(x)
        ev.ntt_inverse_galois(d, elts, out=d)
        assert np.array_equal(to_host(d), want) and ctx.scratch_bytes == held, (k, per, "repeated in place")
        if k >= 3:
            ctx.set_scratch_limit(1)
            fit = max(1, min(64, (1 << 17) // (per * L * n)))   # elements per slice under 1 MiB (2^17 words)
            assert -(-k // fit) >= 3
            d = r.dev(x)
            ev.ntt_inverse_galois(d, elts, out=d)
            ctx.set_scratch_limit(1024)
            assert np.array_equal(to_host(d), want) and ctx.scratch_bytes == held, (k, per, "in place, sliced")


def _hoisted_qp_case(r, k, T, seed):
    from deeppowers_amd.evaluator import Ciphertext, to_host
    pe, orc, L, n = r.p, r.orc, r.L, r.n
    Ld = L - 1
    data = Oracle(pe.log2_n, pe.moduli[:-1], pe.psi[:-1])
    elts = [pow(3, i + 1, 2 * n) for i in range(k)]
    if k:
        elts[-1] = 2 * n - 1
    keys = orc.fill(max(k, 1) * Ld * 2, seed).reshape(max(k, 1), Ld, 2, L, n)[:k]
    cts = data.fill(T * 2, seed + 1 + k).reshape(T, 2, Ld, n)
    cts[0, 1] = (np.array(pe.moduli[:-1], np.uint64) - np.uint64(1))[:, None]       # worst-case digits
    got = to_host(r.ev.rotate_hoisted_qp(Ciphertext(r.dev(cts)), elts, r.dev(keys) if k else None))
    assert got.shape == (k + 1, T, 2, L, n)
    idx = list(range(k)) if k <= 8 else [0, 1, 15, 16, 63, 64, k - 1]
    for t in range(T):
        want = orc.rotate_hoisted_qp(cts[t], [elts[i] for i in idx], keys[idx] if k else keys, threads=0)
        assert np.array_equal(got[0, t], want[0]), (k, t, "identity block")
        for w, i in zip(want[1:], idx):
            assert np.array_equal(got[1 + i, t], w), (k, t, i)


@pytest.mark.parametrize("kind,ln", CONTEXTS, ids=IDS)
def test_rotate_hoisted_qp_bit_exact(rig, kind, ln):
    r = rig(kind, ln)
    for k, T in (((5, 1), (66, 2), (0, 2)) if ln == 15 else ((5, 1), (0, 2))):
        _hoisted_qp_case(r, k, T, 801)


def test_rotate_hoisted_qp_on_the_all_fold_chain_of_n32768():
    """FheParams.n32768(8): 7 digits - the loop-form stream kernel, not the up-front one (which stops at 6)"""
    p = ntt_primes(15, 8)
    assert {expected_class(q) for q in p.moduli} == {"fold"}
    r = Rig(p)
    try:
        assert r.ctx.uses_fold
        _hoisted_qp_case(r, 2, 1, 841)
    finally:
        r.close()


@pytest.mark.parametrize("kind,ln", N32768, ids=[f"{k}_n32768" for k, _ in N32768])
def test_rotate_hybrid_hoisted_composed_path(rig, kind, ln):
    """3 rotations of 2 items through the deferred-division pipeline, d_work / d_rotated0 NULL; and again in slices of one rotation"""
    import torch
    from deeppowers_amd.evaluator import to_host
    r = rig(kind, ln)
    pe, orc, L, n, ctx = r.p, r.orc, r.L, r.n, r.ctx
    Ld, k, T = L - 1, 3, 2
    data = Oracle(pe.log2_n, pe.moduli[:-1], pe.psi[:-1])
    elts = [3, pow(3, 9, 2 * n), 2 * n - 1]
    keys = orc.fill(k * Ld * 2, 703).reshape(k, Ld, 2, L, n)
    cts = r.words(data, (T, 2), 704)
    want = np.stack([orc.rotate_hoisted(cts[t], elts, keys, threads=0) for t in range(T)], axis=1)      # [k][T][2][Ld][N]: rotation-major
    d_in, d_keys = r.dev(cts), r.dev(keys)
    ge = (C.c_uint32 * k)(*elts)
    for limit in (1024, 9):   # a (rotation, all items) block over Q P is T 2 L N words = 3 MiB: 9 MiB holds block 0, the inputs' share and ONE rotation per slice
        ctx.set_scratch_limit(limit)
        out = torch.zeros((k * T, 2, Ld, n), dtype=torch.int64, device=ctx.device)
        digits = torch.empty((T, Ld, L, n), dtype=torch.int64, device=ctx.device)
        _cabi.check(ctx._lib.dpfhe_rotate_hybrid_hoisted(ctx.handle, out.data_ptr(), d_in.data_ptr(), T, ge, d_keys.data_ptr(), None, None, digits.data_ptr(), k, None),
                    "dpfhe_rotate_hybrid_hoisted")
        assert np.array_equal(to_host(out).reshape(k, T, 2, Ld, n), want), limit
    ctx.set_scratch_limit(1024)


@pytest.mark.parametrize("kind,ln", N32768, ids=[f"{k}_n32768" for k, _ in N32768])
def test_the_whole_deferred_sum(rig, kind, ln):
    """tests/test_gpu_bsgs_qp.py test_rescale_bsgs_and_the_whole_deferred_sum at N = 32768 with 3 giant steps of 2 tokens:
         rescale_bsgs(INTT(sum_i switch_key_qp(rot_i)), rot)
    equals the oracle's same order of operations word for word, and the per-term path up to one rounding per term."""
    import torch
    from deeppowers_amd.evaluator import Ciphertext, to_host
    r = rig(kind, ln)
    pe, orc, L, n, ctx, ev = r.p, r.orc, r.L, r.n, r.ctx, r.ev
    Ld, n2, T = L - 1, 3, 2
    data = Oracle(pe.log2_n, pe.moduli[:-1], pe.psi[:-1])
    rot = data.fill(n2 * T * 2, 831).reshape(n2, T, 2, Ld, n)
    keys = orc.fill((n2 - 1) * Ld * 2, 833).reshape(n2 - 1, Ld, 2, L, n)
    d_rot = r.dev(rot)
    terms = ev.switch_key_qp(Ciphertext(d_rot[1:].reshape((n2 - 1) * T, 2, Ld, n)), r.dev(keys), T)      # [(n2-1) T][2][L][N]
    summed = torch.empty((T, 2, L, n), dtype=torch.int64, device=ctx.device)
    _cabi.check(ctx._lib.dpfhe_reduce_sum(ctx.handle, summed.data_ptr(), terms.data_ptr(), n2 - 1, T * 2, None), "dpfhe_reduce_sum")
    ev.ntt_inverse_(summed)
    got = to_host(ev.rescale_bsgs(summed, d_rot))
    acc = np.zeros((T, 2, L, n), np.uint64)
    for i in range(1, n2):
        acc = orc.dyadic("add", acc, orc.switch_key_qp(rot[i], keys[i - 1], threads=0))
    want = orc.rescale(orc.ntt_inv(acc))
    for t in range(T):
        for a in range(n2):
            want[t, 0] = data.dyadic("add", want[t, 0][None].copy(), rot[a, t, 0][None].copy())[0]
        want[t, 1] = data.dyadic("add", want[t, 1][None].copy(), rot[0, t, 1][None].copy())[0]
    assert np.array_equal(got, want)
    per_term = rot[0].copy()
    for i in range(1, n2):
        per_term = data.dyadic("add", per_term, orc.keyswitch_hybrid(rot[i], keys[i - 1], 2, threads=0))
    q = np.array(pe.moduli[:-1], np.uint64)[None, None, :, None]
    diff = (got.astype(object) - per_term.astype(object)) % q.astype(object)
    diff = np.minimum(diff, q.astype(object) - diff)
    assert int(diff.max()) <= n2


@pytest.mark.parametrize("kind,ln", N32768, ids=[f"{k}_n32768" for k, _ in N32768])
def test_footprints_at_n32768(rig, kind, ln):
    """the three entries inside tests/footprint.py's arena, as tests/test_gpu_footprint.py holds them at the smaller rings: guard bands, both fill patterns,
    16-byte alignment, every caller buffer at exactly the header's size; dpfhe_ntt_inv_galois apart and with d_out == d_in, one element and six"""
    import test_gpu_footprint as fp
    r = rig(kind, ln)
    lib, h, L, n, orc = r.ctx._lib, r.ctx.handle, r.L, r.n, r.orc
    fp.run_rotate_hoisted_qp(r, 0, 2)
    fp.run_rotate_hoisted_qp(r, 3, 2)
    fp.run_rotate_hoisted(r, 3, 2)
    for k, per in ((6, 2), (1, 1)):
        elts = galois_elements(ln)[:k] if k > 1 else [2 * n - 1]
        x = r.words(orc, (k, per), 720)
        inv = orc.ntt_inv(x, threads=0)
        want = np.stack([orc.apply_galois(inv[e], elts[e]) for e in range(k)])
        c = fp.Case(r)
        c.inp("in", x, per * L * n)
        c.out("out", x.size, per * L * n, want)
        c.run(f"dpfhe_ntt_inv_galois {k} x {per}", lambda at: lib.dpfhe_ntt_inv_galois(h, at("out"), at("in"), per, fp.u32(elts), k, at.stream))
        c = fp.Case(r)
        c.inout("io", x, per * L * n, want)
        c.run(f"dpfhe_ntt_inv_galois {k} x {per}, d_out == d_in", lambda at: lib.dpfhe_ntt_inv_galois(h, at("io"), at("io"), per, fp.u32(elts), k, at.stream))
