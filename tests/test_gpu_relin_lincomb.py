"""-m gpu: the fused relinearise + linear combination + rescale on the device (include/dpfhe.h dpfhe_relinearize_lincomb_rescale_hybrid; csrc/fused_rescale.h
(c), relin_lincomb_rescale_kernel in csrc/kernels_keyswitch.h).

Word for word against the ORACLE's hybrid relinearisation, orc.keyswitch_hybrid(ct3, key, 3), followed by the Python-integer sum and rescale of
tests/relin_lincomb_ref.py (every division through the CRT integer of its coefficient): the fused path at N = 256 (one partial chunk) and N = 4096 on the pinned
fold primes at Ld = 2 (one output limb) and Ld = 4 and on a mixed-class context, the composed path at N = 16384 (one case, batch 1); K in {0, 1, 5, 15}; terms at
Ld and Ld + 2 limbs mixed in one call, the limbs that are not read filled with a word that is no residue; and the 6 x 6 planted edges of
tests/test_relin_lincomb_cpu.py reached through the whole entry: the key is solved as in tests/test_gpu_fused_rescale.py so that item 0's key-switched sums sit
on the edges of P, and a term's word on the last data limb is solved so that s_last lands on the edges of q_last.  The oracle confirms both before the device is
asked.  K = 0 with weight one against the device's own dpfhe_relinearize_rescale_hybrid.
arena_cases() is the footprint case (terms between guard bands, a taller term's upper limbs holding non-residues that must neither be read nor change), and - run
again by tests/test_gpu_stream_contract_relin_lincomb.py with Case.gate set - the stream-contract case."""
import ctypes as C

import numpy as np
import pytest

import fused_rescale_ref as fr
import relin_lincomb_ref as rl
import test_gpu_footprint as fp
import test_gpu_fused_rescale as fu
from deeppowers_amd.evaluator import Ciphertext, to_host

pytestmark = pytest.mark.gpu

rig = fu.rig
# (context, log2 N, [(K, batch)]): every K on the small ring at both batches; at N = 4096 every K once, the batches shared out
SMALL = [(name, 8, [(K, b) for K in (0, 1, 5, 15) for b in (1, 3)]) for name in ("pinned_ld2", "pinned_ld4")]
LARGE = [(name, 12, [(0, 1), (1, 3), (5, 1), (15, 1)]) for name in ("pinned_ld2", "pinned_ld4", "f64_under_fold")]
COMPOSED = [("fold_ld2", 14, [(5, 1)])]
CASES = SMALL + LARGE + COMPOSED


def reference(r, ct3, key, terms, w):
    """the parent's hybrid relinearisation by the oracle, then the integers"""
    return rl.combine_reference(list(r.p.moduli[:-1]), r.orc.keyswitch_hybrid(ct3, key, 3, threads=0), terms, w)


def device(r, ct3, key, terms, w):
    import torch
    out = r.ev.relinearize_lincomb_rescale_hybrid(Ciphertext(r.dev(ct3)), r.dev(key), [r.dev(z) for z in terms], r.dev(w))
    torch.cuda.synchronize()
    return to_host(out.data)


@pytest.mark.parametrize("name,log2n,shapes", CASES, ids=[f"{n}_n{1 << ln}" for n, ln, _ in CASES])
def test_equals_the_oracle_and_the_integers(rig, name, log2n, shapes):
    r = rig(name, log2n)
    Ld, data = r.L - 1, fp.data_oracle(r)
    assert r.ctx.uses_fold == name.startswith(("pinned", "fold"))
    key = r.words(r.orc, (Ld, 2), 41)
    for K, batch in shapes:
        ct3 = r.words(data, (batch, 3), 50 + batch)
        terms, w = rl.terms_and_weights(r.p, K, batch, 60 + K)
        assert [z.shape[2] for z in terms] == rl.term_limbs(K, Ld)
        got, want = device(r, ct3, key, terms, w), reference(r, ct3, key, terms, w)
        assert got.shape == want.shape == (batch, 2, Ld - 1, r.n)
        assert np.array_equal(got, want), (name, log2n, K, batch, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("K", (0, 1, 5))
@pytest.mark.parametrize("name", ("pinned_ld2", "pinned_ld4", "f64_under_fold"))
def test_planted_edges(rig, name, K):
    r = rig(name, 8)
    p, Ld = r.p, r.L - 1
    ct3, key, plan = fu.planted(r, 2, 77)
    assert plan == rl.plan_of(p) and len({(wp, t) for _, wp, t in plan}) == 36
    terms, w = rl.terms_and_weights(p, K, 2, 78 + K)
    mid = r.orc.keyswitch_hybrid(ct3, key, 3, threads=0)
    rl.aim_s_last(p, mid[0, :, Ld - 1], ct3[0, :, Ld - 1], terms, w, plan)
    # the oracle's own words: the sums still sit on the edges of P (only c0, c1 or a term moved), and s_last on the edges of the last data prime
    S = r.orc.ntt_inv(r.orc.switch_key_qp(np.ascontiguousarray(ct3[:, 1:]), key, threads=0), threads=0)
    mid = r.orc.keyswitch_hybrid(ct3, key, 3, threads=0)
    for c in range(2):
        assert [int(S[0, c, -1, j]) for j, _, _ in plan] == [wp for _, wp, _ in plan]
        s_last = rl.sums(list(p.moduli[:-1]), mid, terms, w, 0, c)[-1]
        assert [int(s_last[j]) for j, _, _ in plan] == [t for _, _, t in plan]
    got, want = device(r, ct3, key, terms, w), rl.combine_reference(list(p.moduli[:-1]), mid, terms, w)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    # and the last pass alone, on the same sums: the host twin
    assert np.array_equal(rl.pass_twin(p, S, ct3, terms, w), want)


@pytest.mark.parametrize("name,log2n", [("pinned_ld2", 8), ("pinned_ld4", 12), ("f64_under_fold", 12), ("fold_ld2", 14)])
def test_no_terms_weight_one_is_the_devices_relinearize_rescale(rig, name, log2n):
    import torch
    r = rig(name, log2n)
    Ld, data = r.L - 1, fp.data_oracle(r)
    key = r.words(r.orc, (Ld, 2), 43)
    ct3 = r.words(data, (2, 3), 53)
    w = np.zeros((2, Ld), np.uint64)
    w[0] = 1
    want = r.ev.relinearize_rescale_hybrid(Ciphertext(r.dev(ct3)), r.dev(key))
    torch.cuda.synchronize()
    assert np.array_equal(device(r, ct3, key, [], w), to_host(want.data))


def arena_cases(r):
    """the entry with every buffer carved out of one arena at 16-byte (not 32-byte) alignment between guard bands of a whole item: d_work at exactly
    batch * 2 * L * N words, every term a buffer of its own, the taller terms' upper limbs holding a word that is no residue (read, it would change an output
    word; it must also still be there afterwards)"""
    lib, h, L, n, orc = r.ctx._lib, r.ctx.handle, r.L, r.n, r.orc
    Ld, data = L - 1, fp.data_oracle(r)
    key = r.words(orc, (Ld, 2), 303)
    for K, batch in ((0, 1), (2, 3), (5, 1)):
        ct3 = r.words(data, (batch, 3), 313)
        terms, w = rl.terms_and_weights(r.p, K, batch, 323 + K)
        assert K < 2 or (terms[1].shape[2] == Ld + 2 and (terms[1][:, :, Ld:] == rl.NOT_A_RESIDUE).all())
        c = fp.Case(r)
        c.inp("in", ct3, 3 * Ld * n)
        c.inp("key", key, 2 * L * n)
        for k, z in enumerate(terms):
            c.inp(f"z{k}", z, 2 * z.shape[2] * n)
        c.inp("w", w, Ld)
        c.scratch("work", batch * 2 * L * n, 2 * L * n)
        c.out("out2", batch * 2 * (Ld - 1) * n, 2 * (Ld - 1) * n, reference(r, ct3, key, terms, w))
        limbs = fp.u32([z.shape[2] for z in terms])

        def call(at, K=K, batch=batch, limbs=limbs):
            ptrs = (C.c_void_p * max(K, 1))(*[at(f"z{k}") for k in range(K)])
            return lib.dpfhe_relinearize_lincomb_rescale_hybrid(h, at("out2"), at("in"), at("key"), at("work"), ptrs, limbs, K, at("w"), batch, at.stream)
        c.run(f"dpfhe_relinearize_lincomb_rescale_hybrid K = {K} x{batch}", call)


ARENA = [("pinned_ld4", 8), ("f64_under_fold", 12)]


@pytest.mark.parametrize("name,log2n", ARENA)
def test_footprint(rig, name, log2n):
    assert fp.Case.gate is None
    arena_cases(rig(name, log2n))


def test_device_entry_rejects_bad_arguments(rig):
    import torch
    r = rig("pinned_ld4", 8)
    lib, h, L, Ld, n = r.ctx._lib, r.ctx.handle, r.L, r.L - 1, r.n
    z = lambda *s: torch.zeros(s, dtype=torch.int64, device=r.ctx.device)
    out, in3, key, work, w = z(1, 2, Ld - 1, n), z(1, 3, Ld, n), z(Ld, 2, L, n), z(1, 2, L, n), z(4, Ld)
    t0, t1 = z(1, 2, Ld, n), z(1, 2, Ld + 2, n)
    f = lib.dpfhe_relinearize_lincomb_rescale_hybrid

    def rc(out=out, in3=in3, key=key, work=work, terms=(t0, t1), limbs=None, K=None, w=w, batch=1, skew=None):
        a = {k: (v.data_ptr() if v is not None else None) for k, v in dict(out=out, in3=in3, key=key, work=work, w=w).items()}
        if skew:
            a[skew] += 8
        ptrs = (C.c_void_p * 16)(*[t.data_ptr() if t is not None else None for t in terms])
        lm = fp.u32([t.shape[2] if t is not None else Ld for t in terms] if limbs is None else limbs)
        return f(h, a["out"], a["in3"], a["key"], a["work"], ptrs, lm, len(terms) if K is None else K, a["w"], batch, None)

    assert rc() == 0
    assert rc(batch=0) == 0 and rc(batch=0, out=None) == 0
    assert f(h, out.data_ptr(), in3.data_ptr(), key.data_ptr(), work.data_ptr(), None, None, 0, w.data_ptr(), 1, None) == 0      # no terms: no arrays
    assert f(h, out.data_ptr(), in3.data_ptr(), key.data_ptr(), work.data_ptr(), None, None, 1, w.data_ptr(), 1, None) == 2000
    for name in ("out", "in3", "key", "work", "w"):
        assert rc(**{name: None}) == 2000, name
        assert rc(skew=name) == 2000, name
    assert rc(terms=(t0, None)) == 2000
    many = tuple(z(1, 2, Ld, n) for _ in range(16))
    assert rc(terms=many[:15], w=z(17, Ld)) == 0 and rc(terms=many, w=z(18, Ld)) == 2000 and b"15" in lib.dpfhe_last_error()
    assert rc(limbs=[Ld, Ld - 1]) == 2000 and b"fewer limbs" in lib.dpfhe_last_error()
    for other in ("in3", "key", "work", "w"):
        assert rc(out=dict(in3=in3, key=key, work=work, w=w)[other]) == 2000, other                       # out overlaps ...
    assert rc(out=t1) == 2000 and rc(work=t1.view(-1)[: work.numel()]) == 2000                               # ... a term; work overlaps a term
    assert rc(work=in3) == 2000 and rc(work=key) == 2000
    assert rc(terms=(t0, t0)) == 0 and rc(terms=(in3.view(-1)[: t0.numel()].view_as(t0), t1)) == 0           # read-only buffers may alias each other
    torch.cuda.synchronize()
    two = fp.ParamsRig("two_limbs", fr.pinned(8, 2))                                                         # Ld = 1: nothing to drop
    one = fp.ParamsRig("one_limb", fr.pinned(8, 1))                                                          # no special prime
    try:
        assert rc() == 0
        h = two.ctx.handle
        assert rc() == 2002
        h = one.ctx.handle
        assert rc() == 2002
    finally:
        two.close()
        one.close()
    with pytest.raises(Exception):
        r.ev.relinearize_lincomb_rescale_hybrid(Ciphertext(in3), key, [t0], w)                               # w has K + 2 = 3 rows for one term
    torch.cuda.synchronize()
