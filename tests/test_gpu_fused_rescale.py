"""-m gpu: the fused rescales on the device (include/dpfhe.h dpfhe_relinearize_rescale_hybrid, dpfhe_lincomb_rescale; csrc/fused_rescale.h, the kernels in
csrc/kernels_keyswitch.h).

dpfhe_relinearize_rescale_hybrid against the ORACLE, word for word: orc.rescale(orc.keyswitch_hybrid(ct3, key, 3)) - the fused path at N = 256 (one partial
chunk) and N = 4096 on the pinned fold primes at Ld = 2 (one output limb) and Ld = 4 and on a mixed-class context, the composed path at N = 16384; batches
1 and 3; and the 6 x 6 planted edges of tests/test_fused_rescale_cpu.py, reached through the whole entry: the key is solved (tests/remainder_edges.py
key_for_targets) so that item 0's key-switched sums ARE a chosen polynomial whose special-limb words sit on the edges of P, and the free input words on the
last data limb are solved so that the intermediate word there lands on the edges of q_last.  The oracle confirms both before the device is asked.
dpfhe_lincomb_rescale against the host twin (which tests/test_fused_rescale_cpu.py holds to Python integers) on the CPU test's shapes.
arena_cases() is the footprint case, and - run again by tests/test_gpu_stream_contract_fused_rescale.py with Case.gate set - the stream-contract case."""
import numpy as np
import pytest

import class_edges
import fused_rescale_ref as fr
import remainder_edges as re_
import test_gpu_footprint as fp
from deeppowers_amd import _cabi
from deeppowers_amd.evaluator import Ciphertext, to_host
from deeppowers_amd.params import ntt_primes

pytestmark = pytest.mark.gpu

FUSED = [("pinned_ld2", 8), ("pinned_ld4", 8), ("pinned_ld2", 12), ("pinned_ld4", 12), ("f64_under_fold", 12)]
COMPOSED = [("fold_ld2", 14)]
LINCOMB = [(name, ln) for ln in (8, 10) for name in ("pinned_ld2", "pinned_ld4", "shoup", "f64_under_fold")]


def params(name, log2n):
    if name.startswith("pinned_ld"):
        return fr.pinned(log2n, int(name[9:]) + 1)
    if name == "fold_ld2":
        return ntt_primes(log2n, 3)
    return class_edges.edge_moduli(name, log2n)


@pytest.fixture
def rig():
    made = []

    def make(name, log2n):
        r = fp.ParamsRig(name, params(name, log2n))
        made.append(r)
        return r
    yield make
    for r in made:
        r.close()


def reference(r, ct3, key):
    """the two entries of the parent, by the oracle: the hybrid relinearisation on the extended context, then the rescale on the data context"""
    return fp.data_oracle(r).rescale(r.orc.keyswitch_hybrid(ct3, key, 3, threads=0))


def device(r, ct3, key):
    import torch
    out = r.ev.relinearize_rescale_hybrid(Ciphertext(r.dev(ct3)), r.dev(key))
    torch.cuda.synchronize()
    return to_host(out.data)


@pytest.mark.parametrize("name,log2n", FUSED + COMPOSED, ids=fp.ids(FUSED + COMPOSED))
def test_relinearize_rescale_hybrid_equals_the_oracle(rig, name, log2n):
    r = rig(name, log2n)
    Ld, data = r.L - 1, fp.data_oracle(r)
    assert r.ctx.uses_fold == name.startswith(("pinned", "fold"))
    key = r.words(r.orc, (Ld, 2), 41)
    for batch in ((1,) if (name, log2n) in COMPOSED else (1, 3)):
        ct3 = r.words(data, (batch, 3), 50 + batch)
        got, want = device(r, ct3, key), reference(r, ct3, key)
        assert got.shape == want.shape == (batch, 2, Ld - 1, r.n)
        assert np.array_equal(got, want), (name, log2n, batch, np.argwhere(got != want)[:4])


def planted(r, batch, seed):
    """(ct3, key, plan): item 0's sums over Q P are a chosen polynomial S whose special-limb words at coefficients 0 .. 35 are P_EDGES[j // 6], and
    (c0, c1) on the last data limb there are solved so that the intermediate word is T_EDGES[j % 6]"""
    orc, p, L, Ld, n = r.orc, r.p, r.L, r.L - 1, r.n
    data = fp.data_oracle(r)
    P, ql = p.moduli[-1], p.moduli[Ld - 1]
    ct3 = data.fill(batch * 3, seed).reshape(batch, 3, Ld, n)
    S = orc.fill(2, seed + 1).reshape(2, L, n)
    plan = [(j, fr.edge_value(fr.P_EDGES[j // 6], P, ql), fr.edge_value(fr.T_EDGES[j % 6], P, ql)) for j in range(36)]
    for j, wp, _ in plan:
        S[:, L - 1, j] = wp
    x = re_.digit_transforms(orc, ct3[0, 2])
    tgt = orc.fill(Ld * 2, seed + 2).reshape(Ld, 2, L, n)
    total = orc.ntt_fwd(S, threads=0)
    for j in range(Ld - 1):
        total = re_.sub(orc, total, np.ascontiguousarray(tgt[j]))
    tgt[Ld - 1] = total
    key, zero = re_.key_for_targets(orc, x, tgt, orc.fill(Ld * 2, seed + 3).reshape(Ld, 2, L, n))
    assert not zero.any()
    # the oracle's own sums for item 0 are S
    c2_only = np.zeros((1, 2, Ld, n), np.uint64)
    c2_only[0, 1] = ct3[0, 2]
    assert np.array_equal(orc.ntt_inv(orc.switch_key_qp(c2_only, key, threads=0), threads=0)[0], S)
    for c in range(2):
        rdiv = fr.divide_by_p(p.moduli, S[c])
        for j, _, t in plan:
            ct3[0, c, Ld - 1, j] = (t - int(rdiv[j])) % ql
    mid = orc.keyswitch_hybrid(ct3, key, 3, threads=0)
    for c in range(2):
        assert [int(mid[0, c, Ld - 1, j]) for j, _, _ in plan] == [t for _, _, t in plan]
    return ct3, key, plan


@pytest.mark.parametrize("name,log2n", [("pinned_ld2", 8), ("pinned_ld4", 8), ("f64_under_fold", 8)])
def test_relinearize_rescale_hybrid_planted_edges(rig, name, log2n):
    r = rig(name, log2n)
    ct3, key, plan = planted(r, 2, 77)
    assert len({(wp, t) for _, wp, t in plan}) == 36
    got, want = device(r, ct3, key), reference(r, ct3, key)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    # and the last pass alone, on the same sums: the host twin
    S = r.orc.ntt_inv(r.orc.switch_key_qp(np.ascontiguousarray(ct3[:, 1:]), key, threads=0), threads=0)
    assert np.array_equal(fr.relin_rescale_pass_twin(r.p, S, ct3), want)


@pytest.mark.parametrize("name,log2n", LINCOMB, ids=fp.ids(LINCOMB))
def test_lincomb_rescale_equals_the_host_twin(rig, name, log2n):
    import torch
    r = rig(name, log2n)
    cases = [(K, 2 if K <= 2 else 1, False) for K in (1, 2, 15, 16)] + [(3, 3, False), (16, 1, True)]
    for K, batch, full in cases:
        x, w = fr.lincomb_inputs(r.p, K, batch, 100 * K + log2n, full=full)
        got = r.ev.lincomb_rescale(r.dev(x), r.dev(w))
        torch.cuda.synchronize()
        want = fr.lincomb_rescale_twin(r.p, x, w)
        assert np.array_equal(to_host(got), want), (name, log2n, K, batch, full)


def arena_cases(r):
    """both entries with every buffer carved out of one arena at 16-byte (not 32-byte) alignment between guard bands of a whole item, d_work at exactly
    batch * 2 * L * N words"""
    lib, h, L, n, orc = r.ctx._lib, r.ctx.handle, r.L, r.n, r.orc
    Ld, data = L - 1, fp.data_oracle(r)
    key = r.words(orc, (Ld, 2), 303)
    for batch in (1, 3):
        ct3 = r.words(data, (batch, 3), 313)
        c = fp.Case(r)
        c.inp("in", ct3, 3 * Ld * n)
        c.inp("key", key, 2 * L * n)
        c.scratch("work", batch * 2 * L * n, 2 * L * n)
        c.out("out2", batch * 2 * (Ld - 1) * n, 2 * (Ld - 1) * n, reference(r, ct3, key))
        c.run(f"dpfhe_relinearize_rescale_hybrid x{batch}",
              lambda at: lib.dpfhe_relinearize_rescale_hybrid(h, at("out2"), at("in"), at("key"), at("work"), batch, at.stream))
    for K, batch in ((3, 3), (16, 1)):
        x, w = fr.lincomb_inputs(r.p, K, batch, 7 + K)
        c = fp.Case(r)
        c.inp("x", x, 2 * L * n)
        c.inp("w", w, L)
        c.out("out", batch * 2 * (L - 1) * n, 2 * (L - 1) * n, fr.lincomb_rescale_twin(r.p, x, w))
        c.run(f"dpfhe_lincomb_rescale K = {K} x{batch}", lambda at: lib.dpfhe_lincomb_rescale(h, at("out"), at("x"), at("w"), K, batch, at.stream))


@pytest.mark.parametrize("name,log2n", [("pinned_ld4", 8), ("f64_under_fold", 12)])
def test_footprint(rig, name, log2n):
    assert fp.Case.gate is None
    arena_cases(rig(name, log2n))


def test_device_entries_reject_bad_arguments(rig):
    import torch
    r = rig("pinned_ld2", 8)
    p, lib, h, L, Ld, n = r.p, r.ctx._lib, r.ctx.handle, r.L, r.L - 1, r.n
    z = lambda *s: torch.zeros(s, dtype=torch.int64, device=r.ctx.device)
    out, in3, key, work = z(1, 2, Ld - 1, n), z(1, 3, Ld, n), z(Ld, 2, L, n), z(1, 2, L, n)
    a = (out.data_ptr(), in3.data_ptr(), key.data_ptr(), work.data_ptr())
    f = lib.dpfhe_relinearize_rescale_hybrid
    assert f(h, *a, 1, None) == 0
    assert f(h, a[0] + 8, a[1], a[2], a[3], 1, None) == 2000                      # misaligned
    assert f(h, None, a[1], a[2], a[3], 1, None) == 2000
    assert f(h, a[1], a[1], a[2], a[3], 1, None) == 2000                          # out overlaps in
    assert f(h, a[3], a[1], a[2], a[3], 1, None) == 2000                          # out overlaps work
    two = fp.ParamsRig("two_limbs", fr.pinned(8, 2))                              # Ld = 1: nothing to drop
    try:
        assert f(two.ctx.handle, *a, 1, None) == 2002
    finally:
        two.close()
    x, w, o = z(2, 1, 2, L, n), z(3, L), z(1, 2, L - 1, n)
    g = lib.dpfhe_lincomb_rescale
    assert g(h, o.data_ptr(), x.data_ptr(), w.data_ptr(), 2, 1, None) == 0
    assert g(h, o.data_ptr(), x.data_ptr(), w.data_ptr(), 0, 1, None) == 2000 and g(h, o.data_ptr(), x.data_ptr(), w.data_ptr(), 17, 1, None) == 2000
    assert g(h, o.data_ptr(), x.data_ptr(), w.data_ptr(), 2, 0, None) == 2000
    assert g(h, x.data_ptr(), x.data_ptr(), w.data_ptr(), 2, 1, None) == 2000
    assert g(h, o.data_ptr() + 8, x.data_ptr(), w.data_ptr(), 2, 1, None) == 2000
    assert g(h, o.data_ptr(), x.data_ptr(), None, 2, 1, None) == 2000
    one = fp.ParamsRig("one_limb", fr.pinned(8, 1))
    try:
        assert g(one.ctx.handle, o.data_ptr(), x.data_ptr(), w.data_ptr(), 2, 1, None) == 2002
    finally:
        one.close()
    with pytest.raises(_cabi.DpfheError):
        r.ev.lincomb_rescale(x, w[:2].contiguous())
    torch.cuda.synchronize()
