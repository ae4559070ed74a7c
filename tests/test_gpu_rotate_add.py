"""-m gpu: the rotate-and-add ladder on the device (include/dpfhe.h dpfhe_rotate_add_hybrid; csrc/rotate_add.h, the last pass in csrc/kernels_rotate.h).

Against the ORACLE's own composition, word for word and step by step: data.apply_galois, orc.keyswitch_hybrid(.., 2), a modular add - and against the
device's existing entries, dpfhe_rotate_hybrid_grouped + dpfhe_add.  The fused key switch at N = 256 (one partial chunk) and N = 4096 on the pinned fold
primes at Ld = 2 and Ld = 4 and on a mixed-class context, generic primes at N = 1024, the composed key products at N = 16384 and N = 32768 (the last pass
gathers from global memory above N = 8192: workmap.h kRotateAddStagedMaxN); 1 and 3 steps, 1 and 3 items, the elements of tests/test_rotate_add_cpu.py.
A transparent input (c1 = 0) whose c0 words make c0 + sigma(c0) land on 0, 1, q - 1 and wrap; and the planted words of the CPU test reached through the
whole entry: the key is solved (tests/remainder_edges.py key_for_targets) so that item 0's key products ARE the planted polynomial, which the oracle
confirms before the device is asked.
arena_cases() is the footprint case, and - run again by tests/test_gpu_stream_contract_rotate_add.py with Case.gate set - the stream-contract case."""
import numpy as np
import pytest

import class_edges
import fused_rescale_ref as fr
import remainder_edges as re_
import rotate_add_ref as ra
import test_gpu_footprint as fp
from deeppowers_amd.evaluator import Ciphertext, Context, Evaluator, to_host
from deeppowers_amd.params import FheParams, ntt_primes

pytestmark = pytest.mark.gpu

FUSED = [("pinned_ld2", 8), ("pinned_ld4", 8), ("pinned_ld2", 12), ("pinned_ld4", 12), ("f64_under_fold", 12), ("shoup", 10)]
COMPOSED = [("fold_ld2", 14), ("fold_ld2", 15)]
ALL_SHAPES = ((3, 1), (3, 3), (1, 1), (1, 3))      # (steps, items)
COMPOSED_SHAPES = ((3, 1), (1, 3))


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


def ladder_elements(n, steps):
    """three steps: 3, 3^(N/4), 2N - 3; one step: 2N - 1 - together the elements of the CPU test"""
    e = ra.elements(n)
    return [e[0], e[1], e[3]] if steps == 3 else [e[2]]


def reference(r, ct, elts, keys):
    """the ladder by the oracle's entries: the automorphism on the data context, the hybrid key switch on the extended one, a modular add"""
    data = fp.data_oracle(r)
    acc = np.ascontiguousarray(ct)
    for g, key in zip(elts, keys):
        rot = data.apply_galois(acc.reshape(-1, data.L, r.n), g).reshape(acc.shape)
        ks = r.orc.keyswitch_hybrid(rot, np.ascontiguousarray(key), 2, threads=0)
        acc = data.dyadic("add", acc.reshape(-1, data.L, r.n), ks.reshape(-1, data.L, r.n), threads=0).reshape(acc.shape)
    return acc


def device(r, ct, elts, keys):
    import torch
    out = r.ev.rotate_add_hybrid(Ciphertext(r.dev(ct)), elts, r.dev(keys))
    torch.cuda.synchronize()
    return to_host(out.data)


def device_composed(r, ct, elts, keys):
    """the parent's entries on the device: dpfhe_rotate_hybrid_grouped (one element, every item in its group) and dpfhe_add on the data context"""
    import torch
    p = r.p
    dctx = Context(FheParams(p.log2_n, tuple(p.moduli[:-1]), tuple(p.psi[:-1])), 0)
    try:
        dev_ = Evaluator(dctx)
        acc, dk = Ciphertext(r.dev(ct)), r.dev(keys)
        for i, g in enumerate(elts):
            rot = r.ev.rotate_hybrid_grouped(acc, [g], ct.shape[0], dk[i:i + 1])
            acc = Ciphertext(dev_.add_words(acc.data, rot.data))
        torch.cuda.synchronize()
        return to_host(acc.data)
    finally:
        dctx.close()


@pytest.mark.parametrize("name,log2n", FUSED + COMPOSED, ids=fp.ids(FUSED + COMPOSED))
def test_rotate_add_equals_the_oracle_and_the_composed_entries(rig, name, log2n):
    r = rig(name, log2n)
    Ld, data = r.L - 1, fp.data_oracle(r)
    assert r.ctx.uses_fold == name.startswith(("pinned", "fold"))
    for steps, batch in (COMPOSED_SHAPES if (name, log2n) in COMPOSED else ALL_SHAPES):
        elts = ladder_elements(r.n, steps)
        keys = r.words(r.orc, (steps, Ld, 2), 41 + steps)
        ct = r.words(data, (batch, 2), 50 + batch)
        got, want = device(r, ct, elts, keys), reference(r, ct, elts, keys)
        assert got.shape == want.shape == (batch, 2, Ld, r.n)
        assert np.array_equal(got, want), (name, log2n, steps, batch, np.argwhere(got != want)[:4])
        assert np.array_equal(device_composed(r, ct, elts, keys), want), (name, log2n, steps, batch)


@pytest.mark.parametrize("name,log2n", [("pinned_ld2", 8), ("shoup", 10), ("pinned_ld4", 12)])
def test_transparent_input_sums_land_on_the_edges(rig, name, log2n):
    """c1 = 0: every digit is zero, every key product is zero, the division by P gives 0 - the output is (c0 + sigma_g(c0), 0), and the planted pairs of
    {0, 1, q - 1} make that sum 0, 1, q - 1, and wrap (q - 1 + 1 = 0, 2 q - 2 = q - 2)"""
    r = rig(name, log2n)
    Ld, g = r.L - 1, 3
    _, ct, plan = ra.pass_inputs(r.p, 2, 19, g)
    ct[:, 1] = 0
    keys = r.words(r.orc, (1, Ld, 2), 23)
    want = reference(r, ct, [g], keys)
    assert not want[:, 1].any()
    for l, q in enumerate(r.p.moduli[:Ld]):
        sums = {int(want[0, 0, l, k]) for k, *_ in plan}
        assert sums == {0, 1, 2, q - 1, q - 2}, (l, sorted(sums))     # 0 + 0, 0 + 1, 1 + 1, (q - 1) + 0 and the wraps: 1 + (q - 1) = 0, 2 q - 2 = q - 2, ...
    assert np.array_equal(device(r, ct, [g], keys), want)


def planted(r, batch, seed, g):
    """(ct, key, S, plan): item 0's key products over Q P are the polynomial S that rotate_add_ref.pass_inputs plants (round(S / P), c0[k] and the gathered
    word over {0, 1, q - 1}^3 at a plain and a negated position, the special-limb words on the edges of P)"""
    orc, L, Ld, n = r.orc, r.L, r.L - 1, r.n
    data = fp.data_oracle(r)
    work, ct, plan = ra.pass_inputs(r.p, batch, seed, g)
    S = np.ascontiguousarray(work[0])
    rot = data.apply_galois(np.ascontiguousarray(ct[0]), g)                        # [2][Ld][N]: the digits are sigma_g(c1)
    x = re_.digit_transforms(orc, rot[1])
    tgt = orc.fill(Ld * 2, seed + 2).reshape(Ld, 2, L, n)
    total = orc.ntt_fwd(S, threads=0)
    for j in range(Ld - 1):
        total = re_.sub(orc, total, np.ascontiguousarray(tgt[j]))
    tgt[Ld - 1] = total
    key, zero = re_.key_for_targets(orc, x, tgt, orc.fill(Ld * 2, seed + 3).reshape(Ld, 2, L, n))
    assert not zero.any()
    # the oracle's own products for item 0 are S, and the integers reach every planted combination on them
    assert np.array_equal(orc.ntt_inv(orc.switch_key_qp(rot[None], key, threads=0), threads=0)[0], S)
    return ct, key, S, plan


@pytest.mark.parametrize("name,log2n", [("pinned_ld2", 8), ("pinned_ld4", 8), ("f64_under_fold", 8)])
def test_rotate_add_planted_edges(rig, name, log2n):
    r = rig(name, log2n)
    g = 3
    ct, key, S, plan = planted(r, 2, 77, g)
    got = ra.reached(r.p, S[None], ct, g, plan)
    assert len({c[:4] for c in got}) == 54 and {c[4] for c in got} == set(fr.P_EDGES)
    want = reference(r, ct, [g], key[None])
    assert np.array_equal(device(r, ct, [g], key[None]), want)
    # and the last pass alone, on the oracle's products of every item: the host twin
    rot = fp.data_oracle(r).apply_galois(ct.reshape(-1, r.L - 1, r.n), g).reshape(ct.shape)
    sums = r.orc.ntt_inv(r.orc.switch_key_qp(rot, key, threads=0), threads=0)
    assert np.array_equal(ra.pass_twin(r.p, sums, ct, g), want)


def arena_cases(r, shapes=ALL_SHAPES):
    """every buffer carved out of one arena at 16-byte (not 32-byte) alignment between guard bands of a whole item, d_work at exactly batch * 2 * L * N words,
    d_acc at exactly batch * 2 * Ld * N - and NULL where there is one step"""
    lib, h, L, n, orc = r.ctx._lib, r.ctx.handle, r.L, r.n, r.orc
    Ld, data = L - 1, fp.data_oracle(r)
    ct_words = 2 * Ld * n
    for steps, batch in shapes:
        elts = ladder_elements(n, steps)
        keys = r.words(orc, (steps, Ld, 2), 303 + steps)
        ct = r.words(data, (batch, 2), 313 + batch)
        c = fp.Case(r)
        c.inp("in2", ct, ct_words)
        c.inp("keys", keys, Ld * 2 * L * n)
        c.scratch("work", batch * 2 * L * n, 2 * L * n)
        if steps > 1:
            c.scratch("acc", batch * ct_words, ct_words)
        c.out("out2", batch * ct_words, ct_words, reference(r, ct, elts, keys))
        c.run(f"dpfhe_rotate_add_hybrid {steps} steps x{batch}",
              lambda at: lib.dpfhe_rotate_add_hybrid(h, at("out2"), at("in2"), fp.u32(elts), at("keys"), at("work"), at("acc") if steps > 1 else None, steps, batch,
                                                     at.stream))


FOOTPRINT = [("pinned_ld4", 8, ALL_SHAPES), ("f64_under_fold", 12, ALL_SHAPES), ("fold_ld2", 14, COMPOSED_SHAPES)]


@pytest.mark.parametrize("name,log2n,shapes", FOOTPRINT, ids=fp.ids([f[:2] for f in FOOTPRINT]))
def test_footprint(rig, name, log2n, shapes):
    assert fp.Case.gate is None
    arena_cases(rig(name, log2n), shapes)


def test_device_entry_rejects_bad_arguments(rig):
    import torch
    r = rig("pinned_ld2", 8)
    lib, h, L, Ld, n = r.ctx._lib, r.ctx.handle, r.L, r.L - 1, r.n
    z = lambda *s: torch.zeros(s, dtype=torch.int64, device=r.ctx.device)
    out, in2, keys, work, acc = z(1, 2, Ld, n), z(1, 2, Ld, n), z(2, Ld, 2, L, n), z(1, 2, L, n), z(1, 2, Ld, n)
    a = [out.data_ptr(), in2.data_ptr(), fp.u32([3, 9]), keys.data_ptr(), work.data_ptr(), acc.data_ptr()]
    f = lib.dpfhe_rotate_add_hybrid

    def call(steps=2, batch=1, **kw):
        b = list(a)
        for i, v in kw.items():
            b[int(i[1:])] = v
        return f(h, *b, steps, batch, None)
    assert call() == 0 and call(steps=1, _5=None) == 0 and call(batch=0) == 0
    assert call(steps=0) == 2000
    assert call(_5=None) == 2000                                       # two steps need d_acc
    assert call(_0=None) == 2000 and call(_1=None) == 2000 and call(_2=None) == 2000 and call(_3=None) == 2000 and call(_4=None) == 2000
    for i in (0, 1, 3, 4, 5):
        assert call(**{f"_{i}": a[i] + 8}) == 2000                     # misaligned
    assert call(_2=fp.u32([3, 4])) == 2000 and call(_2=fp.u32([2 * n + 1, 3])) == 2000      # even, >= 2N
    assert call(_0=a[1]) == 2000 and call(_0=a[4]) == 2000 and call(_5=a[0]) == 2000 and call(_5=a[1]) == 2000 and call(_4=a[1]) == 2000   # overlaps
    assert call(batch=1 << 40) == 2000                                 # a grid too large for one launch
    one = fp.ParamsRig("one_limb", fr.pinned(8, 1))                    # no special prime
    try:
        assert f(one.ctx.handle, *a, 2, 1, None) == 2002
    finally:
        one.close()
    with pytest.raises(Exception):
        r.ev.rotate_add_hybrid(Ciphertext(in2), [3, 9], keys[:1].contiguous())
    torch.cuda.synchronize()
