"""-m gpu: hoisted slot sums on the device (include/dpfhe.h dpfhe_rotate_sum_hoisted; csrc/kernels_rotate_sum.h, workmap.h QpSumMap), word for word against the
oracle's parts: Oracle.rotate_hoisted_qp's blocks 1 .. R summed mod q_l in numpy, its inverse transform, class_edges.rescale_bsgs_reference with the input as
the one addend.  Inputs are Rig.words (stripes in item 0, q - 1 in every word of item 1 and of key 1).
arena_cases() is the footprint case and, run again by tests/test_gpu_stream_contract_rotate_sum.py with Case.gate set, the stream-contract case."""
import numpy as np
import pytest

import test_gpu_footprint as fp
from class_edges import CLASSES, adversarial_key, rescale_bsgs_reference
from deeppowers_amd.evaluator import Ciphertext, Context, Evaluator, to_host
from deeppowers_amd.params import FheParams

pytestmark = pytest.mark.gpu
rig = fp.rig

# a ring below one segment (one item; a tile + a remainder tile; a tile with 3 live rows; the cap); several segments per class, 9 (Ld + 1) terms; the mixture
# with a tile of 4 and one of 3; P of another class; composed transforms
SHAPES = ([("fold", 8, (1, 1)), ("fold", 8, (7, 5)), ("fold", 8, (3, 3)), ("fold", 8, (64, 2))] + [(k, 12, (9, 4)) for k in CLASSES + ("mixed",)]
          + [("mixed", 12, (9, 7)), ("f64_under_fold", 12, (3, 2)), ("fold", 14, (3, 2)), ("fold", 15, (3, 2))])
FOOTPRINT = [("fold", 8), ("f64_under_fold", 12), ("fold", 14)]


def inputs(r, R, T, seed):
    """(R elements, their keys, T items)"""
    n = r.n
    e = [3, pow(3, -1, 2 * n), 5, n + 1, 2 * n - 1, 2 * n - 3, pow(3, 77, 2 * n), 1, pow(3, n // 4, 2 * n)] + [pow(5, i, 2 * n) for i in range(2, R)]
    return e[:R], r.words(r.orc, (max(R, 2), r.L - 1, 2), seed)[:R], r.words(fp.data_oracle(r), (max(T, 2), 2), seed + 1)[:T]


def device_and_reference(r, cts, elts, keys):
    got = to_host(r.ev.rotate_sum_hoisted(Ciphertext(r.dev(cts)), elts, r.dev(keys)).data)
    return got, reference(r, cts, elts, keys)


def reference(r, cts, elts, keys):
    S = np.zeros((cts.shape[0], 2, r.L, r.n), np.uint64)
    for t in range(cts.shape[0]):
        for block in r.orc.rotate_hoisted_qp(cts[t], elts, keys, threads=0)[1:]:
            S[t] = (S[t] + block) % r.qcol                 # (below 2^61: no wrap)
    return rescale_bsgs_reference(r.orc, fp.data_oracle(r), r.orc.ntt_inv(S, threads=0), cts[None])


@pytest.mark.parametrize("kind,log2n,shape", SHAPES, ids=[f"{k}_n{1 << ln}_r{s[0]}x{s[1]}" for k, ln, s in SHAPES])
def test_rotate_sum_equals_the_oracle(rig, kind, log2n, shape):
    r = rig(kind, log2n)
    elts, keys, cts = inputs(r, *shape, 810)
    got, want = device_and_reference(r, cts, elts, keys)
    assert np.array_equal(got, want), (kind, log2n, shape, np.argwhere(got != want)[:4])
    if shape[0] == 1:      # the words of dpfhe_rotate_hybrid_hoisted followed by dpfhe_add, on the device
        dctx = Context(FheParams(r.p.log2_n, tuple(r.p.moduli[:-1]), tuple(r.p.psi[:-1])), 0)
        rot = r.ev.rotate_hybrid_hoisted(Ciphertext(r.dev(cts)), elts, r.dev(keys))
        got = to_host(Evaluator(dctx).add_words(r.dev(cts), rot.data))
        dctx.close()
        assert np.array_equal(got, want)


def test_adversarial_keys_fill_the_lazy_sums(rig):
    """fold, N = 8192, nine rotations of one item: rotation g's key is perm_g of the adversarial key of the item's digits, so every key product the kernel
    adds lazily is q - 1 (tests/test_gpu_digit_ladder.py holds adversarial_key to its claim)"""
    r = rig("fold", 13)
    (elts, _, cts), orc = inputs(r, 9, 1, 830), r.orc
    key = adversarial_key(orc, cts[0, 1], 831)[0]
    keys = np.stack([orc.ntt_fwd(orc.apply_galois(orc.ntt_inv(key, threads=0), g), threads=0) for g in elts])
    assert np.array_equal(*device_and_reference(r, cts, elts, keys))


def arena_cases(r, shapes=((3, 1), (5, 5))):
    """every buffer carved out of one arena at 16-byte alignment between guard bands, scratch at exactly the header's sizes"""
    lib, h, L, n, Ld = r.ctx._lib, r.ctx.handle, r.L, r.n, r.L - 1
    for R, T in shapes:
        elts, keys, cts = inputs(r, R, T, 840)
        c = fp.Case(r)
        c.inp("in2", cts, 2 * Ld * n)
        c.inp("keys", keys, Ld * 2 * L * n)
        for name, item in (("in_ntt", 2 * Ld * n), ("digits", Ld * L * n), ("sum_qp", 2 * L * n)):
            c.scratch(name, T * item, item)
        c.out("out2", T * 2 * Ld * n, 2 * Ld * n, reference(r, cts, elts, keys))
        c.run(f"dpfhe_rotate_sum_hoisted {R} rotations x{T}",
              lambda at: lib.dpfhe_rotate_sum_hoisted(h, at("out2"), at("in2"), T, fp.u32(elts), at("keys"), R, at("in_ntt"), at("digits"), at("sum_qp"), at.stream))


def test_footprint(rig):
    for kind, log2n in FOOTPRINT:
        arena_cases(rig(kind, log2n))


def test_device_entry_rejects_bad_arguments(rig):
    import torch
    r = rig("fold", 8)
    lib, h, L, Ld, n = r.ctx._lib, r.ctx.handle, r.L, r.L - 1, r.n
    fill = lambda *s: torch.full(s, 7, dtype=torch.int64, device=r.ctx.device)
    t = {"out": fill(1, 2, Ld, n), "in": fill(1, 2, Ld, n), "keys": fill(65, Ld, 2, L, n), "in_ntt": fill(1, 2, Ld, n), "digits": fill(1, Ld, L, n), "sum_qp": fill(1, 2, L, n)}
    a = dict({k: v.data_ptr() for k, v in t.items()}, elts=fp.u32([3] * 65), n_rot=2)

    def call(handle=h, items=1, **kw):
        b = dict(a, **kw)
        return lib.dpfhe_rotate_sum_hoisted(handle, b["out"], b["in"], items, b["elts"], b["keys"], b["n_rot"], b["in_ntt"], b["digits"], b["sum_qp"], None)
    assert call(n_rot=0) == call(n_rot=65) == call(elts=fp.u32([3, 4])) == call(elts=fp.u32([2 * n + 1, 3])) == 2000      # the cap; even, >= 2N
    for name in t:
        assert call(**{name: a[name] + 8}) == 2000 and call(**{name: None}) == 2000               # misaligned, null
    assert call(out=a["in"]) == call(sum_qp=a["digits"]) == call(in_ntt=a["in"]) == call(items=1 << 40) == 2000      # overlaps; a grid too large for one launch
    lone = Context(FheParams(8, tuple(r.p.moduli[:1]), tuple(r.p.psi[:1])), 0)                   # no special prime
    code = call(handle=lone.handle)
    lone.close()
    torch.cuda.synchronize()
    assert code == 2002 and call(items=0) == 0 and bool((t["out"] == 7).all())                    # every refusal left the output untouched
