"""-m gpu: the device words against tests/golden/sympy_anchor.json - words sympy alone produced at the metric rings (tests/golden/make_golden.py
sympy_anchor).  This file does not import oracle/: inputs come from the fixture's seeds (tests/sympy_anchor.py restates splitmix64 with numpy), expected
words from the fixture, and everything runs through the C ABI (deeppowers_amd.evaluator is its ctypes mirror).  All comparisons are bit for bit."""
import numpy as np
import pytest

import sympy_anchor as sa
from deeppowers_amd.params import FheParams

FOLD_NAMES = ("fold", "pinned0", "pinned1", "pinned2", "pinned3", "pinned4")
CLASS_NAMES = ("fold", "f64", "fold_scaled", "f64_wide", "shoup")
HALVES_MIN_POLYS, QUARTERS_MIN_POLYS = 2304, 768      # launch.h kHalvesMinPolys / kQuartersMinPolys (residue polynomials, fold contexts)
CACHE_BYTES = 256 << 20                               # launch.h kInfinityCacheBytes: a fold transform at N = 4096 / 8192 that touches more runs non-temporal


def _by_name(log2n):
    out = {}
    for r in sa.transform_records(log2n):
        out.setdefault(r["name"], []).append(r)
    return out


def _groups():
    """(log2n, the primes of one context): every anchored prime alone, the five class primes together (per-limb classes: ntt_classes_kernel) and the
    pinned primes of the ring together (a fold context of several limbs)"""
    out = []
    for log2n in sa.TRANSFORM_LOG2NS:
        names = list(_by_name(log2n))
        out += [(log2n, (nm,)) for nm in names]
        if log2n <= 13:
            out.append((log2n, CLASS_NAMES))
        pinned = tuple(nm for nm in names if nm.startswith("pinned"))
        if len(pinned) > 1:
            out.append((log2n, pinned))
    return out


def tile_counts(log2n, L, fold):
    """RNS polynomials per tiled batch: past every threshold at which launch_ntt changes the kernel form of a fold context (just below and at the halves /
    quarters thresholds; past 256 MiB touched in place - out of place touches twice as much - at N = 4096, 8192 and, in quarters form, 16384), else a
    batch of three"""
    if not fold or log2n >= 15:
        return (3,)
    up = lambda residue_polys: -(-residue_polys // L)
    past_cache = CACHE_BYTES // (8 << log2n) + 1
    if log2n == 12:
        return (up(past_cache),)
    if log2n == 13:
        return (up(HALVES_MIN_POLYS) - 1, up(HALVES_MIN_POLYS), up(past_cache))
    return (up(QUARTERS_MIN_POLYS) - 1, up(QUARTERS_MIN_POLYS), up(past_cache // 2 + 1))


@pytest.mark.gpu
@pytest.mark.parametrize("log2n,names", _groups(), ids=lambda v: "+".join(v) if isinstance(v, tuple) else "n%d" % (1 << v))
def test_transform_anchors(log2n, names):
    """forward and inverse, in place and out of place, as a one-polynomial batch and tiled past the thresholds that change the kernel form: every tiled
    item equals item 0 on the device, item 0 and the last item are held to the anchor on the host"""
    import torch
    from deeppowers_amd.evaluator import Context, Evaluator, to_device, to_host
    by_name = _by_name(log2n)
    n, L = 1 << log2n, len(names)
    p = FheParams(log2n, tuple(by_name[nm][0]["q"] for nm in names), tuple(by_name[nm][0]["psi"] for nm in names))
    ctx = Context(p, 0)
    ev = Evaluator(ctx)
    try:
        fold = all(nm in FOLD_NAMES for nm in names)
        if fold:
            assert ctx.limb_classes == ("fold",) * L
        elif log2n <= 14 and (L > 1 or names[0] != "shoup"):
            assert ctx.limb_classes == names          # the class primes run on their own class
        else:
            assert ctx.limb_classes == ("shoup",) * L
        # limb l of the k-th buffer is the k-th record of prime l: the primes of one context carry the same (input kind, direction) in the same order
        assert len({len(by_name[nm]) for nm in names}) == 1
        for k in range(len(by_name[names[0]])):
            recs = [by_name[nm][k] for nm in names]
            assert len({(r["direction"], r["input"]) for r in recs}) == 1
            inverse = recs[0]["direction"] == "inv"
            x = np.stack([sa.fill(r["input"], r["seed"], [r["q"]], n)[0] for r in recs])
            run_oop = ev.ntt_inverse if inverse else ev.ntt_forward
            run_inplace = ev.ntt_inverse_ if inverse else ev.ntt_forward_

            def held(words, where):
                for l, r in enumerate(recs):
                    sa.assert_anchor(r, words[l], n, where)

            one = to_device(x[None], ctx.device)
            held(to_host(run_oop(one))[0], "one polynomial, out of place")
            held(to_host(run_inplace(one.clone()))[0], "one polynomial, in place")
            for count in tile_counts(log2n, L, fold):
                tiled = one.expand(count, L, n).contiguous()
                for where, got in (("out of place", run_oop(tiled)), ("in place", run_inplace(tiled.clone()))):
                    assert torch.equal(got, got[:1].expand_as(got)), (count, where)
                    held(to_host(got[0]), "%d tiled, %s, item 0" % (count, where))
                    held(to_host(got[count - 1]), "%d tiled, %s, last item" % (count, where))
                del tiled, got
    finally:
        ctx.close()


# ---- the tensor product -------------------------------------------------------------------------------------------------------------------------------
MULTIPLY = sa.fixture()["multiply"]


def _mul_ctx(r):
    from deeppowers_amd.evaluator import Context, Evaluator
    ctx = Context(FheParams(r["log2n"], tuple(r["moduli"]), tuple(r["psi"])), 0)
    return ctx, Evaluator(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("r", MULTIPLY, ids=lambda r: r["name"])
def test_multiply_anchors(r):
    """dpfhe_ct_mul(flags = 0) at every anchored case; on the pinned primes every form set_ct_mul_variant offers; at the metric pair whose transforms are
    anchored the other three flag combinations; and that pair tiled to a batch of 13 - no multiple of 8 - so that it is also held at the end of a batch"""
    import torch
    from deeppowers_amd.evaluator import Ciphertext, to_device, to_host
    n = 1 << r["log2n"]
    a, b = sa.multiply_operands(r)
    ctx, ev = _mul_ctx(r)
    try:
        A, B = Ciphertext(to_device(a[None], ctx.device)), Ciphertext(to_device(b[None], ctx.device))
        sa.assert_anchor(r, to_host(ev.multiply(A, B).data), n, "flags 0")
        if r["name"].startswith("metric"):
            assert ctx.variants() == ["quad", "dual"]
            for form in ("dual", "quad"):
                ctx.set_ct_mul_variant(form)
                sa.assert_anchor(r, to_host(ev.multiply(A, B).data), n, form)
        if "ntt_c" in r:
            An, Bn = (Ciphertext(ev.ntt_forward(v.data), is_ntt=True) for v in (A, B))
            sa.assert_anchor(r["ntt_a"], to_host(An.data), n, "the operand's transform")
            sa.assert_anchor(r["ntt_b"], to_host(Bn.data), n, "the operand's transform")
            sa.assert_anchor(r["ntt_c"], to_host(ev.multiply(A, B, out_ntt=True).data), n, "DPFHE_OUT_NTT")
            sa.assert_anchor(r, to_host(ev.multiply(An, Bn, out_ntt=False).data), n, "DPFHE_IN_NTT")
            sa.assert_anchor(r["ntt_c"], to_host(ev.multiply(An, Bn, out_ntt=True).data), n, "DPFHE_IN_NTT | DPFHE_OUT_NTT")
            batch = 13
            got = ev.multiply(Ciphertext(A.data.expand(batch, *a.shape).contiguous()), Ciphertext(B.data.expand(batch, *b.shape).contiguous())).data
            assert torch.equal(got, got[:1].expand_as(got))
            sa.assert_anchor(r, to_host(got[0]), n, "item 0 of 13")
            sa.assert_anchor(r, to_host(got[batch - 1]), n, "item 12 of 13")
    finally:
        ctx.close()


@pytest.mark.gpu
def test_multiply_forms_at_n8192_on_the_pinned_prime():
    """"quad" and "dual" at N = 8192: the pinned limb of the anchored N = 8192 pair in a fold context of its own, against that limb's digests"""
    from deeppowers_amd.evaluator import Ciphertext, Context, Evaluator, to_device, to_host
    r = next(r for r in MULTIPLY if r["name"] == "n8192_pinned_f64")
    n, L = 1 << r["log2n"], len(r["moduli"])
    a, b = sa.multiply_operands(r)
    ctx = Context(FheParams(r["log2n"], (r["moduli"][0],), (r["psi"][0],)), 0)
    ev = Evaluator(ctx)
    try:
        assert ctx.limb_classes == ("fold",) and ctx.variants() == ["quad", "dual"]
        A, B = (Ciphertext(to_device(v[None, :, :1], ctx.device)) for v in (a, b))
        for form in ("quad", "dual"):
            ctx.set_ct_mul_variant(form)
            got = to_host(ev.multiply(A, B).data)[0]
            for comp in range(3):
                assert sa.digest(got[comp, 0]) == r["poly_sha256"][comp * L], (form, comp)
    finally:
        ctx.close()


# ---- integer operations and key switching at N = 4096 on the metric configuration -----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c", sa.fixture()["integer"]["cases"], ids=lambda c: c["op"] + "-" + c["input"])
def test_integer_operation_anchors(c):
    from deeppowers_amd.evaluator import Context, Evaluator, to_device, to_host
    fx = sa.fixture()["integer"]
    n = 1 << fx["log2n"]
    ctx = Context(FheParams(fx["log2n"], tuple(fx["moduli"]), tuple(fx["psi"])), 0)
    ev = Evaluator(ctx)
    try:
        x = to_device(sa.fill(c["input"], c["seed"], fx["moduli"], n)[None], ctx.device)
        if c["op"] == "rescale":
            got = ev.rescale_words(x)
        elif c["op"] == "base_extend":
            src = x[:, c["src_limb0"]:c["src_limb0"] + c["n_src"]].contiguous()
            got = ev.base_extend(src, c["src_limb0"], c["dst_limb0"], c["n_dst"])
        else:
            got = ev.scale_round(x, c["drop_limb0"], c["n_drop"], c["keep_limb0"], c["n_keep"], c["multiplier"])
        sa.assert_anchor(c, to_host(got), n, "device")
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("c", sa.fixture()["keyswitch"]["cases"], ids=lambda c: c["op"] + "-" + c["input"])
def test_key_switching_anchors(c):
    """dpfhe_relinearize on 4 limbs and dpfhe_switch_key_hybrid on 3 data limbs plus P, from the header's formulas (a digit [c]_{q_j} is limb j read in
    [0, q_j)); the keys are uniform words in the NTT domain"""
    from deeppowers_amd.evaluator import Ciphertext, Context, Evaluator, to_device, to_host
    fx = sa.fixture()["keyswitch"]
    n, moduli = 1 << fx["log2n"], fx["moduli"]
    L = len(moduli)
    ctx = Context(FheParams(fx["log2n"], tuple(moduli), tuple(fx["psi"])), 0)
    ev = Evaluator(ctx)
    try:
        if c["op"] == "relinearize":
            ct = sa.fill(c["input"], c["seed"], moduli * 3, n).reshape(1, 3, L, n)
            key = sa.fill("random", c["key_seed"], sa.key_moduli(moduli, L), n).reshape(L, 2, L, n)
            got = ev.relinearize(Ciphertext(to_device(ct, ctx.device)), to_device(key, ctx.device))
        else:
            ct = sa.fill(c["input"], c["seed"], moduli[:L - 1] * 2, n).reshape(1, 2, L - 1, n)
            key = sa.fill("random", c["key_seed"], sa.key_moduli(moduli, L - 1), n).reshape(L - 1, 2, L, n)
            got = ev.keyswitch_hybrid(Ciphertext(to_device(ct, ctx.device)), to_device(key, ctx.device))      # 2 components: dpfhe_switch_key_hybrid
        sa.assert_anchor(c, to_host(got.data), n, "device")
    finally:
        ctx.close()


# ---- the Galois identity ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("log2n,names,which", [(12, CLASS_NAMES, g) for g in range(4)] + [(16, ("pinned4",), g) for g in range(4)],
                         ids=lambda v: "+".join(v) if isinstance(v, tuple) else str(v))
def test_galois_identity(log2n, names, which):
    """(sigma_g a)(rho) = a(rho^g) at 32 sampled rho = psi^odd per limb, by Horner's rule on Python integers, applied to dpfhe_apply_galois and - a being
    the device's inverse transform of the anchored input, itself held to its anchor here - to dpfhe_ntt_inv_galois, out of place and in place"""
    from deeppowers_amd.evaluator import Context, Evaluator, to_device, to_host
    by_name = _by_name(log2n)
    n, L = 1 << log2n, len(names)
    g = sa.galois_elements(n)[which]
    recs = [next(r for r in by_name[nm] if r["direction"] == "inv" and r["input"] == "random") for nm in names]
    ctx = Context(FheParams(log2n, tuple(r["q"] for r in recs), tuple(r["psi"] for r in recs)), 0)
    ev = Evaluator(ctx)
    try:
        x = to_device(np.stack([sa.fill("random", r["seed"], [r["q"]], n)[0] for r in recs])[None], ctx.device)
        a_dev = ev.ntt_inverse(x)
        a = to_host(a_dev)[0]
        for l, r in enumerate(recs):
            sa.assert_anchor(r, a[l], n, "inverse transform")
        rotated = to_host(ev.apply_galois_words(a_dev, g))[0]
        fused = to_host(ev.ntt_inverse_galois(x, [g]))[0]
        inplace = x.clone()
        ev.ntt_inverse_galois(inplace, [g], out=inplace)
        assert np.array_equal(to_host(inplace)[0], fused)
        for l, r in enumerate(recs):
            assert sa.galois_identity_failures(a[l], rotated[l], g, r["q"], r["psi"], 1000 + l) == [], ("dpfhe_apply_galois", names[l], g)
            assert sa.galois_identity_failures(a[l], fused[l], g, r["q"], r["psi"], 2000 + l) == [], ("dpfhe_ntt_inv_galois", names[l], g)
    finally:
        ctx.close()
