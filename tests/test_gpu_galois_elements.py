"""-m gpu: every Galois-taking entry of include/dpfhe.h along the ELEMENT, word for word against the oracle compositions the entries' own modules use
(apply_galois, then keyswitch_hybrid, rotate_hoisted, rotate_hoisted_qp or ntt_inv): the whole group {+-3^k} at N = 256 (and N = 1024 for the LDS gather of
dpfhe_ntt_inv_galois), tests/galois_elements.py edge_elements - the 2-adic families g = +-1 mod 2^j, the slot-sum ladders' 3^(+-2^k), the elements next to 2N -
at the rings where a kernel takes another path:

  entry                          every element                                   edge_elements
  dpfhe_ntt_inv_galois           N = 256 (position path), N = 1024 (LDS gather,   N = 4096, 8192, 16384 (one piece); N = 32768, 65536 (split; in place through
    out of place and in place    16 launch groups), fold; N = 1024 mixed classes  the stream's arena)
  dpfhe_apply_galois             N = 256                                          N = 8192, 16384, 65536
  dpfhe_rotate_hybrid_batch      N = 256                                          N = 8192 (gather staged in LDS), N = 16384 (gather from global memory), Ld = 1
    n_in = 1 and n_in = batch
  dpfhe_rotate_hybrid_grouped    N = 256, groups of 2                             N = 8192, groups of 2 (the same kernel, the element per group)
  dpfhe_rotate_hybrid_hoisted    N = 256                                          N = 4096, 8192 (fused kernels); N = 16384 (composed)
    2 tokens
  dpfhe_rotate_hoisted_qp        N = 256 at L = 3 (up-front form) and L = 9       N = 1024 mixed classes; N = 8192, 16384
    2 tokens                     (stream form)
  dpfhe_rotate_add_hybrid        N = 256: eight ladders of 32 steps, every        N = 8192, 16384: one single-step call per element
    2 items                      element once as a step

The elements of a case always go in ONE call where the entry takes a list, so the launch groups of 64 elements are crossed (edge_elements has 67 at
N = 8192).  Keys are orc.fill words; one ciphertext component is q - 1 in every word; inputs are distinct per item up to N = 4096 and three base inputs cycled
above.  Contexts are the smallest that reach the branch: two or three fold limbs unless the table says otherwise.  What decides each map on the host and in
the NTT domain is enumerated on the CPU (tests/test_galois_elements_cpu.py); the coefficient-domain gathers of kernels_rotate.h run only here."""
import numpy as np
import pytest

import galois_elements as ge
import test_gpu_bsgs_qp as bq
from class_edges import Rig
from deeppowers_amd.params import ntt_primes
from oracle.cbind import Oracle

pytestmark = pytest.mark.gpu


@pytest.fixture
def rig():
    made = []

    def make(kind, ln, L=2):
        r = Rig(bq._params("mixed")) if kind == "mixed" else Rig(ntt_primes(ln, L))
        assert r.p.log2_n == ln
        if kind == "mixed":
            assert r.ctx.limb_classes == bq.MIXED_CLASSES
        else:
            assert r.ctx.uses_fold and r.L == L
        r.data = Oracle(ln, r.p.moduli[:-1], r.p.psi[:-1])
        made.append(r)
        return r
    yield make
    for r in made:
        r.close()


def elements(ln, which):
    return ge.all_elements(ln) if which == "all" else ge.edge_elements(ln)


def case_id(case):
    return "-".join(f"n{1 << v}" if i == 1 else str(v) for i, v in enumerate(case))


def inputs(orc, count, lead, seed):
    """(base [m][*lead][L][N], index [count]): item i of a case is base[index[i]] - distinct items up to N = 4096, three base items cycled above; component
    lead - 1 of base item 1 (of item 0 when there is one item) is q - 1 in every word"""
    m = count if orc.n <= 4096 else min(count, 3)
    base = orc.fill(m * lead, seed).reshape(m, lead, orc.L, orc.n)
    base[min(1, m - 1), lead - 1] = np.array(orc.moduli, np.uint64)[:, None] - np.uint64(1)
    return base, np.arange(count) % m


def wrong(got, want, elts, per=1):
    """the elements whose words differ (got, want: [len(elts) * per]...)"""
    return [g for e, g in enumerate(elts) if not np.array_equal(got[e * per:(e + 1) * per], want[e * per:(e + 1) * per])]


# ---- dpfhe_ntt_inv_galois ------------------------------------------------------------------------------------------------------------------------------------
NTT_CASES = [("fold", 8, "all"), ("fold", 10, "all"), ("mixed", 10, "all"), ("fold", 12, "edge"), ("fold", 13, "edge"), ("fold", 14, "edge"),
             ("fold", 15, "edge"), ("fold", 16, "edge")]


@pytest.mark.parametrize("kind,ln,which", NTT_CASES, ids=[case_id(c) for c in NTT_CASES])
def test_ntt_inverse_galois(rig, kind, ln, which):
    from deeppowers_amd.evaluator import to_host
    r = rig(kind, ln)
    orc, L, n, ev = r.orc, r.L, r.n, r.ev
    elts = elements(ln, which)
    k = len(elts)
    base, idx = inputs(orc, k, 1, 1300 + ln)
    inv = orc.ntt_inv(base, threads=0)
    want = np.stack([orc.apply_galois(inv[i], g) for i, g in zip(idx, elts)])              # [k][1][L][N]
    x = base[idx]
    d = r.dev(x)
    got = to_host(ev.ntt_inverse_galois(d, elts))
    assert wrong(got, want, elts) == [], "out of place"
    assert np.array_equal(to_host(d), x), "the input of an out-of-place call changed"
    ev.ntt_inverse_galois(d, elts, out=d)
    assert wrong(to_host(d), want, elts) == [], "in place"
    if ln >= 15:
        assert r.ctx.scratch_bytes >= 64 * L * n * 8                                      # a launch group of 64 elements was staged in the arena


# ---- dpfhe_apply_galois --------------------------------------------------------------------------------------------------------------------------------------
APPLY_CASES = [(8, "all"), (13, "edge"), (14, "edge"), (16, "edge")]


@pytest.mark.parametrize("ln,which", APPLY_CASES, ids=[f"n{1 << ln}-{w}" for ln, w in APPLY_CASES])
def test_apply_galois_words(rig, ln, which):
    import torch
    from deeppowers_amd.evaluator import to_host
    r = rig("fold", ln)
    orc = r.orc
    x, _ = inputs(orc, 3, 1, 1400 + ln)
    x[2, 0, :, 0::5] = 0                                                                  # the sign of zero
    d = r.dev(x)
    out = torch.empty_like(d)
    bad = []
    for g in elements(ln, which):
        out.zero_()
        r.ev.apply_galois_words(d, g, out=out)
        if not np.array_equal(to_host(out), orc.apply_galois(x, g)):
            bad.append(g)
    assert bad == []
    assert np.array_equal(to_host(d), x)


# ---- dpfhe_rotate_hybrid_batch, dpfhe_rotate_hybrid_grouped ----------------------------------------------------------------------------------------------------
BATCH_CASES = [(8, 3, "all"), (13, 2, "edge"), (14, 2, "edge")]


def rotation_keys(r, k, seed):
    keys = r.orc.fill(k * (r.L - 1) * 2, seed).reshape(k, r.L - 1, 2, r.L, r.n)
    return keys, r.dev(keys)


@pytest.mark.parametrize("ln,L,which", BATCH_CASES, ids=[f"n{1 << ln}-l{L}-{w}" for ln, L, w in BATCH_CASES])
def test_rotate_hybrid_batch(rig, ln, L, which):
    from deeppowers_amd.evaluator import Ciphertext, to_host
    r = rig("fold", ln, L)
    orc, data = r.orc, r.data
    elts = elements(ln, which)
    k = len(elts)
    keys, dkeys = rotation_keys(r, k, 1500 + ln)
    base, idx = inputs(data, k, 2, 1510 + ln)
    # n_in = batch: item i under element i
    cts = base[idx]
    got = to_host(r.ev.rotate_hybrid_batch(Ciphertext(r.dev(cts)), elts, dkeys).data)
    w = np.stack([orc.keyswitch_hybrid(data.apply_galois(base[i:i + 1], g), keys[e], 2, threads=0)[0] for e, (i, g) in enumerate(zip(idx, elts))])
    assert wrong(got, w, elts) == [], "n_in = batch"
    # n_in = 1: THE item (the one with the q - 1 component) under every element
    one = base[min(1, len(base) - 1)][None]
    got = to_host(r.ev.rotate_hybrid_batch(Ciphertext(r.dev(one)), elts, dkeys).data)
    w = np.stack([orc.keyswitch_hybrid(data.apply_galois(one, g), keys[e], 2, threads=0)[0] for e, g in enumerate(elts)])
    assert wrong(got, w, elts) == [], "n_in = 1"


GROUPED_CASES = [(8, 3, "all"), (13, 2, "edge")]


@pytest.mark.parametrize("ln,L,which", GROUPED_CASES, ids=[f"n{1 << ln}-l{L}-{w}" for ln, L, w in GROUPED_CASES])
def test_rotate_hybrid_grouped(rig, ln, L, which):
    from deeppowers_amd.evaluator import Ciphertext, to_host
    r = rig("fold", ln, L)
    orc, data, T = r.orc, r.data, 2
    elts = elements(ln, which)
    k = len(elts)
    keys, dkeys = rotation_keys(r, k, 1520 + ln)
    base, idx = inputs(data, k * T, 2, 1530 + ln)
    got = to_host(r.ev.rotate_hybrid_grouped(Ciphertext(r.dev(base[idx])), elts, T, dkeys).data)
    w = np.concatenate([orc.keyswitch_hybrid(data.apply_galois(base[idx[e * T:(e + 1) * T]], g), keys[e], 2, threads=0) for e, g in enumerate(elts)])
    assert wrong(got, w, elts, per=T) == []


# ---- dpfhe_rotate_hybrid_hoisted -------------------------------------------------------------------------------------------------------------------------------
HOISTED_CASES = [(8, 3, "all"), (12, 3, "edge"), (13, 3, "edge"), (14, 2, "edge")]


@pytest.mark.parametrize("ln,L,which", HOISTED_CASES, ids=[f"n{1 << ln}-l{L}-{w}" for ln, L, w in HOISTED_CASES])
def test_rotate_hybrid_hoisted(rig, ln, L, which):
    from deeppowers_amd.evaluator import Ciphertext, to_host
    r = rig("fold", ln, L)
    orc, data, n, T = r.orc, r.data, r.n, 2
    elts = elements(ln, which)
    k = len(elts)
    keys, dkeys = rotation_keys(r, k, 1600 + ln)
    cts, _ = inputs(data, T, 2, 1610 + ln)
    got = to_host(r.ev.rotate_hybrid_hoisted(Ciphertext(r.dev(cts)), elts, dkeys).data).reshape(k, T, 2, L - 1, n)     # rotation-major
    for t in range(T):
        assert wrong(got[:, t], orc.rotate_hoisted(cts[t], elts, keys, threads=0), elts) == [], t


# ---- dpfhe_rotate_hoisted_qp -----------------------------------------------------------------------------------------------------------------------------------
QP_CASES = [("fold", 8, 3, "all"), ("fold", 8, 9, "all"), ("mixed", 10, 4, "edge"), ("fold", 13, 3, "edge"), ("fold", 14, 2, "edge")]


@pytest.mark.parametrize("kind,ln,L,which", QP_CASES, ids=[f"{kind}-n{1 << ln}-l{L}-{w}" for kind, ln, L, w in QP_CASES])
def test_rotate_hoisted_qp(rig, kind, ln, L, which):
    """L = 3: hoisted_qp_upfront_kernel (up to 6 digits); L = 9: hoisted_qp_stream_kernel (8 digits)"""
    from deeppowers_amd.evaluator import Ciphertext, to_host
    r = rig(kind, ln, L)
    assert r.L == L
    orc, data, n, T = r.orc, r.data, r.n, 2
    elts = elements(ln, which)
    k = len(elts)
    keys, dkeys = rotation_keys(r, k, 1700 + ln + L)
    cts, _ = inputs(data, T, 2, 1710 + ln + L)
    got = to_host(r.ev.rotate_hoisted_qp(Ciphertext(r.dev(cts)), elts, dkeys))
    assert got.shape == (k + 1, T, 2, L, n)
    for t in range(T):
        want = orc.rotate_hoisted_qp(cts[t], elts, keys, threads=0)
        assert np.array_equal(got[0, t], want[0]), (t, "identity block")
        assert wrong(got[1:, t], want[1:], elts) == [], t


# ---- dpfhe_rotate_add_hybrid -----------------------------------------------------------------------------------------------------------------------------------
def ladder_reference(r, ct, elts, keys):
    """acc <- acc + keyswitch_hybrid(sigma_g(acc), key), step by step, by the oracle's entries (tests/test_gpu_rotate_add.py reference)"""
    data = r.data
    acc = np.ascontiguousarray(ct)
    for g, key in zip(elts, keys):
        rot = data.apply_galois(acc.reshape(-1, data.L, r.n), g).reshape(acc.shape)
        ks = r.orc.keyswitch_hybrid(rot, np.ascontiguousarray(key), 2, threads=0)
        acc = data.dyadic("add", acc.reshape(-1, data.L, r.n), ks.reshape(-1, data.L, r.n), threads=0).reshape(acc.shape)
    return acc


def test_rotate_add_ladders_over_the_whole_group(rig):
    """N = 256: eight ladders of 32 steps; ladder j runs the elements 2 (8 i + j) + 1, so every ladder mixes both halves of the group"""
    from deeppowers_amd.evaluator import Ciphertext, to_host
    r = rig("fold", 8, 3)
    every = ge.all_elements(8)
    ct, _ = inputs(r.data, 2, 2, 1800)
    run = []
    for j in range(8):
        elts = every[j::8]
        assert len(elts) == 32
        run += elts
        keys, dkeys = rotation_keys(r, 32, 1810 + j)
        got = to_host(r.ev.rotate_add_hybrid(Ciphertext(r.dev(ct)), elts, dkeys).data)
        assert np.array_equal(got, ladder_reference(r, ct, elts, keys)), (j, elts)
    assert sorted(run) == every


ADD_CASES = [(13, 3), (14, 2)]


@pytest.mark.parametrize("ln,L", ADD_CASES, ids=[f"n{1 << ln}-l{L}" for ln, L in ADD_CASES])
def test_rotate_add_single_steps(rig, ln, L):
    """N = 8192: the last pass gathers sigma_g(c0) from LDS; N = 16384: from global memory, behind the composed key products"""
    from deeppowers_amd.evaluator import Ciphertext, to_host
    r = rig("fold", ln, L)
    elts = ge.edge_elements(ln)
    keys, dkeys = rotation_keys(r, len(elts), 1900 + ln)
    base, idx = inputs(r.data, len(elts) * 2, 2, 1910 + ln)
    dbase = r.dev(base)
    bad = []
    for e, g in enumerate(elts):
        pick = [int(idx[2 * e]), int(idx[2 * e + 1])]
        got = to_host(r.ev.rotate_add_hybrid(Ciphertext(dbase[pick].contiguous()), [g], dkeys[e:e + 1]).data)
        if not np.array_equal(got, ladder_reference(r, base[pick], [g], keys[e:e + 1])):
            bad.append(g)
    assert bad == []
