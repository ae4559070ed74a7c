"""-m gpu: every key-switching entry along the DIGIT COUNT, 1 to 40, through Evaluator against oracle.c.

The key-switching kernels pick their form and their lazy-reduction schedule from the number of digits (the data limbs of the context: L with RNS-digit
keys, Ld = L - 1 under a special prime); the rest of the suite moves along ring degree, class, prime edge and batch but stays below 10 digits.  The
rungs (class_edges.LADDER) stand on both sides of every rule that reads the digit count:

  relin_kernel<FoldArith>      lazy sums of mul60 products, reduced when 13 have been added: first at the 14th digit, then at the 26th and 38th
  launch_relin                 relin_shared_kernel for fold, 1024 <= N <= 4096, 4..7 digits; relin_kernel otherwise (and kLdsKeys key tiles at N = 8192)
  launch_hoisted_ks            hoisted_ks2_kernel (merged) for fold, Ld <= 7 and rotations x L x tokens >= 512; the split kernel otherwise
  dpfhe_rotate_hoisted_qp      hoisted_qp_upfront_kernel<LD> for Ld 1..6, hoisted_qp_stream_kernel from 7; Dot30 column sums folded every 8 terms
  per-limb classes             L <= 16 (16 nibbles of active_map); 17 limbs run on the context-wide policy

Every comparison is a whole buffer, word for word, against the oracle (threads=0), which reduces after every product whatever the digit count and is
held to Python integers at 8, 14 and 17 limbs by tests/test_digit_ladder_cpu.py.  Inputs are Rig.words - stripes in item 0, q - 1 in every word of
item 1, ciphertexts and keys - and, on the fold rungs, ADVERSARIAL keys (class_edges.adversarial_key): random words would never fill a lazy sum
(17 random products are about 8.5 q, a word holds 16 q), and q - 1 in the inputs does not either, the products being taken in the NTT domain; these
keys make every lazily added product of item 0 the word q - 1, so the schedule runs at the worst case it was designed for.  One case = one entry on
one rung; a rung's context and keys are built once and shared by its cases."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from class_edges import LADDER, Rig, adversarial_key, chain_classes, edge_chain, rescale_bsgs_reference
from oracle.cbind import Oracle

pytestmark = pytest.mark.gpu

ENTRIES_RNS = ("relinearize", "apply_galois")                                      # L digits
ENTRIES_P = ("keyswitch_hybrid", "rotate_hybrid_batch", "rotate_hybrid_grouped", "rotate_hybrid_hoisted", "switch_key_qp_1x3", "switch_key_qp_9x2",
             "rotate_hoisted_qp")                                                   # L - 1 digits
ENTRIES_FOLD = ("adversarial_relinearize", "adversarial_switch_key_qp", "adversarial_keyswitch_hybrid")
CASES = [(rung, e) for rung in LADDER
         for e in ENTRIES_RNS + (ENTRIES_P if rung[2] >= 2 else ()) + (ENTRIES_FOLD[:1 if rung[2] < 2 else 3] if rung[0] == "fold" else ())]
IDS = [f"{k}_n{1 << ln}_l{L}-{e}" for (k, ln, L), e in CASES]


class LadderRig(Rig):
    """the context of one rung, with the key material its cases share"""

    def __init__(self, kind, log2n, L):
        super().__init__(edge_chain(kind, log2n, L))
        classes = chain_classes(kind, L)
        if kind == "fold":
            assert self.ctx.uses_fold and self.ctx.limb_classes == ("fold",) * L
        elif L <= 16:
            assert self.ctx.limb_classes == classes, (kind, L, self.ctx.limb_classes)      # per-limb classes: all 16 nibbles of the active-limb map
        else:
            assert self.ctx.limb_classes == ("shoup",) * L, (kind, L, self.ctx.limb_classes)
        self.data = Oracle(log2n, self.p.moduli[:-1], self.p.psi[:-1]) if L >= 2 else None
        self.batch = 2 if L * L * self.n > (1 << 21) else 3
        # the one rung on which a key alone is 200 MB (N = 8192, 40 limbs): the smallest batches that still reach every form - one or two rotations, one item
        # per key
        self.heavy = L * L * self.n > (1 << 23)
        self.max_keys = 16 if kind == "fold" and L in (8, 9) else 9
        self._made = {}

    def shared(self, name):
        """evk [L][2][L][N] / key [L-1][2][L][N]: (host, device), stripes in digit 0's key and q - 1 in every word of digit 1's"""
        if name == "key":
            base, dbase = self.shared("key_polys")
            return base[: self.L - 1], dbase[: self.L - 1]
        if name not in self._made:
            k = self.words(self.orc, (self.L if name == "evk" else self.L - 1 + self.max_keys - 1, 2), 900 + len(name))
            self._made[name] = (k, self.dev(k))
        return self._made[name]

    def rotation_keys(self, k):
        """k keys [L-1][2][L][N]: key i = digit keys i .. i + L - 2 of one run of L - 2 + max_keys of them (windows: every key differs from its neighbours
        in every digit, and nothing is filled or sent twice) -> (the host views, the device tensor [k][L-1][2][L][N])"""
        import torch
        assert k <= self.max_keys
        base, dbase = self.shared("key_polys")
        Ld = self.L - 1
        return [base[i:i + Ld] for i in range(k)], torch.stack([dbase[i:i + Ld] for i in range(k)])


@pytest.fixture(scope="module")
def rung_rig():
    held = {}

    def get(rung):
        if rung not in held:
            for r in held.values():
                r.close()
            held.clear()
            held[rung] = LadderRig(*rung)
        return held[rung]
    yield get
    for r in held.values():
        r.close()


def host(t):
    from deeppowers_amd.evaluator import to_host
    return to_host(t)


def elements(n, k):
    elts = [pow(3, i + 1, 2 * n) for i in range(k)]
    elts[-1] = 2 * n - 1
    return elts


# ---- the entries ---------------------------------------------------------------------------------------------------------------------------------------------
def relinearize(r):
    from deeppowers_amd.evaluator import Ciphertext
    evk, dk = r.shared("evk")
    c3 = r.words(r.orc, (r.batch, 3), 910)
    got = r.ev.relinearize(Ciphertext(r.dev(c3)), dk)
    assert np.array_equal(host(got.data), r.orc.relinearize(c3, evk, threads=0))


def apply_galois(r):
    from deeppowers_amd.evaluator import Ciphertext
    evk, dk = r.shared("evk")
    a = r.words(r.orc, (r.batch, 2), 911)
    for g in (5, 2 * r.n - 1):
        got = r.ev.apply_galois(Ciphertext(r.dev(a)), g, dk)
        assert np.array_equal(host(got.data), r.orc.switch_key(r.orc.apply_galois(a, g), evk, threads=0)), g


def keyswitch_hybrid(r):
    from deeppowers_amd.evaluator import Ciphertext
    key, dkey = r.shared("key")
    for comps in (2, 3):
        ct = r.words(r.data, (r.batch, comps), 912 + comps)
        got = r.ev.keyswitch_hybrid(Ciphertext(r.dev(ct)), dkey)
        assert np.array_equal(host(got.data), r.orc.keyswitch_hybrid(ct, key, comps, threads=0)), comps


def rotate_hybrid_batch(r):
    from deeppowers_amd.evaluator import Ciphertext
    k, n, orc, data = 2 if r.heavy else 3, r.n, r.orc, r.data
    elts = elements(n, k)
    keys, dks = r.rotation_keys(k)
    cts = r.words(data, (2, 2), 920)[:1]
    got = host(r.ev.rotate_hybrid_batch(Ciphertext(r.dev(cts)), elts, dks).data)
    for i in range(k):
        assert np.array_equal(got[i], orc.keyswitch_hybrid(data.apply_galois(cts, elts[i]), keys[i], 2, threads=0)[0]), ("batch", i)


def rotate_hybrid_grouped(r):
    from deeppowers_amd.evaluator import Ciphertext
    k, T, n, orc, data = 2 if r.heavy else 3, 2, r.n, r.orc, r.data
    elts = elements(n, k)
    keys, dks = r.rotation_keys(k)
    items = r.words(data, (k * T, 2), 921)
    got = host(r.ev.rotate_hybrid_grouped(Ciphertext(r.dev(items)), elts, T, dks).data)
    for i in range(k):
        want = orc.keyswitch_hybrid(data.apply_galois(items[i * T:(i + 1) * T], elts[i]), keys[i], 2, threads=0)
        assert np.array_equal(got[i * T:(i + 1) * T], want), ("grouped", i)


def hoisted_shapes(kind, L):
    """(rotations, tokens): 3 x 2 everywhere; on the fold rungs with 8 and 9 limbs 16 x 4 - 512 (rotation, limb, token) tiles, so the merged kernel at
    Ld = 7 and, by the digit count alone, the split one at Ld = 8 - and with 8 limbs also 9 x 7: 504 tiles, the split kernel at Ld = 7"""
    shapes = [(3, 2)]
    if L >= 40:           # (one rotation of two tokens: at N = 8192 a key of 40 limbs is 200 MB)
        shapes = [(1, 2)]
    if kind == "fold" and L in (8, 9):
        shapes.append((16, 4))
    if kind == "fold" and L == 8:
        shapes.append((9, 7))
    return shapes


def rotate_hybrid_hoisted(r, kind):
    from deeppowers_amd.evaluator import Ciphertext
    n, Ld = r.n, r.L - 1
    for k, T in hoisted_shapes(kind, r.L):
        assert (k * r.L * T >= 512) == ((k, T) == (16, 4))
        elts = elements(n, k)
        keys, dks = r.rotation_keys(k)
        cts = r.words(r.data, (T, 2), 930 + k)
        got = host(r.ev.rotate_hybrid_hoisted(Ciphertext(r.dev(cts)), elts, dks).data).reshape(k, T, 2, Ld, n)
        keys = np.stack(keys)
        for t in range(T):
            assert np.array_equal(got[:, t], r.orc.rotate_hoisted(cts[t], elts, keys, threads=0)), (k, T, t)


def switch_key_qp(r, k, group):
    from deeppowers_amd.evaluator import Ciphertext
    keys, dks = r.rotation_keys(k)
    items = r.words(r.data, (max(k * group, 2), 2), 940 + k)[: k * group]
    if k > 1:
        items[k * group - 1] = items[0]                    # the stripes under the last key as well
    got = host(r.ev.switch_key_qp(Ciphertext(r.dev(items)), dks, group))
    assert got.shape == (k * group, 2, r.L, r.n)
    # the oracle spreads the ITEMS of a call over its threads and a call takes one key: with several keys the calls run side by side instead, one thread each
    with ThreadPoolExecutor(k) as pool:
        wants = list(pool.map(lambda i: r.orc.switch_key_qp(items[i * group:(i + 1) * group], keys[i], threads=0 if k == 1 else 1), range(k)))
    for i in range(k):
        assert np.array_equal(got[i * group:(i + 1) * group], wants[i]), (k, group, i)


def switch_key_qp_1x3(r):
    switch_key_qp(r, 1, 2 if r.heavy else 3)


def switch_key_qp_9x2(r):
    """nine keys: the key-major order of workgroups (launch_relin: from eight keys, whatever the group)"""
    switch_key_qp(r, 9, 1 if r.heavy else 2)


def rotate_hoisted_qp(r):
    """every block against the oracle, then closed as the packed layers close it: inverse transform, division by P, the input added back"""
    from deeppowers_amd.evaluator import Ciphertext
    k, T, n, L, orc = 1 if r.heavy else 3, 2, r.n, r.L, r.orc
    elts = elements(n, k)
    keys, dks = r.rotation_keys(k)
    keys = np.stack(keys)
    cts = r.words(r.data, (T, 2), 950)
    dev_cts = r.dev(cts)
    blocks = r.ev.rotate_hoisted_qp(Ciphertext(dev_cts), elts, dks)
    got = host(blocks)
    assert got.shape == (k + 1, T, 2, L, n)
    want = np.stack([orc.rotate_hoisted_qp(cts[t], elts, keys, threads=0) for t in range(T)], axis=1)
    assert np.array_equal(got, want)
    last = blocks[k].clone()
    r.ev.ntt_inverse_(last)
    closed = host(r.ev.rescale_bsgs(last, dev_cts[None]))
    assert np.array_equal(closed, rescale_bsgs_reference(orc, r.data, orc.ntt_inv(want[k], threads=0), cts[None]))


# ---- adversarial keys (fold rungs) ---------------------------------------------------------------------------------------------------------------------------
def checked_adversarial_key(orc, digits, seed):
    """class_edges.adversarial_key with its own claims asserted: x e = q - 1 wherever x != 0 (by the oracle's modular multiply, itself held to Python
    integers on the CPU, where this product is also taken in Python integers), and at most 1 word in 1000 with x = 0"""
    key, x, n_zero = adversarial_key(orc, digits, seed)
    qcol = np.array(orc.moduli, np.uint64)[:, None]
    prod = orc.dyadic("mul", x, np.ascontiguousarray(key[:, 0]), threads=0)
    assert np.array_equal(key[:, 0], key[:, 1])
    assert bool(((prod == qcol - np.uint64(1)) | (x == 0)).all())
    assert n_zero * 1000 <= x.size, (n_zero, x.size)
    return key, n_zero


def constant_words(moduli, value, n):
    return np.array([[value % q] * n for q in moduli], np.uint64)


def adversarial_relinearize(r):
    """L digits: every product relin_kernel / relin_shared_kernel adds for item 0 is q - 1; the sum is the constant -L in the NTT domain, so the result
    is (c0, c1) with coefficient 0 lowered by L"""
    from deeppowers_amd.evaluator import Ciphertext
    orc, L = r.orc, r.L
    c3 = r.words(orc, (r.batch, 3), 960)
    evk, n_zero = checked_adversarial_key(orc, c3[0, 2], 961)
    want = orc.relinearize(c3, evk, threads=0)
    if n_zero == 0:
        closed = c3[0, :2].copy()
        closed[:, :, 0] = (closed[:, :, 0] + (r.qcol[:, 0] - np.uint64(L))) % r.qcol[:, 0]
        assert np.array_equal(want[0], closed)
    got = r.ev.relinearize(Ciphertext(r.dev(c3)), r.dev(evk))
    assert np.array_equal(host(got.data), want)
    a = c3[:, 1:].copy()                                  # the same digits as component 1 of a 2-component item: dpfhe_switch_key (MODE 1), g = 1
    got = r.ev.apply_galois(Ciphertext(r.dev(a)), 1, r.dev(evk))
    assert np.array_equal(host(got.data), orc.switch_key(a, evk, threads=0))


def adversarial_hybrid_key(r):
    """the adversarial key of the rung's Ld digit polynomials (component 1 of item 0 of one fixed fill), built once: (digits, key, device key, n_zero)"""
    if "adversarial" not in r._made:
        digits = r.words(r.data, (2, 2), 970)[0, 1].copy()
        key, n_zero = checked_adversarial_key(r.orc, digits, 971)
        r._made["adversarial"] = (digits, key, r.dev(key), n_zero)
    return r._made["adversarial"]


def adversarial_switch_key_qp(r):
    """Ld digits on L limbs: every product relin_kernel MODE 4 adds for item 0 is q - 1, and it returns the constant -Ld in every word of that item"""
    from deeppowers_amd.evaluator import Ciphertext
    orc, data, Ld, n = r.orc, r.data, r.L - 1, r.n
    digits, key, dkey, n_zero = adversarial_hybrid_key(r)
    items = r.words(data, (2 if r.heavy else 3, 2), 972)
    items[0, 1] = digits
    want = orc.switch_key_qp(items, key, threads=0)
    if n_zero == 0:
        assert np.array_equal(want[0], np.stack([constant_words(r.p.moduli, -Ld, n)] * 2))
    got = host(r.ev.switch_key_qp(Ciphertext(r.dev(items)), dkey[None], items.shape[0]))
    assert np.array_equal(got, want)


def adversarial_keyswitch_hybrid(r):
    """the same key under MODE 2 / 3: divided by P the sum, Q P - Ld, rounds to Q = 0, so keyswitch_hybrid returns (c0, 0) for two components and
    (c0, c1) for three"""
    from deeppowers_amd.evaluator import Ciphertext
    orc, data = r.orc, r.data
    digits, key, dkey, n_zero = adversarial_hybrid_key(r)
    for comps in (2, 3):
        ct = r.words(data, (r.batch, comps), 973 + comps)
        ct[0, comps - 1] = digits
        want = orc.keyswitch_hybrid(ct, key, comps, threads=0)
        if n_zero == 0:
            closed = ct[0, :2].copy()
            if comps == 2:
                closed[1] = 0
            assert np.array_equal(want[0], closed), comps
        got = r.ev.keyswitch_hybrid(Ciphertext(r.dev(ct)), dkey)
        assert np.array_equal(host(got.data), want), comps


RUN = {f.__name__: f for f in (relinearize, apply_galois, keyswitch_hybrid, rotate_hybrid_batch, rotate_hybrid_grouped, switch_key_qp_1x3, switch_key_qp_9x2,
                              rotate_hoisted_qp, adversarial_relinearize, adversarial_switch_key_qp, adversarial_keyswitch_hybrid)}


@pytest.mark.parametrize("rung,entry", CASES, ids=IDS)
def test_key_switching_along_the_digit_count(rung_rig, rung, entry):
    r = rung_rig(rung)
    if entry == "rotate_hybrid_hoisted":
        rotate_hybrid_hoisted(r, rung[0])
    else:
        RUN[entry](r)
