"""The primes at the edges of the per-limb arithmetic classes (deeppowers_amd/csrc/tables.h limb_class), and the one Python statement of that rule.

Each class admits primes by a numeric rule whose bound is the one its lazy arithmetic needs, so the margin is smallest at the edge of the rule.
`catalogue(log2n)` lists, for a ring degree, the primes = 1 mod 2N nearest each bound: name -> [(q, psi), ...] ordered from the bound inward (up to
four, as many as exist; psi the smallest primitive 2N-th root).  An entry with no prime at this N is absent.

  fold_edge        2^60 - d with the largest d < 2^24            fold_near      2^60 - d with the smallest d (for contrast)
  shoup60          the largest primes below 2^60 - 2^24 (just outside fold: the widest words the generic path takes)
  fscaled_edge_k   2^k - d0 with the largest admitted d0 (d0 2^(60-k) < 2^24), 48 <= k <= 59
  fscaled_out_k    the next primes below fscaled_edge_k's band: f64_wide for k <= 50, shoup for k >= 51
  f64_edge         the largest primes below 2^47                 f64_wide_low   the smallest primes at or above 2^47 that fold_scaled does not take
  f64_wide_edge    the largest primes below 2^50 that fold_scaled does not take
  shoup_above_k    the smallest primes above 2^k, k in {50, 59} (the upper half of a scaling chain)
  smallest         the smallest primes = 1 mod 2N
"""
import functools

import numpy as np

from deeppowers_amd.params import FheParams, is_prime, min_primitive_2n_root
from oracle.cbind import Oracle

FSCALED_KS = tuple(range(48, 60))
SHOUP_ABOVE_KS = (50, 59)
PER_ENTRY = 4


def expected_class(q):
    """tables.h limb_class, restated: the arithmetic a limb of prime q runs on (in a context that has per-limb classes)"""
    if q < (1 << 60) and (1 << 60) - q < (1 << 24):
        return "fold"
    if q < (1 << 47):
        return "f64"
    k = q.bit_length()
    if 48 <= k <= 59 and (((1 << k) - q) << (60 - k)) < (1 << 24):
        return "fold_scaled"
    if q < (1 << 50):
        return "f64_wide"
    return "shoup"


def worst_case(x, qcol, n):
    """stripes of extreme residues in the first item: q - 1 everywhere in one stretch, alternating q - 1 / 0 in another, the half point in a third"""
    x[0, ..., : n // 8] = qcol - np.uint64(1)
    x[0, ..., n // 8: n // 4: 2] = qcol - np.uint64(1)
    x[0, ..., n // 8 + 1: n // 4: 2] = 0
    x[0, ..., n // 4: n // 4 + n // 8] = qcol // np.uint64(2)
    return x


def _first_at_or_above(v, two_n):
    """the smallest q = 1 mod 2N with q >= v"""
    return v + (1 - v) % two_n


def _first_at_or_below(v, two_n):
    """the largest q = 1 mod 2N with q <= v"""
    return v - (v - 1) % two_n


def _walk(start, stop, step, two_n, want=None, count=PER_ENTRY):
    """primes q = 1 mod 2N from `start` (itself = 1 mod 2N) towards `stop` (exclusive) in steps of +-2N, of class `want` if given"""
    out, q = [], start
    while len(out) < count and (q < stop if step > 0 else q > stop):
        if q > 2 and is_prime(q) and (want is None or expected_class(q) == want):
            out.append(q)
        q += step * two_n
    return out


def neighbour(q, log2n, direction):
    """the next prime = 1 mod 2N after q in `direction` (+1 up, -1 down), or None (none below 2^60 / above 2)"""
    two_n = 2 << log2n
    found = _walk(q + direction * two_n, (1 << 60) if direction > 0 else 2, direction, two_n, count=1)
    return found[0] if found else None


@functools.lru_cache(maxsize=None)
def catalogue_moduli(log2n):
    """name -> tuple of primes (see the module docstring), without the roots"""
    two_n = 2 << log2n
    up = lambda v, stop, want=None: _walk(_first_at_or_above(v, two_n), stop, +1, two_n, want)
    down = lambda v, stop, want=None: _walk(_first_at_or_below(v, two_n), stop, -1, two_n, want)
    cat = {
        "fold_edge": up((1 << 60) - (1 << 24) + 1, 1 << 60),
        "fold_near": down((1 << 60) - 1, (1 << 60) - (1 << 24)),
        "shoup60": down((1 << 60) - (1 << 24), 1 << 59),
        "f64_edge": down((1 << 47) - 1, 1 << 46),
        "f64_wide_low": up(1 << 47, 1 << 48, "f64_wide"),
        "f64_wide_edge": down((1 << 50) - 1, 1 << 49, "f64_wide"),
        "smallest": up(two_n + 1, 1 << 47),
    }
    for k in FSCALED_KS:
        band = 1 << (k - 36)                      # admitted: d0 = 2^k - q < 2^(k-36), i.e. d0 2^(60-k) < 2^24
        cat[f"fscaled_edge_{k}"] = up((1 << k) - band + 1, 1 << k)
        cat[f"fscaled_out_{k}"] = down((1 << k) - band, 1 << (k - 1))
    for k in SHOUP_ABOVE_KS:
        cat[f"shoup_above_{k}"] = up((1 << k) + 1, 1 << (k + 1))
    return {name: tuple(qs) for name, qs in cat.items() if qs}


@functools.lru_cache(maxsize=None)
def catalogue(log2n):
    """name -> tuple of (q, psi), ordered from the class bound inward"""
    n = 1 << log2n
    return {name: tuple((q, min_primitive_2n_root(n, q)) for q in qs) for name, qs in catalogue_moduli(log2n).items()}


def entry_class(name):
    """the class every prime of catalogue entry `name` must have (fscaled_out_k depends on k)"""
    if name.startswith("fscaled_out_"):
        return "f64_wide" if int(name.rsplit("_", 1)[1]) <= 50 else "shoup"
    if name.startswith("fscaled_edge_"):
        return "fold_scaled"
    if name.startswith("shoup"):
        return "shoup"
    return {"fold_edge": "fold", "fold_near": "fold", "f64_edge": "f64", "f64_wide_low": "f64_wide", "f64_wide_edge": "f64_wide", "smallest": "f64"}[name]


# ---- the edge contexts of the GPU tests (tests/test_gpu_class_edges.py, tests/test_gpu_packed_stage_edges.py) and of their CPU counterparts --------------------
CLASSES = ("fold", "f64", "fold_scaled", "f64_wide", "shoup")
FSCALED_ORDER = (59, 56, 50, 58, 57, 55, 54, 53, 52, 51, 49, 48)   # edge primes of several shifts, the widest scaling first

# the deployable hybrid shapes: kind -> (the data limbs, the catalogue entry whose first prime is the special prime P, the context's last limb)
MIXED_P = {
    "f64_under_fold": (lambda cat, first: list(cat["f64_edge"][:3]), "fold_edge"),
    "fold_scaled_under_shoup": (lambda cat, first: [e for k in FSCALED_ORDER for e in first(f"fscaled_edge_{k}")][:3], "shoup60"),
    "f64_wide_under_fold_scaled": (lambda cat, first: list(cat["f64_wide_edge"][:2]), "fscaled_edge_59"),
    "shoup_under_f64": (lambda cat, first: list(cat["shoup60"][:2]), "f64_edge"),            # P narrower than the data
    "fold_under_smallest": (lambda cat, first: list(cat["fold_edge"][:3]), "smallest"),      # fold data limbs that are not an all-fold context
}
MIXED_P_CLASSES = {
    "f64_under_fold": ("f64",) * 3 + ("fold",),
    "fold_scaled_under_shoup": ("fold_scaled",) * 3 + ("shoup",),
    "f64_wide_under_fold_scaled": ("f64_wide",) * 2 + ("fold_scaled",),
    "shoup_under_f64": ("shoup",) * 2 + ("f64",),
    "fold_under_smallest": ("fold",) * 3 + ("f64",),
}


def edge_moduli(kind, log2n):
    """the primes of an edge context: a uniform context of one class (2 - 4 primes nearest its bound), 'mixed' (one edge prime of every class plus
    shoup60, fscaled_out_50 and the smallest prime), 'shoup60' (the matvec context: the widest generic-path primes), a MIXED_P kind (the deployable
    hybrid shape: data limbs of one class under a special prime of another), or 'fold_scaled6' (five fold_scaled digits and a fold_scaled P)"""
    cat = catalogue(log2n)
    first = lambda name, i=0: [cat[name][i]] if name in cat and len(cat[name]) > i else []
    if kind == "fold":
        ps = list(cat["fold_edge"][:4])
    elif kind == "f64":
        ps = list(cat["f64_edge"][:3]) + first("smallest")
    elif kind == "fold_scaled":
        ps = [e for k in FSCALED_ORDER for e in first(f"fscaled_edge_{k}")][:4]
    elif kind == "f64_wide":
        ps = list(cat["f64_wide_edge"][:2]) + list(cat["f64_wide_low"][:2])
    elif kind == "shoup":
        ps = list(cat["shoup60"][:2]) + first("shoup_above_59") + first("shoup_above_50")
    elif kind == "shoup60":
        ps = list(cat["shoup60"][:2])
    elif kind == "fold2":
        ps = list(cat["fold_edge"][:2])
    elif kind == "mixed":
        ps = (first("fold_edge") + first("f64_edge") + first("fscaled_edge_59") + first("smallest") + first("shoup_above_50") + first("fscaled_out_50")
              + first("shoup60") + first("f64_wide_low"))
    elif kind in MIXED_P:
        data, special = MIXED_P[kind]
        ps = data(cat, first) + first(special)
    elif kind == "smallest":      # q far below 2^32, below a large plaintext modulus and any flood value (the host-twinned device operations); without
        ps = [e for e in cat["smallest"] if e[0] != 65537][:3]   # 65537 = 1 mod 2N itself: the packed layers' plaintext modulus must stay coprime to Q
    elif kind == "fold_scaled6":
        ps = [e for k in FSCALED_ORDER for e in first(f"fscaled_edge_{k}")][:4] + first("fscaled_edge_59", 1) + first("fscaled_edge_58", 1)
    else:
        raise ValueError(kind)
    assert len(ps) >= 2 and len({q for q, _ in ps}) == len(ps), (kind, log2n)   # (fscaled_out_50 is f64_wide_edge's first prime: the mixture takes f64_wide_low)
    return FheParams(log2n, tuple(q for q, _ in ps), tuple(w for _, w in ps))


# ---- digit ladders: contexts of any limb count (tests/test_gpu_digit_ladder.py, tests/test_digit_ladder_cpu.py) -----------------------------------------
CHAIN_KINDS = ("fold", "shoup", "f64", "fold_scaled", "f64_wide")
MIXED_CHAIN_ORDER = ("fold", "f64", "fold_scaled", "f64_wide", "shoup")     # limb i of mixed16 / mixed17 has class i mod 5: limb 15 is a fold limb


@functools.lru_cache(maxsize=None)
def chain_moduli(kind, log2n, count):
    """the `count` primes = 1 mod 2N of class `kind` nearest the class bound, in the catalogue's order (the first PER_ENTRY are the catalogue's own)"""
    two_n = 2 << log2n
    if kind == "fold":          # fold_edge: from the bound 2^60 - 2^24 upward
        qs = _walk(_first_at_or_above((1 << 60) - (1 << 24) + 1, two_n), 1 << 60, +1, two_n, count=count)
    elif kind == "shoup":       # shoup60: from just outside fold downward
        qs = _walk(_first_at_or_below((1 << 60) - (1 << 24), two_n), 1 << 59, -1, two_n, "shoup", count=count)
    elif kind == "f64":         # f64_edge
        qs = _walk(_first_at_or_below((1 << 47) - 1, two_n), 1 << 46, -1, two_n, count=count)
    elif kind == "f64_wide":    # f64_wide_edge
        qs = _walk(_first_at_or_below((1 << 50) - 1, two_n), 1 << 49, -1, two_n, "f64_wide", count=count)
    elif kind == "fold_scaled":  # fscaled_edge_k, four per shift: the edge prime of every shift (the widest scaling first), then the second of every shift, ...
        per = {k: _walk(_first_at_or_above((1 << k) - (1 << (k - 36)) + 1, two_n), 1 << k, +1, two_n, count=PER_ENTRY) for k in FSCALED_ORDER}
        qs = [per[k][i] for i in range(PER_ENTRY) for k in FSCALED_ORDER if len(per[k]) > i][:count]
    else:
        raise ValueError(kind)
    assert len(qs) == count and len(set(qs)) == count, (kind, log2n, count, len(qs))
    return tuple(qs)


def edge_chain(kind, log2n, count=None):
    """a context of `count` limbs at the edge of one class (CHAIN_KINDS), or 'mixed16' / 'mixed17': 16 / 17 limbs that cycle the five classes
    (MIXED_CHAIN_ORDER), each class's limbs its edge primes in order - limb 15, the top nibble of the active-limb map, is a fold limb"""
    if kind in ("mixed16", "mixed17"):
        total = int(kind[5:])
        assert count in (None, total)
        per = {c: chain_moduli(c, log2n, -(-total // len(MIXED_CHAIN_ORDER))) for c in MIXED_CHAIN_ORDER}
        qs = tuple(per[MIXED_CHAIN_ORDER[i % 5]][i // 5] for i in range(total))
        assert expected_class(qs[15]) != "shoup"
    else:
        qs = chain_moduli(kind, log2n, count)
    assert len(set(qs)) == len(qs)
    return FheParams(log2n, qs, tuple(min_primitive_2n_root(1 << log2n, q) for q in qs))


def chain_classes(kind, count):
    """the class of every limb of edge_chain(kind, log2n, count), by construction"""
    if kind in ("mixed16", "mixed17"):
        return tuple(MIXED_CHAIN_ORDER[i % 5] for i in range(int(kind[5:])))
    return (kind,) * count


# the rungs of tests/test_gpu_digit_ladder.py: (kind, log2 N, context limbs L).  RNS-digit keys give L digits, a special prime L - 1.
#   fold, N = 256: every L to 18 (relin_kernel reduces its lazy sums first at the 14th digit), then both sides of the reductions at digits 26 and 38
#   fold, N = 1024 / 4096: both sides of relin_shared_kernel's 4..7 digits, for L digits and for L - 1
#   fold, N = 8192: the LDS key tiles, hoisted_qp_upfront_kernel<6> / hoisted_qp_stream_kernel from 7, the Dot30 fold every 8 terms, 14+ digits, 17 limbs, 40
#   every other class, uniform: 8 digits, and 16 / 17 limbs (per-limb classes / the context-wide policy)
#   mixed16 / mixed17: every class in one context on both sides of that switch
LADDER = ([("fold", 8, L) for L in tuple(range(1, 19)) + (26, 27, 40)]
          + [("fold", ln, L) for ln in (10, 12) for L in (3, 4, 5, 7, 8, 9)]
          + [("fold", 13, L) for L in (7, 8, 9, 10, 14, 15, 17, 40)]
          + [(k, ln, L) for k in CHAIN_KINDS[1:] for ln in (8, 12) for L in (8, 16, 17)]
          + [("mixed16", 12, 16), ("mixed17", 12, 17)])


def _pow_words(orc, base, exponents):
    """base [1][L][N] ** exponents[l] mod q_l, word by word, by the oracle's modular multiply (square and multiply, the exponent's bits per limb)"""
    result = np.ones_like(base)
    e = np.array(exponents, dtype=object)
    for bit in range(max(int(v).bit_length() for v in exponents)):
        take = np.array([(int(v) >> bit) & 1 for v in e], bool)[None, :, None]
        result = np.where(take, orc.dyadic("mul", result, base), result)
        base = orc.dyadic("mul", base, base)
    return result


def inverse_words(orc, x):
    """x [m][L][N], no word zero -> x^-1 mod q_l word by word: one Fermat inversion of the product over m (Montgomery's trick), by the oracle's multiply"""
    m = x.shape[0]
    pref = np.empty_like(x)
    pref[0] = x[0]
    for j in range(1, m):
        pref[j] = orc.dyadic("mul", pref[j - 1][None], x[j][None], threads=0)[0]
    inv = _pow_words(orc, np.ascontiguousarray(pref[m - 1][None]), [q - 2 for q in orc.moduli])
    out = np.empty_like(x)
    for j in range(m - 1, 0, -1):
        out[j] = orc.dyadic("mul", inv, pref[j - 1][None], threads=0)[0]
        inv = orc.dyadic("mul", inv, x[j][None], threads=0)
    out[0] = inv[0]
    return out


def adversarial_key(orc, digits, seed):
    """A key-switching key under which every lazily added product of one item is q - 1, the largest canonical word.

    digits [nd][N]: the digit polynomials of that item (limb j of its last component, words below q_j); orc: the context the key lives on (L limbs).
    x[j][i] = NTT_i(digits[j] mod q_i) is what a key-switching kernel multiplies with key word [j][comp][i]; both components get
    e = (q_i - 1) x^-1 mod q_i, so x e = q_i - 1 in every word and the sum over the digits is the constant -nd mod q_i.  Where x = 0 the word stays random.
    The special case "every target q - 1" of tests/remainder_edges.py key_for_targets.
    -> (key [nd][2][L][N], x [nd][L][N], the number of words with x = 0)"""
    import remainder_edges as re_
    x = re_.digit_transforms(orc, digits)
    rnd = orc.fill(x.shape[0], seed)
    tgt = re_.constant(orc, (x.shape[0], 2), lambda q: q - 1)
    key, zero = re_.key_for_targets(orc, x, tgt, np.stack([rnd, rnd], axis=1))
    return key, x, int(zero.sum())


def reported_classes(p):
    """what dpfhe_ctx_limb_class reports: the catalogue's class per limb where the context has per-limb classes (8 <= log2 N <= 14, L <= 16), the
    context-wide policy otherwise (fold when every limb is 2^60 - d, shoup else)"""
    want = tuple(expected_class(q) for q in p.moduli)
    if all(c == "fold" for c in want):
        return want
    if p.log2_n > 14 or p.n_limbs > 16:
        return ("shoup",) * p.n_limbs
    return want


class Rig:
    def __init__(self, kind, log2n=None):
        """an edge context by name (edge_moduli(kind, log2n)), or ready FheParams (the digit ladders' edge_chain contexts)"""
        from deeppowers_amd.evaluator import Context, Evaluator
        if isinstance(kind, FheParams):
            kind, log2n, self.p = None, kind.log2_n, kind
        else:
            self.p = edge_moduli(kind, log2n)
        self.kind = kind
        self.L, self.n = self.p.n_limbs, self.p.n
        self.orc = Oracle.from_params(self.p)
        self.ctx = Context(self.p, 0)
        self.ev = Evaluator(self.ctx)
        self.qcol = np.array(self.p.moduli, np.uint64)[:, None]
        assert self.ctx.limb_classes == reported_classes(self.p), (kind, log2n, self.ctx.limb_classes, [hex(q) for q in self.p.moduli])
        if kind in CLASSES and log2n <= 14:
            assert set(self.ctx.limb_classes) == {kind}
        if kind == "mixed":
            assert set(self.ctx.limb_classes) == set(CLASSES)
        if kind in MIXED_P:
            assert self.ctx.limb_classes == MIXED_P_CLASSES[kind], (kind, log2n, self.ctx.limb_classes)
        if kind == "fold_scaled6":
            assert self.ctx.limb_classes == ("fold_scaled",) * 6, (kind, log2n, self.ctx.limb_classes)

    def dev(self, a):
        from deeppowers_amd.evaluator import to_device
        return to_device(np.ascontiguousarray(a), self.ctx.device)

    def words(self, orc, lead, seed):
        """orc.fill words shaped [*lead][L][N] with worst_case stripes in item 0 and q - 1 everywhere in item 1"""
        count = int(np.prod(lead))
        x = orc.fill(count, seed).reshape(tuple(lead) + (orc.L, orc.n))
        qcol = np.array(orc.moduli, np.uint64)[:, None]
        worst_case(x, qcol, orc.n)
        if lead[0] > 1:
            x[1] = qcol - np.uint64(1)
        return x

    def close(self):
        self.ctx.close()


def rescale_bsgs_reference(orc, data, t_qp, addends):
    """dpfhe_rescale_bsgs from the oracle's parts (orc: the extended context, data: its first L - 1 limbs): round(t_qp / P), plus component 0 of every
    addend, plus component 1 of addend 0.  t_qp [batch][2][L][N], addends [n_add][batch][2][L-1][N] -> [batch][2][L-1][N]"""
    want = orc.rescale(t_qp)
    for t in range(t_qp.shape[0]):
        for a in range(addends.shape[0]):
            want[t, 0] = data.dyadic("add", want[t, 0][None].copy(), addends[a, t, 0][None].copy())[0]
        if addends.shape[0]:
            want[t, 1] = data.dyadic("add", want[t, 1][None].copy(), addends[0, t, 1][None].copy())[0]
    return want
