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

from deeppowers_amd.params import is_prime, min_primitive_2n_root

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
