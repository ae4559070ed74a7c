"""CPU: plaintext addition on residues (include/dpfhe.h dpfhe_add_plain_host, csrc/plain_add.h).

The host twin must give c0 +- p mod q_l computed here with Python integers, on every limb class, with the sums the one conditional subtraction
decides on - q - 1, q, q + 1, 0 and 2 q - 2 - planted in every item, for broadcast, grouped and one-to-one plaintext items, with 2 and 3
components, in place and out of place.  The device kernel is held to the host twin by tests/test_gpu_add_plain.py."""
import ctypes as C

import numpy as np
import pytest

from deeppowers_amd import _cabi
from deeppowers_amd.params import FheParams, ntt_primes
from test_plain_add_cpu import PARAMS, random_ct
from test_seeded_cpu import SENTINEL

# (x, p) per limb of modulus q, as functions of q: x + p lands on q - 1, q, q + 1, 0, 2 q - 2 and q again; x + (q - p), the word the subtraction
# forms, on q - 1, q, q + 1, 2 q - 2 (it is never below 1), and on 1 and 2 q - 1, its two extremes
EDGES = ((lambda q: q - 1, lambda q: 0), (lambda q: q - 1, lambda q: 1), (lambda q: q - 1, lambda q: 2), (lambda q: 0, lambda q: 0),
         (lambda q: q - 1, lambda q: q - 1), (lambda q: 1, lambda q: q - 1),
         (lambda q: 0, lambda q: 1), (lambda q: 1, lambda q: 0), (lambda q: q - 2, lambda q: 0), (lambda q: 0, lambda q: q - 1))


def twin(p: FheParams, ct: np.ndarray, plain: np.ndarray, negate=False, out=None) -> np.ndarray:
    """dpfhe_add_plain_host: ct uint64 [batch][comps][L][N], plain uint64 [P][L][N] -> a new array (or `out`)"""
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    plain = np.ascontiguousarray(plain, dtype=np.uint64)
    res = ct.copy() if out is None else out
    lib = _cabi.load()
    m = (C.c_uint64 * p.n_limbs)(*p.moduli)
    _cabi.check(lib.dpfhe_add_plain_host(m, p.n_limbs, p.log2_n, res.ctypes.data, ct.ctypes.data, plain.ctypes.data, ct.shape[0], ct.shape[1],
                                         plain.shape[0], 1 if negate else 0), "dpfhe_add_plain_host")
    return res


def reference(p: FheParams, ct: np.ndarray, plain: np.ndarray, negate=False) -> np.ndarray:
    """(c0 +- p) mod q_l with Python integers"""
    out = ct.copy()
    group = ct.shape[0] // plain.shape[0]
    for i in range(ct.shape[0]):
        for l, q in enumerate(p.moduli):
            c0, b = ct[i, 0, l].astype(object), plain[i // group, l].astype(object)
            out[i, 0, l] = np.array([int(v) % q for v in (c0 - b if negate else c0 + b)], dtype=np.uint64)
    return out


def operands(rng, p: FheParams, batch, comps, items):
    """random canonical words with the EDGES pairs at coefficients 0 .. 9 of every limb of every ciphertext item and plaintext item"""
    ct = random_ct(rng, p, batch, comps)
    plain = random_ct(rng, p, items, 1)[:, 0]
    for l, q in enumerate(p.moduli):
        for k, (fx, fp) in enumerate(EDGES):
            ct[:, 0, l, k] = fx(q)
            plain[:, l, k] = fp(q)
    return ct, np.ascontiguousarray(plain)


SHAPES = ((2, 2, 1, False), (3, 3, 3, True), (4, 2, 2, True), (6, 3, 2, False))   # batch, comps, plaintext items, negate


@pytest.mark.parametrize("name", list(PARAMS))
def test_twin_matches_python_integers(name):
    p = PARAMS[name]()
    rng = np.random.default_rng(len(name))
    for batch, comps, items, negate in SHAPES:
        ct, plain = operands(rng, p, batch, comps, items)
        got = twin(p, ct, plain, negate)
        want = reference(p, ct, plain, negate)
        assert np.array_equal(got, want), (name, batch, comps, items, negate)
        assert np.array_equal(got[:, 1:], ct[:, 1:])                          # components >= 1 untouched
        assert all(int(got[:, 0, l].max()) < q for l, q in enumerate(p.moduli))   # canonical out


def test_the_edge_sums_are_what_they_claim():
    """the planted pairs reach q - 1, q, q + 1, 0 and 2 q - 2 before the subtraction, and the twin's words at them are the reduced sums"""
    p = PARAMS["mixed"]()
    ct, plain = operands(np.random.default_rng(1), p, 1, 2, 1)
    added, subbed = twin(p, ct, plain), twin(p, ct, plain, negate=True)
    for l, q in enumerate(p.moduli):
        x, b = [int(v) for v in ct[0, 0, l, :10]], [int(v) for v in plain[0, l, :10]]
        assert {q - 1, q, q + 1, 0, 2 * q - 2} <= {a + c for a, c in zip(x, b)}
        assert {q - 1, q, q + 1, 2 * q - 2, 1, 2 * q - 1} <= {a + q - c for a, c in zip(x, b)}
        assert [int(v) for v in added[0, 0, l, :10]] == [(a + c) % q for a, c in zip(x, b)]
        assert [int(v) for v in subbed[0, 0, l, :10]] == [(a - c) % q for a, c in zip(x, b)]


def test_smallest_primes_and_forty_limbs():
    """every q far below 2^32, and more limbs than any kernel-argument table holds: one launch walks them all, the twin likewise"""
    from class_edges import edge_moduli
    for p in (edge_moduli("smallest", 8), ntt_primes(8, 40, 31)):
        rng = np.random.default_rng(p.n_limbs)
        ct, plain = operands(rng, p, 4, 2, 2)
        added = twin(p, ct, plain)
        assert np.array_equal(added, reference(p, ct, plain))
        assert np.array_equal(twin(p, added, plain, negate=True), ct)         # add then subtract: the input's words


def test_in_place_out_of_place_and_sentinel():
    p = PARAMS["mixed"]()
    ct, plain = operands(np.random.default_rng(5), p, 4, 3, 2)
    want = reference(p, ct, plain)
    out = np.full(ct.shape, SENTINEL, dtype=np.uint64)
    assert np.array_equal(twin(p, ct, plain, out=out), want)                  # out of place: every word written, other components copied
    ip = ct.copy()
    lib = _cabi.load()
    m = (C.c_uint64 * p.n_limbs)(*p.moduli)
    assert lib.dpfhe_add_plain_host(m, p.n_limbs, p.log2_n, ip.ctypes.data, ip.ctypes.data, plain.ctypes.data, 4, 3, 2, 0) == 0
    assert np.array_equal(ip, want)


def test_broadcast_rule():
    """ciphertext item i takes plaintext item i / (batch / plain_items)"""
    p = ntt_primes(8, 2, 60)
    rng = np.random.default_rng(7)
    ct, plain = operands(rng, p, 6, 2, 3)
    got = twin(p, ct, plain)
    for i in range(6):
        assert np.array_equal(got[i:i + 1], twin(p, ct[i:i + 1], plain[i // 2:i // 2 + 1])), i


def test_rejections_return_invalid_argument():
    p = FheParams.n4096_l4()
    lib = _cabi.load()
    m = (C.c_uint64 * p.n_limbs)(*p.moduli)
    even = (C.c_uint64 * p.n_limbs)(*([p.moduli[0] + 1] + list(p.moduli[1:])))
    buf = np.zeros((9, 2, p.n_limbs, p.n), dtype=np.uint64)                   # ct = items 0 .. 3, a second ciphertext buffer = items 4 .. 7
    ct3 = np.zeros((4, 3, p.n_limbs, p.n), dtype=np.uint64)
    plain = np.zeros((2, p.n_limbs, p.n), dtype=np.uint64)
    o, pl = buf.ctypes.data, plain.ctypes.data
    item = 2 * p.n_limbs * p.n * 8

    def call(moduli=m, out=o, inp=o, plain_p=pl, batch=4, comps=2, items=2, log2n=p.log2_n, n_limbs=p.n_limbs):
        return lib.dpfhe_add_plain_host(moduli, n_limbs, log2n, out, inp, plain_p, batch, comps, items, 0)

    assert call() == 0
    assert call(out=o + 4 * item) == 0                                        # out of place, apart
    assert call(comps=3, out=ct3.ctypes.data, inp=ct3.ctypes.data) == 0
    for kw in (dict(moduli=None), dict(out=None), dict(inp=None), dict(plain_p=None), dict(comps=1), dict(comps=4), dict(batch=0), dict(batch=0, items=0),
               dict(batch=3), dict(items=3), dict(items=0), dict(log2n=7), dict(log2n=17), dict(n_limbs=0), dict(moduli=even),
               dict(out=o + item), dict(out=o + 8),                            # out and in overlap without being equal
               dict(out=pl, inp=pl),                                           # out overlaps the plaintext
               dict(batch=1 << 31, items=1)):                                  # a grid too large for one launch (refused before any word is read)
        assert call(**kw) == 2000, kw
    assert not buf.any()                                                       # nothing written by any rejected call
    plain[1, 2, 5] = p.moduli[2]                                               # a plaintext word that is not canonical
    assert call() == 2000
    plain[1, 2, 5] -= 1
    assert call() == 0
    assert int(buf[2, 0, 2, 5]) == p.moduli[2] - 1 and int(buf[:, 0].astype(object).sum()) == 2 * (p.moduli[2] - 1)


def test_device_entry_refuses_null_pointers_without_a_device():
    lib = _cabi.load()
    buf = np.zeros(64, dtype=np.uint64)
    a = buf.ctypes.data
    assert lib.dpfhe_add_plain(None, a, a, a, 1, 2, 1, 0, None) == 2000
    assert lib.dpfhe_add_plain(None, None, None, None, 1, 2, 1, 0, None) == 2000
    assert b"dpfhe_add_plain" in lib.dpfhe_last_error()
