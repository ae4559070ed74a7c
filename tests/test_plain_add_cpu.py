"""CPU: exact plaintext addition (include/dpfhe.h dpfhe_add_plain_scaled_host, csrc/plain_add.h).

The host twin must give c0 +- round(Q b / t) mod q_l computed here with Python integers straight from the definition (not through the
t^-1 identity the library uses), on every limb class, for prime and composite t, for b over all of [0, 2^32), for broadcast, one-to-one and
grouped plaintext items, and with 2 and 3 components.  The device kernel is held to the host twin by tests/test_gpu_plain_add.py."""
import ctypes as C

import numpy as np
import pytest

from deeppowers_amd import _cabi
from deeppowers_amd.params import FheParams, is_prime, min_primitive_2n_root, ntt_primes
from test_seeded_cpu import SENTINEL, _shoup_prime, mixed_params, pinned60, primes31


def big_prime_t():
    """the largest prime below 2^32 that is 1 mod 2^17 (slot-packable at every ring degree up to 2^16)"""
    t = (1 << 32) - ((1 << 32) - 1) % (1 << 17)
    while not is_prime(t):
        t -= 1 << 17
    return t


T_PRIME_BIG = big_prime_t()
T_COMPOSITE = 3 * 5 * 7 * 11 * 13 * 17 * 19   # odd, coprime to every modulus below
T_VALUES = (65537, T_PRIME_BIG, T_COMPOSITE)


def shoup55(log2n=8, count=3):
    """`count` generic-class (Shoup) primes of 55 bits"""
    n = 1 << log2n
    qs, ps = [], []
    q, _ = _shoup_prime(log2n, 55)
    while len(qs) < count:
        if is_prime(q) and (((1 << 55) - q) << 5) >= (1 << 24):
            qs.append(q)
            ps.append(min_primitive_2n_root(n, q))
        q -= 2 * n
    return FheParams(log2n, tuple(qs), tuple(ps))


PARAMS = {"pinned60": pinned60, "primes31": lambda: primes31(8), "shoup55": shoup55, "mixed": lambda: mixed_params(8)}


def twin(p: FheParams, ct: np.ndarray, plain: np.ndarray, t: int, negate=False, out=None) -> np.ndarray:
    """dpfhe_add_plain_scaled_host: ct uint64 [batch][comps][L][N], plain uint64 [P][N] -> a new array (or `out`)"""
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    plain = np.ascontiguousarray(plain, dtype=np.uint64)
    res = ct.copy() if out is None else out
    lib = _cabi.load()
    m = (C.c_uint64 * p.n_limbs)(*p.moduli)
    _cabi.check(lib.dpfhe_add_plain_scaled_host(m, p.n_limbs, p.log2_n, res.ctypes.data, ct.ctypes.data, plain.ctypes.data, ct.shape[0], ct.shape[1],
                                                plain.shape[0], t, 1 if negate else 0), "dpfhe_add_plain_scaled_host")
    return res


def reference(p: FheParams, ct: np.ndarray, plain: np.ndarray, t: int, negate=False) -> np.ndarray:
    """c0 +- round(Q b / t) mod q_l with Python integers; t is odd, so round(x / t) = floor((2 x + t) / 2 t) has no tie"""
    Q = 1
    for q in p.moduli:
        Q *= q
    out = ct.copy()
    group = ct.shape[0] // plain.shape[0]
    for i in range(ct.shape[0]):
        b = plain[i // group].astype(object)
        r = (2 * Q * b + t) // (2 * t)
        for l, q in enumerate(p.moduli):
            c0 = ct[i, 0, l].astype(object)
            out[i, 0, l] = np.array([int(v) % q for v in (c0 - r if negate else c0 + r)], dtype=np.uint64)
    return out


def random_ct(rng, p: FheParams, batch, comps):
    q = np.array(p.moduli, dtype=np.uint64)[None, None, :, None]
    return (rng.integers(0, 1 << 63, (batch, comps, p.n_limbs, p.n), dtype=np.uint64) % q).astype(np.uint64)


def random_plain(rng, items, n, t):
    b = rng.integers(0, 1 << 32, (items, n), dtype=np.uint64)
    b[0, :6] = [0, t - 1, t, t + 1, (1 << 32) - 1, (1 << 32) - 2]   # the edges of [0, 2^32) and of one period of t
    return b


@pytest.mark.parametrize("name", list(PARAMS))
@pytest.mark.parametrize("t", T_VALUES)
def test_twin_matches_definition(name, t):
    p = PARAMS[name]()
    rng = np.random.default_rng(t % 1000 + len(name))
    for batch, comps, items, negate in ((2, 2, 1, False), (3, 3, 3, True), (4, 2, 2, True)):
        ct = random_ct(rng, p, batch, comps)
        plain = random_plain(rng, items, p.n, t)
        got = twin(p, ct, plain, t, negate)
        assert np.array_equal(got, reference(p, ct, plain, t, negate)), (name, t, batch, comps, items, negate)
        assert np.array_equal(got[:, 1:], ct[:, 1:])                          # components >= 1 untouched


@pytest.mark.parametrize("t", (65537, T_PRIME_BIG))
def test_twin_matches_definition_on_the_smallest_primes(t):
    """every limb a smallest prime = 1 mod 2N (class_edges 'smallest'): q far below 2^32 and, for the large t, far below t, so
    round(Q b / t) wraps each limb many times over - what tests/test_gpu_plain_add.py's comparison at the catalogue's extremes rests on"""
    from class_edges import edge_moduli
    for log2n in (8, 12):
        p = edge_moduli("smallest", log2n)
        assert min(p.moduli) < t and max(p.moduli) < 1 << 18 and all(t % q for q in p.moduli)
        rng = np.random.default_rng(t % 1000 + log2n)
        for batch, comps, items, negate in ((2, 2, 1, False), (4, 3, 2, True)):
            ct = random_ct(rng, p, batch, comps)
            ct[-1] = np.array(p.moduli, dtype=np.uint64)[None, :, None] - np.uint64(1)
            plain = random_plain(rng, items, p.n, t)
            got = twin(p, ct, plain, t, negate)
            assert np.array_equal(got, reference(p, ct, plain, t, negate)), (log2n, t, batch, comps, items, negate)
            assert np.array_equal(got[:, 1:], ct[:, 1:])


def test_twin_in_place_out_of_place_and_sentinel():
    p = PARAMS["mixed"]()
    rng = np.random.default_rng(5)
    ct = random_ct(rng, p, 4, 3)
    plain = random_plain(rng, 2, p.n, 65537)
    want = reference(p, ct, plain, 65537)
    out = np.full(ct.shape, SENTINEL, dtype=np.uint64)
    assert np.array_equal(twin(p, ct, plain, 65537, out=out), want)        # out of place: every word written, other components copied
    ip = ct.copy()
    lib = _cabi.load()
    m = (C.c_uint64 * p.n_limbs)(*p.moduli)
    assert lib.dpfhe_add_plain_scaled_host(m, p.n_limbs, p.log2_n, ip.ctypes.data, ip.ctypes.data, plain.ctypes.data, 4, 3, 2, 65537, 0) == 0
    assert np.array_equal(ip, want)


def test_add_then_sub_is_identity_and_more_than_32_limbs():
    """40 limbs: the constants travel in groups of 32 limbs per launch, the twin walks the same groups"""
    p = ntt_primes(8, 40, 31)
    rng = np.random.default_rng(9)
    ct = random_ct(rng, p, 2, 2)
    plain = random_plain(rng, 1, p.n, T_PRIME_BIG)
    added = twin(p, ct, plain, T_PRIME_BIG)
    assert np.array_equal(added, reference(p, ct, plain, T_PRIME_BIG))
    assert np.array_equal(twin(p, added, plain, T_PRIME_BIG, negate=True), ct)


def test_round_is_the_nearest_integer():
    """b = 1, L = 1: round(q / t) itself"""
    p = FheParams.config1()
    q = p.moduli[0]
    ct = np.zeros((1, 2, 1, p.n), dtype=np.uint64)
    plain = np.zeros((1, p.n), dtype=np.uint64)
    plain[0, 0], plain[0, 1] = 1, 2
    for t in T_VALUES:
        got = twin(p, ct, plain, t)
        assert int(got[0, 0, 0, 0]) == (2 * q + t) // (2 * t) and int(got[0, 0, 0, 1]) == (4 * q + t) // (2 * t)
        assert int(twin(p, ct, plain, t, negate=True)[0, 0, 0, 0]) == (q - (2 * q + t) // (2 * t)) % q


def test_rejections_return_invalid_argument():
    p = pinned60()
    lib = _cabi.load()
    m = (C.c_uint64 * p.n_limbs)(*p.moduli)
    ct = np.zeros((4, 2, p.n_limbs, p.n), dtype=np.uint64)
    ct3 = np.zeros((4, 3, p.n_limbs, p.n), dtype=np.uint64)
    plain = np.zeros((2, p.n), dtype=np.uint64)
    o, pl = ct.ctypes.data, plain.ctypes.data

    def call(moduli=m, out=o, inp=o, plain_p=pl, batch=4, comps=2, items=2, t=65537, log2n=p.log2_n, n_limbs=p.n_limbs):
        return lib.dpfhe_add_plain_scaled_host(moduli, n_limbs, log2n, out, inp, plain_p, batch, comps, items, t, 0)

    assert call() == 0
    assert call(comps=3, out=ct3.ctypes.data, inp=ct3.ctypes.data) == 0
    for kw in (dict(moduli=None), dict(out=None), dict(inp=None), dict(plain_p=None),
               dict(comps=1), dict(comps=4), dict(batch=3), dict(items=3), dict(items=0),
               dict(t=65536), dict(t=1), dict(t=2), dict(t=(1 << 32) + 1), dict(t=(1 << 33) + 1),
               dict(log2n=7), dict(n_limbs=0)):
        assert call(**kw) == 2000, kw
    # t sharing a factor with a modulus: t = q_0 of a 31-bit context
    p31 = primes31(8)
    m31 = (C.c_uint64 * p31.n_limbs)(*p31.moduli)
    c31 = np.zeros((1, 2, p31.n_limbs, p31.n), dtype=np.uint64)
    pl31 = np.zeros((1, p31.n), dtype=np.uint64)
    args = (m31, p31.n_limbs, p31.log2_n, c31.ctypes.data, c31.ctypes.data, pl31.ctypes.data, 1, 2, 1)
    assert lib.dpfhe_add_plain_scaled_host(*args, 65537, 0) == 0
    assert lib.dpfhe_add_plain_scaled_host(*args, p31.moduli[1], 0) == 2000
    # plaintext words are < 2^32
    plain[1, 3] = 1 << 32
    assert call() == 2000
    assert not ct.any()                                                      # nothing written by any rejected call
