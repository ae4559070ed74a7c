"""Slot encoding over Z_t, restated from its definition (include/dpfhe.h "slot encoding") for tests/test_encode_cpu.py and tests/test_gpu_encode.py:
zeta from its definition, evaluation of a polynomial at the slots' points with plain modular arithmetic, a vectorised radix-2 decode for the large
rings, the slot vectors every case uses, and a ctypes wrapper of the host twin."""
import ctypes as C

import numpy as np

from deeppowers_amd import _cabi
from deeppowers_amd.params import is_prime


def smallest_t(log2n):
    """the smallest prime = 1 mod 2N"""
    t = (2 << log2n) + 1
    while not is_prime(t):
        t += 2 << log2n
    return t


def largest_t(log2n):
    """the largest prime below 2^32 that is 1 mod 2N"""
    t = (1 << 32) - ((1 << 32) - 1) % (2 << log2n)
    while not is_prime(t):
        t -= 2 << log2n
    return t


def zeta_of(log2n, t):
    """g^((t-1)/2N) for the smallest g >= 2 for which it has order exactly 2N"""
    n = 1 << log2n
    for g in range(2, t):
        z = pow(g, (t - 1) // (2 * n), t)
        if pow(z, n, t) == t - 1:
            return z
    raise ValueError("no root")


def slot_exponents(log2n):
    """e[i]: slot i is the value at zeta^e[i] (row 0: 3^i, row 1: -3^i, mod 2N)"""
    n = 1 << log2n
    e, x = np.empty(n, dtype=np.int64), 1
    for i in range(n // 2):
        e[i], e[n // 2 + i] = x, 2 * n - x
        x = x * 3 % (2 * n)
    return e


def root_powers(log2n, t, zeta):
    """zeta^k mod t, k < 2N, as uint64"""
    pw, x = np.empty(2 << log2n, dtype=np.uint64), 1
    for k in range(2 << log2n):
        pw[k] = x
        x = x * zeta % t
    return pw


def evaluate_at(coeffs, points, t):
    """Horner over all `points` at once: products stay below 2^64 because t < 2^32"""
    tt = np.uint64(t)
    acc = np.zeros(points.shape, dtype=np.uint64)
    for a in coeffs[::-1]:
        acc = (acc * points + a) % tt
    return acc


def slots_by_evaluation(coeffs, log2n, t, zeta, positions=None):
    """the slot values of the polynomial `coeffs` ([N] uint64 in [0, t)), all of them or those at `positions`"""
    e = slot_exponents(log2n)
    if positions is not None:
        e = e[positions]
    return evaluate_at(coeffs, root_powers(log2n, t, zeta)[e], t)


def _brv(log2n):
    n = 1 << log2n
    r = np.zeros(n, dtype=np.int64)
    for b in range(log2n):
        r |= ((np.arange(n) >> b) & 1) << (log2n - 1 - b)
    return r


def slots_by_transform(coeffs, log2n, t, zeta):
    """all N slot values by a radix-2 transform (natural order in, value at zeta^(2 brv(k) + 1) out at k), numpy uint64"""
    n, tt = 1 << log2n, np.uint64(t)
    pw, brv = root_powers(log2n, t, zeta), _brv(log2n)
    rp = np.empty(n, dtype=np.uint64)
    rp[brv] = pw[:n]
    a = coeffs.astype(np.uint64).copy()
    m, ln = 1, n // 2
    while m < n:
        v = a.reshape(m, 2, ln)
        w = rp[m:2 * m].reshape(m, 1)
        u, x = v[:, 0, :].copy(), v[:, 1, :] * w % tt
        v[:, 0, :] = (u + x) % tt
        v[:, 1, :] = (u + tt - x) % tt
        m, ln = 2 * m, ln // 2
    return a[brv[(slot_exponents(log2n) - 1) // 2]]


def slot_vectors(rng, n, t):
    """random vectors, all zero, all t - 1, one non-zero slot in each row, a constant vector (last: its polynomial is that constant)"""
    v = rng.integers(0, t, (7, n), dtype=np.uint64).astype(np.uint32)
    v[2] = 0
    v[3] = t - 1
    v[4] = 0
    v[4, int(rng.integers(0, n // 2))] = int(rng.integers(1, t))
    v[5] = 0
    v[5, n // 2 + int(rng.integers(0, n // 2))] = int(rng.integers(1, t))
    v[6] = int(rng.integers(1, t))
    return v


def extreme_slot_vectors(rng, n, t):
    """slot_vectors with the extreme values planted: 0, t - 1, (t - 1) / 2 and (t + 1) / 2 side by side in a random vector, and a vector of each of
    the two half points in every slot"""
    v = slot_vectors(rng, n, t)
    edges = np.array([0, t - 1, (t - 1) // 2, (t + 1) // 2], dtype=np.uint32)
    v[0, :4], v[0, n // 2: n // 2 + 4], v[1, -4:] = edges, edges[::-1], edges
    return np.concatenate([v, np.full((1, n), (t - 1) // 2, np.uint32), np.full((1, n), (t + 1) // 2, np.uint32)])


def t_values(log2n, big):
    ts = [smallest_t(log2n), big]
    if log2n <= 15 and 65537 not in ts:
        ts.insert(1, 65537)
    return ts


def twin(moduli, log2n, t, slots, plain=False, out=None):
    """dpfhe_encode_slots_host: slots uint32 [items][N] -> uint64 [items][N] (plain) or [items][L][N]"""
    slots = np.ascontiguousarray(slots, dtype=np.uint32)
    items, n, L = slots.shape[0], 1 << log2n, len(moduli)
    if out is None:
        out = np.empty((items, n) if plain else (items, L, n), dtype=np.uint64)
    m = (C.c_uint64 * L)(*moduli)
    _cabi.check(_cabi.load().dpfhe_encode_slots_host(m, L, log2n, t, out.ctypes.data, slots.ctypes.data, items, _cabi.ENCODE_PLAIN if plain else 0),
                "dpfhe_encode_slots_host")
    return out


def residues(plain_words, moduli, t):
    """centred(m) mod q_l with Python integers: [items][N] -> [items][L][N]"""
    out = np.empty((plain_words.shape[0], len(moduli), plain_words.shape[1]), dtype=np.uint64)
    for i, row in enumerate(plain_words):
        c = [int(a) - t if int(a) > t // 2 else int(a) for a in row]
        for l, q in enumerate(moduli):
            out[i, l] = np.array([v % q for v in c], dtype=np.uint64)
    return out
