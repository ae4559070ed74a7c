"""Complex slot encoding, restated from its definition (include/dpfhe.h "complex slot encoding") for tests/test_complex_encode_cpu.py and
tests/test_gpu_complex_encode.py: Delta m_k = Delta (2/N) Re( sum_i z_i xi^(-3^i k) ) in exact arithmetic on 320-bit roots of unity.

The roots xi^e come from mpmath at 320 bits and are kept as integers scaled by 2^F (F = 288); a double is an exact rational, so a slot times a root
and every sum of such products is formed in Python integers without any rounding.  The only error of a reference value is that of the roots, below
2^-280 of Delta max|z| N: fifty orders of magnitude under the bound the tests hold the encoder to.  Also here: a radix-2 transform on the same integers
for the large rings (anchored on directly evaluated coefficients by its callers), the slot vectors every case uses, the header's two bounds, and
wrappers of the host entries."""
import ctypes as C
import functools
import math
from fractions import Fraction

import mpmath
import numpy as np

from deeppowers_amd import _cabi, ckks

F = 288
ONE = 1 << F


@functools.lru_cache(maxsize=None)
def roots(log2n):
    """(cos, sin) of pi e / N for e < 2N as object arrays of integers scaled by 2^F; a quarter turn from mpmath, the rest by symmetry"""
    n = 1 << log2n
    with mpmath.workprec(320):
        q = [(int(mpmath.floor(mpmath.ldexp(mpmath.cospi(mpmath.mpf(e) / n), F) + 0.5)), int(mpmath.floor(mpmath.ldexp(mpmath.sinpi(mpmath.mpf(e) / n), F) + 0.5)))
             for e in range(n // 2 + 1)]
    cos, sin = np.empty(2 * n, dtype=object), np.empty(2 * n, dtype=object)
    for e in range(2 * n):
        k, r = divmod(e, n // 2)                         # a quarter turn multiplies by i: (c, s) -> (-s, c)
        c, s = q[r]
        cos[e], sin[e] = ((c, s), (-s, c), (-c, -s), (s, -c))[k]
    return cos, sin


def slot_exponents(log2n):
    """3^i mod 2N, i < N/2"""
    n = 1 << log2n
    e, x = np.empty(n // 2, dtype=np.int64), 1
    for i in range(n // 2):
        e[i] = x
        x = x * 3 % (2 * n)
    return e


def _exact(v):
    """doubles -> (integers, shift): v = integers / 2^shift exactly"""
    fr = [Fraction(float(x)) for x in v]
    shift = max(f.denominator.bit_length() - 1 for f in fr)
    return np.array([int(f * (1 << shift)) for f in fr], dtype=object), shift


def direct(z, log2n, scale, ks=None):
    """Delta m_k for the coefficients `ks` (default: all) of one slot vector z (complex [N/2]) as Fractions, by the definition's sum"""
    n = 1 << log2n
    cos, sin = roots(log2n)
    e = slot_exponents(log2n)
    zr, sr = _exact(np.real(z))
    zi, si = _exact(np.imag(z))
    out = []
    for k in (range(n) if ks is None else ks):
        idx = (e * int(k)) % (2 * n)                     # Re(z xi^(-e k)) = re cos + im sin
        s = Fraction(int((zr * cos[idx]).sum()), 1 << (sr + F)) + Fraction(int((zi * sin[idx]).sum()), 1 << (si + F))
        out.append(Fraction(float(scale)) * 2 * s / n)
    return out


def by_transform(z, log2n, scale):
    """Delta m_k for all k as Fractions: c_j = m_j + i m_(j+n) = xi^(-j) (1/n) sum_r v_r exp(-2 pi i r j / n), v_r the value at xi^(4r+1), by a radix-2
    decimation-in-frequency transform on the scaled integers (each product floors at 2^-F)"""
    n, h = 1 << log2n, 1 << (log2n - 1)
    cos, sin = roots(log2n)
    e = slot_exponents(log2n)
    zr, sr = _exact(np.real(z))
    zi, si = _exact(np.imag(z))
    shift = max(sr, si)
    zr, zi = zr * (1 << (shift - sr + F)), zi * (1 << (shift - si + F))       # slots scaled by 2^(shift + F)
    vr, vi = np.empty(h, dtype=object), np.empty(h, dtype=object)
    for i in range(h):
        ex = int(e[i])
        if i % 2 == 0:
            vr[(ex - 1) // 4], vi[(ex - 1) // 4] = zr[i], zi[i]
        else:
            vr[(2 * n - ex - 1) // 4], vi[(2 * n - ex - 1) // 4] = zr[i], -zi[i]
    ln = h
    while ln >= 2:
        a, b = vr.reshape(-1, 2, ln // 2), vi.reshape(-1, 2, ln // 2)
        step = 4 * (h // ln)                             # exp(-2 pi i j / ln) = xi^(-4 j h / ln)
        wr, wi = cos[(np.arange(ln // 2) * step) % (2 * n)], -sin[(np.arange(ln // 2) * step) % (2 * n)]
        ur, ui, xr, xi_ = a[:, 0, :].copy(), b[:, 0, :].copy(), a[:, 1, :].copy(), b[:, 1, :].copy()
        a[:, 0, :], b[:, 0, :] = ur + xr, ui + xi_
        dr, di = ur - xr, ui - xi_
        a[:, 1, :], b[:, 1, :] = (dr * wr - di * wi) >> F, (dr * wi + di * wr) >> F
        ln //= 2
    bits = log2n - 1
    rev = np.zeros(h, dtype=np.int64)
    for b_ in range(bits):
        rev |= ((np.arange(h) >> b_) & 1) << (bits - 1 - b_)
    cr, ci = vr[rev], vi[rev]                            # position brv(j) holds the sum for j
    j = np.arange(h)
    tr, ti = cos[j], -sin[j]                             # xi^(-j)
    mr, mi = (cr * tr - ci * ti) >> F, (cr * ti + ci * tr) >> F
    den = h << (shift + F)
    d = Fraction(float(scale))
    return [d * Fraction(int(x), den) for x in mr] + [d * Fraction(int(x), den) for x in mi]


def max_abs(z):
    return max(math.hypot(float(x.real), float(x.imag)) for x in np.asarray(z, dtype=np.complex128))


def encode_bound(z, log2n, scale):
    """the header's E = 8 log2(N) 2^-53 Delta max|z|"""
    return 8 * log2n * 2.0 ** -53 * float(scale) * max_abs(z)


def decode_bound(coeffs, log2n, scale):
    """the header's D = 8 log2(N) 2^-53 N max|c_k| / scale"""
    return 8 * log2n * 2.0 ** -53 * (1 << log2n) * float(np.abs(np.asarray(coeffs, dtype=np.float64)).max()) / float(scale)


def slot_vectors(rng, log2n):
    """(z, scale) pairs: random |re|, |im| <= 1 at 2^40; |z| up to 2^10 at 2^50; purely real; purely imaginary; unit impulses in slots 0, 1 and
    n - 1; the zero vector; a constant real vector"""
    h = 1 << (log2n - 1)
    def rnd():
        return rng.uniform(-1, 1, h) + 1j * rng.uniform(-1, 1, h)
    def impulse(i):
        v = np.zeros(h, dtype=np.complex128)
        v[i] = 1.0
        return v
    big = rnd() * (1024 / math.sqrt(2))
    return [(rnd(), 2.0 ** 40), (big, 2.0 ** 50), (rnd().real + 0j, 2.0 ** 40), (1j * rnd().imag, 2.0 ** 40), (impulse(0), 2.0 ** 40),
            (impulse(1), 2.0 ** 40), (impulse(h - 1), 2.0 ** 40), (np.zeros(h, dtype=np.complex128), 2.0 ** 40),
            (np.full(h, 0.7215, dtype=np.complex128), 2.0 ** 40)]


def special_vectors(rng, log2n):
    """complex [5][N/2] for the device comparison: random, a constant 8.0 (clamps at Delta = 2^60), one NaN, one Inf, a denormal-sized slot"""
    h = 1 << (log2n - 1)
    v = rng.uniform(-1, 1, (5, h)) + 1j * rng.uniform(-1, 1, (5, h))
    v[1] = 8.0
    v[2, h // 3] = complex(float("nan"), 0.25)
    v[3, h // 5] = complex(0.5, float("inf"))
    v[4, 7] = complex(1e-310, -1e-310)
    return v


def twin(moduli, log2n, slots, scale, plain=False):
    """dpfhe_encode_complex_host: complex or float64 [items][N/2] -> int64 [items][N] (plain) or uint64 [items][L][N]"""
    return ckks.encode_host(slots, scale, log2n, None if plain else moduli)


def residues(plain_words, moduli):
    """c mod q_l with Python integers: int64 [items][N] -> uint64 [items][L][N]"""
    out = np.empty((plain_words.shape[0], len(moduli), plain_words.shape[1]), dtype=np.uint64)
    for i, row in enumerate(plain_words):
        c = [int(a) for a in row]
        for l, q in enumerate(moduli):
            out[i, l] = np.array([v % q for v in c], dtype=np.uint64)
    return out


def apply_galois(coeffs, log2n, g):
    """the coefficients of m(X^g) mod X^N + 1 (g odd)"""
    n = 1 << log2n
    out = np.zeros_like(coeffs)
    for k in range(n):
        d = k * g % (2 * n)
        if d < n:
            out[d] = coeffs[k]
        else:
            out[d - n] = -coeffs[k]
    return out


def host_args(moduli, out, slots):
    return (C.c_uint64 * len(moduli))(*moduli), out.ctypes.data, slots.ctypes.data
