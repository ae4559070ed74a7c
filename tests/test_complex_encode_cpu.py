"""CPU: complex slot encoding (include/dpfhe.h dpfhe_encode_complex_host / dpfhe_decode_complex_host, csrc/cencode.h).

The host twin is held to the DEFINITION and to the header's derived bound |c_k - Delta m_k| <= 1/2 + E, E = 8 log2(N) 2^-53 Delta max|z|, at every
coefficient: against the definition's sum in exact arithmetic on 320-bit roots (tests/complex_encode_ref.py) for N = 256 and 1024, and against a
radix-2 transform on the same numbers, anchored on 64 directly evaluated coefficients, for N = 8192 and 65536.  The largest observed error is
printed; the pass condition is the bound.  The residue output is compared with c mod q_l in Python integers, the clamp and NaN rules with their
exact words, decoding with the sum of the two header bounds, and the Galois maps with the slot rotation and conjugation they must give.  The
device kernels are held to the host twin by tests/test_gpu_complex_encode.py."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from deeppowers_amd import _cabi, ckks
from complex_encode_ref import (apply_galois, by_transform, decode_bound, direct, encode_bound, max_abs, residues, slot_vectors, twin)
from test_plain_add_cpu import PARAMS
from test_seeded_cpu import SENTINEL

Q60 = (1152921504606830593,)
SMALL_LIMBS = (7681, 12289)   # primes = 1 mod 512 near 2^13


def _worst(got, want, bound):
    """max_k |got_k - want_k| as a float, after asserting every coefficient within 1/2 + bound"""
    limit = Fraction(1, 2) + Fraction(bound)
    worst = Fraction(0)
    for c, y in zip(got, want):
        err = abs(int(c) - y)
        assert err <= limit, (int(c), float(y), float(err), float(limit))
        worst = max(worst, abs(err))
    return float(worst)


@pytest.mark.parametrize("log2n", (8, 10))
def test_host_twin_meets_the_bound_against_the_definition(log2n):
    for i, (z, scale) in enumerate(slot_vectors(np.random.default_rng(log2n), log2n)):
        got = twin(Q60, log2n, z[None], scale, plain=True)[0]
        bound = encode_bound(z, log2n, scale)
        worst = _worst(got, direct(z, log2n, scale), bound)
        print(f"N={1 << log2n} vector {i}: largest |c_k - Delta m_k| = {worst:.6f}, bound 1/2 + {bound:.3e}")
        if i == 7:
            assert not got.any()                                       # the zero vector
        if i == 8:                                                     # a constant: E < 1/2 forces round(Delta c) +- 1 and zeros
            assert bound < 0.5 and abs(int(got[0]) - round(scale * 0.7215)) <= 1 and not got[1:].any()


@pytest.mark.parametrize("log2n", (13, 16))
def test_host_twin_meets_the_bound_on_large_rings(log2n):
    n = 1 << log2n
    anchor = np.random.default_rng(20261018).choice(n, 64, replace=False)
    for i, (z, scale) in enumerate(slot_vectors(np.random.default_rng(log2n), log2n)):
        got = twin(Q60, log2n, z[None], scale, plain=True)[0]
        want = by_transform(z, log2n, scale)
        tiny = Fraction(1, 1 << 200) * Fraction(scale) * Fraction(max(max_abs(z), 1.0))
        for k, y in zip(anchor, direct(z, log2n, scale, anchor)):
            assert abs(want[k] - y) <= tiny, "the test's transform disagrees with direct evaluation"
        bound = encode_bound(z, log2n, scale)
        worst = _worst(got, want, bound)
        print(f"N={n} vector {i}: largest |c_k - Delta m_k| = {worst:.6f}, bound 1/2 + {bound:.3e}")
        if i == 7:
            assert not got.any()


@pytest.mark.parametrize("name", list(PARAMS) + ["below_t"])
def test_residue_output_is_the_plain_output_mod_each_limb(name):
    if name == "below_t":
        log2n, moduli = 8, SMALL_LIMBS
    else:
        p = PARAMS[name]()
        log2n, moduli = p.log2_n, p.moduli
    vecs = slot_vectors(np.random.default_rng(5), log2n)
    for z, scale in (vecs[0], vecs[1], (vecs[1][0], 2.0 ** 54)):       # |c_k| beyond 2^58: past all but the widest limbs
        plain = twin(moduli, log2n, z[None], scale, plain=True)
        got = twin(moduli, log2n, z[None], scale)
        assert np.array_equal(got, residues(plain, moduli)), name
        assert all(int(got[:, l].max()) < q for l, q in enumerate(moduli))
    assert int(np.abs(plain).max()) > 1 << 58


def test_limb_sizes_cover_13_31_and_60_bits():
    bits = {int(q).bit_length() for name in PARAMS for q in PARAMS[name]().moduli} | {int(q).bit_length() for q in SMALL_LIMBS}
    assert 13 in bits and 31 in bits and 60 in bits


@pytest.mark.parametrize("log2n", (8, 12))
def test_real_flag_gives_the_words_of_zero_imaginary_parts(log2n):
    x = np.random.default_rng(3).uniform(-4, 4, (3, 1 << (log2n - 1)))
    for plain in (True, False):
        assert np.array_equal(twin(SMALL_LIMBS + Q60, log2n, x, 2.0 ** 45, plain=plain), twin(SMALL_LIMBS + Q60, log2n, x + 0j, 2.0 ** 45, plain=plain))
    assert twin(Q60, log2n, x, 2.0 ** 45, plain=True).any()


def test_clamp_and_nan():
    log2n, h = 8, 128
    got = twin(Q60, log2n, np.full((1, h), 8.0), 2.0 ** 60, plain=True)[0]
    assert int(got[0]) == 1 << 62 and not got[1:].any()                 # 2^63 clamps to 2^62 exactly
    got = twin(Q60, log2n, np.full((1, h), -8.0), 2.0 ** 60, plain=True)[0]
    assert int(got[0]) == -(1 << 62) and not got[1:].any()
    z = np.random.default_rng(1).uniform(-1, 1, (1, h)) + 0j
    z[0, 17] = complex(float("nan"), 0.0)
    moduli = SMALL_LIMBS + Q60
    words = twin(moduli, log2n, z, 2.0 ** 40)[0]
    for l, q in enumerate(moduli):
        assert set(int(w) for w in words[l]) <= {0, (1 << 62) % q, (-(1 << 62)) % q}
    assert set(int(w) for w in twin(moduli, log2n, z, 2.0 ** 40, plain=True)[0]) <= {0, 1 << 62, -(1 << 62)}
    # ties go to even: Delta m_0 = 0.5, 1.5, 2.5 exactly
    for c, want in ((0.5, 0), (1.5, 2), (2.5, 2), (-0.5, 0), (-1.5, -2)):
        assert int(twin(Q60, log2n, np.full((1, h), c), 1.0, plain=True)[0, 0]) == want


@pytest.mark.parametrize("log2n", (8, 16))
def test_decode_inverts_encode_within_the_two_bounds(log2n):
    """an error of at most 1/2 + E in each of N coefficients moves a slot (a sum of N coefficients times unit factors) by at most N (1/2 + E) / Delta;
    the decoder adds its own D"""
    n = 1 << log2n
    for z, scale in slot_vectors(np.random.default_rng(log2n + 50), log2n)[:4]:
        coeffs = ckks.encode_host(z[None], scale, log2n)
        back = ckks.decode_host(coeffs, scale, log2n)[0]
        tol = n * (0.5 + encode_bound(z, log2n, scale)) / scale + decode_bound(coeffs, log2n, scale)
        err = float(np.abs(back - z).max())
        print(f"N={n}: largest |decode(encode(z)) - z| = {err:.3e}, bound {tol:.3e}")
        assert err <= tol
        real = ckks.decode_host(coeffs, scale, log2n, real=True)[0]
        assert np.array_equal(real, back.real)


@pytest.mark.parametrize("log2n", (8, 11))
def test_galois_maps_rotate_and_conjugate_the_slots(log2n):
    n = 1 << log2n
    z, scale = slot_vectors(np.random.default_rng(log2n + 9), log2n)[0]
    coeffs = ckks.encode_host(z[None], scale, log2n)[0]
    tol = n * (0.5 + encode_bound(z, log2n, scale)) / scale + decode_bound(coeffs, log2n, scale)
    rot = ckks.decode_host(apply_galois(coeffs, log2n, 3)[None], scale, log2n)[0]
    assert float(np.abs(rot - np.roll(z, -1)).max()) <= tol             # X -> X^3: left by one
    rot5 = ckks.decode_host(apply_galois(coeffs, log2n, pow(3, 5, 2 * n))[None], scale, log2n)[0]
    assert float(np.abs(rot5 - np.roll(z, -5)).max()) <= tol
    conj = ckks.decode_host(apply_galois(coeffs, log2n, 2 * n - 1)[None], scale, log2n)[0]
    assert float(np.abs(conj - np.conj(z)).max()) <= tol
    assert float(np.abs(rot - z).max()) > 0.01


def test_host_entries_reject_bad_arguments():
    lib = _cabi.load()
    log2n, n = 8, 256
    mod = (C.c_uint64 * 2)(12289, 40961)
    even = (C.c_uint64 * 2)(12289, 40962)
    huge = (C.c_uint64 * 2)(12289, 1 << 60)
    slots = ckks.aligned((2, n // 2), np.complex128)
    out = ckks.aligned((2, 2, n), np.uint64)
    out[...] = SENTINEL
    o, s, d = out.ctypes.data, slots.ctypes.data, 2.0 ** 40
    cases = [(None, 2, log2n, o, s, 2, d, 0), (mod, 2, log2n, None, s, 2, d, 0), (mod, 2, log2n, o, None, 2, d, 0), (mod, 2, log2n, o, s, 0, d, 0),
             (mod, 0, log2n, o, s, 2, d, 0), (mod, 2, 7, o, s, 2, d, 0), (mod, 2, 17, o, s, 2, d, 0), (even, 2, log2n, o, s, 2, d, 0),
             (huge, 2, log2n, o, s, 2, d, 0), (mod, 2, log2n, o, s, 2, d, _cabi.ENCODE_NTT), (mod, 2, log2n, o, s, 2, d, 8),
             (mod, 2, log2n, o, s, 2, d, _cabi.ENCODE_PLAIN | _cabi.ENCODE_NTT), (mod, 2, log2n, o, o, 2, d, 0), (mod, 2, log2n, o + 8, s, 1, d, 0),
             (mod, 2, log2n, o, s + 8, 1, d, 0), (mod, 2, log2n, o, s, 2, 0.0, 0), (mod, 2, log2n, o, s, 2, -1.0, 0),
             (mod, 2, log2n, o, s, 2, float("inf"), 0), (mod, 2, log2n, o, s, 2, float("nan"), 0)]
    for args in cases:
        assert lib.dpfhe_encode_complex_host(*args) == 2000, args
        assert (out == SENTINEL).all()
    assert lib.dpfhe_encode_complex_host(mod, 2, log2n, o, s, 2, d, 0) == 0 and not out.any()
    coeffs = np.ones((2, n), dtype=np.int64)
    back = np.full((2, n), 7.5)
    b, c = back.ctypes.data, coeffs.ctypes.data
    for args in ((log2n, None, c, 2, d, 0), (log2n, b, None, 2, d, 0), (log2n, b, c, 0, d, 0), (7, b, c, 2, d, 0), (17, b, c, 2, d, 0), (log2n, b, c, 2, d, 1),
                 (log2n, b, c, 2, 0.0, 0), (log2n, b, c, 2, float("nan"), 0), (log2n, b, b, 2, d, 0)):
        assert lib.dpfhe_decode_complex_host(*args) == 2000, args
        assert (back == 7.5).all()
    assert lib.dpfhe_decode_complex_host(log2n, b, c, 2, d, 0) == 0 and not (back == 7.5).all()


def test_device_entry_points_reject_null_without_a_device():
    lib = _cabi.load()
    enc = C.c_void_p()
    assert lib.dpfhe_cencoder_create(None, None) == 2000
    assert lib.dpfhe_cencoder_create(C.byref(enc), None) == 2000 and not enc.value
    assert lib.dpfhe_encode_complex(None, None, None, 1, 1.0, 0, None) == 2000
    assert lib.dpfhe_cencoder_destroy(None) == 0
