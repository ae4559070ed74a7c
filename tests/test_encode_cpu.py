"""CPU: slot encoding over Z_t (include/dpfhe.h dpfhe_encode_slots_host, csrc/encode.h).

The host twin is held to the DEFINITION, not to another inverse transform: the polynomial it returns is evaluated at zeta^(3^i) and zeta^(-3^i)
for all N slots with plain modular arithmetic and must give the slot values back (N values fix a polynomial of degree < N, so this pins every
word).  For N >= 8192 all slots are decoded by a radix-2 transform written in tests/encode_ref.py, itself anchored on 256 positions by the
direct evaluation.  The residue output is compared with centred(m) mod q_l in Python integers, on limbs above and below t.  The device kernels
are held to the host twin by tests/test_gpu_encode.py; the host twin walks the same per-group functions (csrc/encode.h enc_group) the kernels run."""
import ctypes as C

import numpy as np
import pytest

from deeppowers_amd import _cabi
from encode_ref import (extreme_slot_vectors, largest_t, residues, slot_vectors, slots_by_evaluation, slots_by_transform, t_values, twin,
                        zeta_of)
from test_plain_add_cpu import PARAMS, big_prime_t
from test_seeded_cpu import SENTINEL

T_BIG = big_prime_t()
Q60 = (1152921504606830593,)   # any odd modulus serves the plain output


def test_t_sets_are_the_expected_ones():
    assert t_values(8, T_BIG) == [7681, 65537, T_BIG] and t_values(12, T_BIG) == [40961, 65537, T_BIG]
    assert t_values(13, T_BIG) == [65537, T_BIG] and t_values(15, T_BIG) == [65537, T_BIG] and t_values(16, T_BIG) == [786433, T_BIG]


@pytest.mark.parametrize("log2n", range(8, 13))
def test_host_twin_satisfies_the_definition_at_every_slot(log2n):
    n = 1 << log2n
    for t in t_values(log2n, T_BIG):
        zeta = zeta_of(log2n, t)
        slots = slot_vectors(np.random.default_rng(log2n * 1000 + t % 997), n, t)
        m = twin(Q60, log2n, t, slots, plain=True)
        assert int(m.max()) < t
        for i in range(slots.shape[0]):
            assert np.array_equal(slots_by_evaluation(m[i], log2n, t, zeta), slots[i].astype(np.uint64)), (log2n, t, i)
        assert int(m[6, 0]) == int(slots[6, 0]) and not m[6, 1:].any()      # a constant vector is the constant polynomial
        assert not m[2].any()


@pytest.mark.parametrize("log2n", range(13, 17))
def test_host_twin_large_rings_every_slot_by_transform(log2n):
    n = 1 << log2n
    for t in t_values(log2n, T_BIG):
        zeta = zeta_of(log2n, t)
        rng = np.random.default_rng(log2n * 1000 + t % 997)
        slots = slot_vectors(rng, n, t)
        m = twin(Q60, log2n, t, slots, plain=True)
        assert int(m.max()) < t
        pos = np.random.default_rng(20261016).choice(n, 256, replace=False)
        for i in range(slots.shape[0]):
            decoded = slots_by_transform(m[i], log2n, t, zeta)
            assert np.array_equal(decoded[pos], slots_by_evaluation(m[i], log2n, t, zeta, pos)), "the test's transform disagrees with direct evaluation"
            assert np.array_equal(decoded, slots[i].astype(np.uint64)), (log2n, t, i)       # no slot left unchecked
        assert int(m[6, 0]) == int(slots[6, 0]) and not m[6, 1:].any()


SMALL_LIMBS = (7681, 12289)   # primes = 1 mod 512 near 2^13: every limb below t


@pytest.mark.parametrize("name", list(PARAMS) + ["below_t"])
@pytest.mark.parametrize("items", (1, 3))
def test_residue_output_is_the_centred_polynomial_mod_each_limb(name, items):
    if name == "below_t":
        log2n, moduli, ts = 8, SMALL_LIMBS, (T_BIG,)
    else:
        p = PARAMS[name]()
        log2n, moduli, ts = p.log2_n, p.moduli, (65537, T_BIG)
    for t in ts:
        rng = np.random.default_rng(items * 31 + t % 1013)
        slots = slot_vectors(rng, 1 << log2n, t)[[0, 3, 4][:items]]
        plain = twin(moduli, log2n, t, slots, plain=True)
        got = twin(moduli, log2n, t, slots)
        assert np.array_equal(got, residues(plain, moduli, t)), (name, t)
        assert all(int(got[:, l].max()) < q for l, q in enumerate(moduli))


def test_residue_output_on_the_smallest_primes_with_the_largest_t():
    """every limb a smallest prime = 1 mod 2N (class_edges 'smallest': q far below t), t the largest prime below 2^32 that is 1 mod 2N, slots at 0,
    t - 1, (t - 1) / 2 and (t + 1) / 2: the polynomial decodes to the slots, its residues are centred(m) mod q_l - what tests/test_gpu_encode.py's
    comparison at the catalogue's extremes rests on"""
    from class_edges import edge_moduli
    for log2n in (8, 12):
        p = edge_moduli("smallest", log2n)
        t = largest_t(log2n)
        assert max(p.moduli) < 1 << 18 and t > (1 << 32) - (1 << 20)
        slots = extreme_slot_vectors(np.random.default_rng(log2n), p.n, t)
        plain = twin(p.moduli, log2n, t, slots, plain=True)
        zeta = zeta_of(log2n, t)
        for i in range(slots.shape[0]):
            assert np.array_equal(slots_by_evaluation(plain[i], log2n, t, zeta), slots[i].astype(np.uint64)), (log2n, i)
        got = twin(p.moduli, log2n, t, slots)
        assert np.array_equal(got, residues(plain, p.moduli, t)), log2n
        assert all(int(got[:, l].max()) < q for l, q in enumerate(p.moduli))


def test_host_twin_rejects_bad_arguments():
    lib = _cabi.load()
    log2n, t, n = 8, 7681, 256
    mod = (C.c_uint64 * 2)(12289, 40961)
    slots = np.zeros((2, n), dtype=np.uint32)
    out = np.full((2, 2, n), SENTINEL, dtype=np.uint64)
    o, s = out.ctypes.data, slots.ctypes.data
    bad_slots = slots.copy()
    bad_slots[1, 77] = t
    even = (C.c_uint64 * 2)(12289, 40962)
    huge = (C.c_uint64 * 2)(12289, 1 << 60)
    cases = [(None, 2, log2n, t, o, s, 2, 0), (mod, 2, log2n, t, None, s, 2, 0), (mod, 2, log2n, t, o, None, 2, 0), (mod, 2, log2n, t, o, s, 0, 0),
             (mod, 0, log2n, t, o, s, 2, 0), (mod, 2, 7, t, o, s, 2, 0), (mod, 2, 17, t, o, s, 2, 0), (even, 2, log2n, t, o, s, 2, 0), (huge, 2, log2n, t, o, s, 2, 0),
             (mod, 2, log2n, 7680, o, s, 2, 0), (mod, 2, log2n, 513 * 5, o, s, 2, 0), (mod, 2, log2n, 12289 * 512 * 11 + 1, o, s, 2, 0), (mod, 2, log2n, 65537 + 512, o, s, 2, 0),
             (mod, 2, log2n, (1 << 32) + 15 * 512 + 1, o, s, 2, 0), (mod, 2, 9, 7681, o, s, 2, 0), (mod, 2, log2n, t, o, bad_slots.ctypes.data, 2, 0),
             (mod, 2, log2n, t, o, s, 2, _cabi.ENCODE_NTT), (mod, 2, log2n, t, o, s, 2, 4), (mod, 2, log2n, t, o, s, 2, 3), (mod, 2, log2n, t, o, o, 2, 0)]
    for args in cases:
        assert lib.dpfhe_encode_slots_host(*args) == 2000, args
        assert (out == SENTINEL).all()
    assert lib.dpfhe_encode_slots_host(mod, 2, log2n, t, o, s, 2, 0) == 0 and not out.any()


def test_device_entry_points_reject_null_without_a_device():
    lib = _cabi.load()
    enc = C.c_void_p()
    assert lib.dpfhe_encoder_create(None, None, 65537) == 2000
    assert lib.dpfhe_encoder_create(C.byref(enc), None, 65537) == 2000 and not enc.value
    assert lib.dpfhe_encode_slots(None, None, None, 1, 0, None) == 2000
    assert lib.dpfhe_encoder_destroy(None) == 0
    assert lib.dpfhe_encoder_root(None) == 0
