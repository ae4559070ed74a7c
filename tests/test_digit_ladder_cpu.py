"""CPU: what tests/test_gpu_digit_ladder.py rests on.

  - class_edges.edge_chain gives, at every rung of class_edges.LADDER, the asked number of distinct primes = 1 mod 2N of the claimed class, the first four
    the catalogue's own, and the C rule of tables.h (through the emulator) takes every one of them for that class;
  - oracle.c's relinearize, keyswitch_hybrid (2 and 3 components), switch_key_qp and rotate_hoisted_qp equal their definitions in Python integers
    (tests/test_packed_stage_edges_cpu.py: direct evaluation of the transform, the lift as the residue in [0, q_j), the division by P on the integer the
    residues represent) at N = 256 with 8, 14 and 17 limbs - the oracle reduces after every product, so nothing in it depends on the digit count, and
    this shows it;
  - the adversarial keys of class_edges.adversarial_key do what they claim, on the oracle alone, at 14, 17 and 40 limbs: x e = q - 1 in Python integers
    for every word with x != 0, at most 1 word in 1000 with x = 0, and the closed form - relinearize returns (c0, c1) with coefficient 0 shifted by -L,
    switch_key_qp the constant -Ld in every word, keyswitch_hybrid (c0, c1) unchanged (the sum is Q P - Ld, which divided by P rounds to Q = 0)."""
import numpy as np
import pytest

from class_edges import (CHAIN_KINDS, LADDER, Rig, adversarial_key, catalogue_moduli, chain_classes, chain_moduli, edge_chain, expected_class,
                         reported_classes)
from deeppowers_amd.params import is_prime
from oracle.cbind import Oracle
from test_class_edges_cpu import ARITH
from test_emulated_kernels import GEOS, emu, run  # noqa: F401  (emu: the module fixture that builds tools/libemu.so)
from test_packed_stage_edges_cpu import N, divide_by_last, intt, ints, key_products, rotate_hoisted_qp_definition, same

LOG2N = 8
assert N == 1 << LOG2N


# ---- the chains -------------------------------------------------------------------------------------------------------------------------------------------------
def test_edge_chain_yields_every_rung_of_the_ladder():
    assert len(set(LADDER)) == len(LADDER)
    for kind, log2n, L in LADDER:
        p = edge_chain(kind, log2n, L)
        n = 1 << log2n
        assert p.n_limbs == L and len(set(p.moduli)) == L, (kind, log2n, L)
        assert tuple(expected_class(q) for q in p.moduli) == chain_classes(kind, L), (kind, log2n, L)
        for q, psi in zip(p.moduli, p.psi):
            assert is_prime(q) and (q - 1) % (2 * n) == 0 and pow(psi, n, q) == q - 1, (kind, log2n, hex(q))
        if kind in CHAIN_KINDS:
            assert reported_classes(p) == ((kind,) * L if kind == "fold" or L <= 16 else ("shoup",) * L)
        else:
            assert expected_class(p.moduli[15]) == "fold"                     # the top nibble of the active-limb map names a fast class
            assert reported_classes(p) == (chain_classes(kind, L) if L == 16 else ("shoup",) * 17)
            assert set(chain_classes(kind, L)) == set(CHAIN_KINDS)


@pytest.mark.parametrize("log2n", (8, 10, 12, 13))
def test_chains_start_at_the_catalogue_and_run_inward(log2n):
    """the walk from each bound inward: at least 64 fold primes (46 at N = 8192) and 18 of every other class; the first four are the catalogue's entry"""
    cat = catalogue_moduli(log2n)
    for kind, entry in (("fold", "fold_edge"), ("shoup", "shoup60"), ("f64", "f64_edge"), ("f64_wide", "f64_wide_edge")):
        qs = chain_moduli(kind, log2n, (46 if log2n == 13 else 64) if kind == "fold" else 18)
        assert qs[:4] == cat[entry][:4], (kind, log2n)
        assert list(qs) == sorted(qs, reverse=kind != "fold"), (kind, log2n)
    qs = chain_moduli("fold_scaled", log2n, 18)
    assert set(qs) <= {q for name, e in cat.items() if name.startswith("fscaled_edge_") for q in e}
    assert all(expected_class(q) == "fold_scaled" for q in qs)


@pytest.mark.parametrize("log2n", sorted({ln for _, ln, _ in LADDER}))
def test_the_c_rule_takes_every_chain_prime_for_its_class(emu, log2n):
    """tables.h through the emulator: the policy of the claimed class accepts every prime of the longest chain of each kind at this ring degree (fold
    primes are refused by no policy but their own rule's complement: the generic policy takes everything)"""
    le = next(le for ln, le in GEOS if ln == log2n)
    z = np.zeros(1 << log2n, np.uint64)
    longest = {}
    for kind, ln, L in LADDER:
        if ln == log2n:
            longest[kind] = max(longest.get(kind, 0), L)
    for kind, L in longest.items():
        p = edge_chain(kind, log2n, L)
        for q, psi, cls in zip(p.moduli, p.psi, chain_classes(kind, L)):
            assert run(emu, ARITH[cls], log2n, le, 0, q, psi, z)[0] == 0, (kind, hex(q), cls)
            for other in ("fold", "fold_scaled"):                         # the two rules that are a band, not a ceiling: exactly their own primes
                assert (run(emu, ARITH[other], log2n, le, 0, q, psi, z)[0] == 0) == (cls == other), (kind, hex(q), other)


# ---- the oracle's key switches against their definitions, by limb count -----------------------------------------------------------------------------------------
def words(orc, lead, seed):
    return Rig.words(None, orc, lead, seed)


def key_switch_terms(digits, key, p):
    """[2][L][N], coefficient domain: INTT_i(sum_j NTT_i(lift_i(digit j)) (.) key[j][comp][i])"""
    kp = key_products(digits, key, p)
    return np.stack([np.stack([intt(kp[c, i], q, psi) for i, (q, psi) in enumerate(zip(p.moduli, p.psi))]) for c in range(2)])


def relinearize_definition(ct3, evk, p):
    """include/dpfhe.h dpfhe_relinearize for one item: (c0, c1) + sum_j [c2]_{q_j} (.) evk_j; ct3 [3][L][N], evk [L][2][L][N] -> [2][L][N]"""
    qcol = np.array(p.moduli, object)[:, None]
    return (key_switch_terms(ct3[2], evk, p) + ct3[:2]) % qcol


def keyswitch_hybrid_definition(ct, key, p):
    """dpfhe_relinearize_hybrid / dpfhe_switch_key_hybrid for one item: round(t / P) + c0 (and + c1 with three components); ct [comps][Ld][N]"""
    qcol = np.array(p.moduli[:-1], object)[:, None]
    out = divide_by_last(key_switch_terms(ct[-1], key, p), p.moduli)
    out[0] = (out[0] + ct[0]) % qcol
    if ct.shape[0] == 3:
        out[1] = (out[1] + ct[1]) % qcol
    return out


@pytest.fixture(scope="module", params=(8, 14, 17))
def chain(request):
    p = edge_chain("fold", LOG2N, request.param)
    return p, Oracle.from_params(p), Oracle(LOG2N, p.moduli[:-1], p.psi[:-1])


def test_relinearize_is_its_definition_at_every_digit_count(chain):
    p, orc, _ = chain
    L = p.n_limbs
    evk = words(orc, (L, 2), 50)                        # stripes in digit 0's key, q - 1 everywhere in digit 1's
    ct3 = words(orc, (2, 3), 51)
    got = orc.relinearize(ct3, evk, threads=0)
    for b in range(2):
        assert same(got[b], relinearize_definition(ints(ct3[b]), ints(evk), p)), (L, b)


def test_keyswitch_hybrid_is_its_definition_at_every_digit_count(chain):
    p, orc, data = chain
    Ld = p.n_limbs - 1
    key = words(orc, (Ld, 2), 52)
    for comps in (2, 3):
        ct = words(data, (2, comps), 53 + comps)
        got = orc.keyswitch_hybrid(ct, key, comps, threads=0)
        b = comps - 2                                   # the stripes with two components, q - 1 in every word with three
        assert same(got[b], keyswitch_hybrid_definition(ints(ct[b]), ints(key), p)), (Ld, comps)


def test_switch_key_qp_is_its_definition_at_every_digit_count(chain):
    p, orc, data = chain
    Ld = p.n_limbs - 1
    key = words(orc, (Ld, 2), 56)
    items = words(data, (2, 2), 57)
    got = orc.switch_key_qp(items, key, threads=0)
    for b in range(2):
        assert same(got[b], key_products(ints(items[b, 1]), ints(key), p)), (Ld, b)


def test_rotate_hoisted_qp_is_its_definition_at_every_digit_count(chain):
    p, orc, data = chain
    Ld = p.n_limbs - 1
    elts = [2 * N - 1]
    keys = words(orc, (Ld, 2), 58)[None]
    cts = words(data, (2, 2), 59)
    for t in range(2):
        got = orc.rotate_hoisted_qp(cts[t], elts, keys, threads=0)
        assert same(got, rotate_hoisted_qp_definition(ints(cts[t]), elts, ints(keys), p)), (Ld, t)


# ---- the adversarial keys, on the oracle alone -------------------------------------------------------------------------------------------------------------------
def check_adversarial(orc, digits, key, x, n_zero):
    """the construction's own claims, in Python integers: both components equal, x e = q - 1 wherever x != 0, at most 1 word in 1000 with x = 0"""
    q = np.array(orc.moduli, object)[None, :, None]
    assert np.array_equal(key[:, 0], key[:, 1]) and key.shape == (digits.shape[0], 2, orc.L, orc.n)
    for j in range(digits.shape[0]):                   # x is the transform of the lifted digit (the oracle's transform is held to its definition elsewhere)
        lifted = np.stack([digits[j] % np.uint64(qi) for qi in orc.moduli])
        assert np.array_equal(x[j], orc.ntt_fwd(lifted[None], threads=0)[0])
    prod = ints(x) * ints(key[:, 0]) % q
    assert bool(((prod == q - 1) | (ints(x) == 0)).all())
    assert n_zero == int((x == 0).sum()) and n_zero * 1000 <= x.size, n_zero


def constant_words(moduli, value, n):
    """[len(moduli)][n]: value mod q_i in every word"""
    return np.array([[value % q] * n for q in moduli], np.uint64)


@pytest.mark.parametrize("L", (14, 17, 40))
def test_adversarial_keys_and_their_closed_form_on_the_oracle(L):
    p = edge_chain("fold", LOG2N, L)
    orc, data = Oracle.from_params(p), Oracle(LOG2N, p.moduli[:-1], p.psi[:-1])
    Ld = L - 1
    qcol = np.array(p.moduli, np.uint64)[:, None]
    # RNS-digit keys: L digits
    ct3 = words(orc, (2, 3), 60)
    evk, x, n_zero = adversarial_key(orc, ct3[0, 2], 61)
    check_adversarial(orc, ct3[0, 2], evk, x, n_zero)
    got = orc.relinearize(ct3, evk, threads=0)
    if n_zero == 0:
        want = ct3[0, :2].copy()
        want[:, :, 0] = (want[:, :, 0] + (qcol[:, 0] - np.uint64(L))) % qcol[:, 0]
        assert np.array_equal(got[0], want)
    # a special prime: Ld digits on L limbs
    items = words(data, (2, 2), 62)
    key, x, n_zero = adversarial_key(orc, items[0, 1], 63)
    check_adversarial(orc, items[0, 1], key, x, n_zero)
    got = orc.switch_key_qp(items, key, threads=0)
    if n_zero == 0:
        assert np.array_equal(got[0], np.stack([constant_words(p.moduli, -Ld, N)] * 2))
        for comps in (2, 3):
            ct = words(data, (2, comps), 64 + comps)
            ct[0, comps - 1] = items[0, 1]
            got = orc.keyswitch_hybrid(ct, key, comps, threads=0)
            want = ct[0, :2].copy()
            if comps == 2:
                want[1] = 0
            assert np.array_equal(got[0], want), comps
