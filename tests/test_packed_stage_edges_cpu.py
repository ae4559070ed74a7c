"""CPU: the oracle's deferred-division functions at the edges of the limb classes, against their definitions in Python integers.

tests/test_gpu_packed_stage_edges.py holds the stages the packed layers run on (dpfhe_rotate_hoisted_qp, dpfhe_ntt_inv_galois, dpfhe_switch_key_qp,
dpfhe_rescale_bsgs) to oracle.c at the class edges; tests/test_class_edges_cpu.py shows oracle.c exact there for the transforms and ct_mul only.  Here
the four oracle functions those GPU tests rest on - Oracle.rotate_hoisted_qp, Oracle.switch_key_qp, Oracle.rescale with the addends of
dpfhe_rescale_bsgs (class_edges.rescale_bsgs_reference, the composition the GPU tests use), and apply_galois after ntt_inv - are held, at N = 256, to
include/dpfhe.h's text for these entries written out with Python integers: the transform is direct evaluation at the odd powers of psi
(pyoracle.ntt_forward_definition, as one matrix of powers per prime, itself checked against that function), the automorphism is the index map
i -> i g mod 2N with X^N = -1, the lift of a digit is its residue taken as an integer in [0, q_j), and the division by P is floor((X + floor(P / 2)) / P)
on the integer X in [0, Q P) that the residues represent.  Nothing here calls oracle.c for the expected value.

Contexts: the uniform edge context of every class, the all-class mixture, and the five data-class-under-another-P shapes (class_edges.MIXED_P).  Inputs
carry the worst_case stripes in item 0 and q - 1 in every word of item 1, in the ciphertexts and in the keys."""
import numpy as np
import pytest

from class_edges import CLASSES, MIXED_P, Rig, edge_moduli, rescale_bsgs_reference
from oracle import pyoracle as po
from oracle.cbind import Oracle

LOG2N, N = 8, 256
KINDS = CLASSES + ("mixed",) + tuple(MIXED_P)


# ---- the definitions, in Python integers (numpy object arrays hold Python ints: nothing wraps) ------------------------------------------------------------
_matrices = {}


def _powers(q, psi):
    """F[k][j] = psi^((2 brv(k) + 1) j) mod q: row k of F is the evaluation at the k-th odd power of psi, forward-output order; and the inverse
    transform's matrix psi^-((2 brv(k) + 1) j) / N, transposed"""
    if (q, psi) not in _matrices:
        bits = N.bit_length() - 1
        ipsi, ninv = pow(psi, q - 2, q), pow(N, q - 2, q)
        F, G = np.empty((N, N), object), np.empty((N, N), object)
        for k in range(N):
            e = 2 * po.bit_reverse(k, bits) + 1
            w, iw, a, b = pow(psi, e, q), pow(ipsi, e, q), 1, ninv
            for j in range(N):
                F[k, j], G[j, k] = a, b
                a, b = a * w % q, b * iw % q
        probe = [(q - 1 - 3 * j * j) % q for j in range(N)]
        assert [int(v) for v in F.dot(np.array(probe, object)) % q] == po.ntt_forward_definition(probe, q, psi), hex(q)
        assert [int(v) for v in G.dot(F.dot(np.array(probe, object)) % q) % q] == probe, hex(q)
        _matrices[(q, psi)] = (F, G)
    return _matrices[(q, psi)]


def ints(a):
    return np.array(a, np.uint64).astype(object)


def ntt(x, q, psi):
    """x: [..., N] Python integers (any size) -> their forward transform mod q"""
    return np.tensordot(x, _powers(q, psi)[0], axes=([-1], [1])) % q


def intt(x, q, psi):
    return np.tensordot(x, _powers(q, psi)[1], axes=([-1], [1])) % q


def sigma(x, g, q):
    """a(X) -> a(X^g) mod (X^N + 1, q): coefficient i goes to i g mod 2N, negated past N"""
    out = np.empty_like(x)
    for i in range(N):
        idx = i * g % (2 * N)
        out[..., idx % N] = x[..., i] if idx < N else (-x[..., i]) % q
    return out


def key_products(c1, key, p, g=1):
    """[Ld][N] digits, key [Ld][2][L][N] -> [2][L][N]: sum_j NTT_i(sigma_g(lift_i([c1]_{q_j}))) (.) key_{j,comp,i}; the lift takes the residue mod q_j as
    an integer in [0, q_j) and reduces it mod q_i, the automorphism acts after the lift"""
    L = p.n_limbs
    out = np.empty((2, L, N), object)
    for i, (q, psi) in enumerate(zip(p.moduli, p.psi)):
        d = ntt(sigma(c1 % q, g, q), q, psi)                                   # [Ld][N]
        for comp in range(2):
            out[comp, i] = (d * key[:, comp, i]).sum(axis=0) % q
    return out


def rotate_hoisted_qp_definition(ct, elts, keys, p):
    """include/dpfhe.h dpfhe_rotate_hoisted_qp for one item: ct [2][Ld][N] -> [1 + k][2][L][N]"""
    L, Ld, P = p.n_limbs, p.n_limbs - 1, p.moduli[-1]
    out = np.zeros((len(elts) + 1, 2, L, N), object)
    for i in range(Ld):
        q, psi = p.moduli[i], p.psi[i]
        out[0, :, i] = ntt(ct[:, i], q, psi) * P % q
    for r, g in enumerate(elts):
        out[1 + r] = key_products(ct[1], keys[r], p, g)
        for i in range(Ld):
            q, psi = p.moduli[i], p.psi[i]
            out[1 + r, 0, i] = (out[1 + r, 0, i] + P * ntt(sigma(ct[0, i], g, q), q, psi)) % q
    return out


def divide_by_last(x, moduli):
    """[..., L, N] residues -> [..., L - 1, N]: floor((X + floor(P / 2)) / P) mod q_i, X in [0, Q P) the integer the residues represent, P the last limb"""
    Q = 1
    for q in moduli:
        Q *= q
    X = 0
    for i, q in enumerate(moduli):
        X = X + x[..., i, :] * ((Q // q) * pow(Q // q, -1, q))
    X = X % Q
    Y = (X + moduli[-1] // 2) // moduli[-1]
    return np.stack([Y % q for q in moduli[:-1]], axis=-2)


def same(got, want):
    return got.shape == want.shape and bool((got.astype(object) == want).all())


# ---- the tests ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=KINDS)
def setup(request):
    p = edge_moduli(request.param, LOG2N)
    orc = Oracle.from_params(p)
    data = Oracle(LOG2N, p.moduli[:-1], p.psi[:-1])
    return request.param, p, orc, data


def words(orc, lead, seed):
    return Rig.words(None, orc, lead, seed)


def test_switch_key_qp_is_its_definition_at_the_edge_primes(setup):
    kind, p, orc, data = setup
    L, Ld = p.n_limbs, p.n_limbs - 1
    key = words(orc, (Ld, 2), 10)                      # stripes in digit 0's key, q - 1 everywhere in digit 1's
    items = words(data, (3, 2), 11)
    got = orc.switch_key_qp(items, key, threads=0)
    for b in range(3):
        assert same(got[b], key_products(ints(items[b, 1]), ints(key), p)), (kind, b)


def test_rotate_hoisted_qp_is_its_definition_at_the_edge_primes(setup):
    kind, p, orc, data = setup
    L, Ld = p.n_limbs, p.n_limbs - 1
    elts = [3, 2 * N - 1]
    keys = np.stack([words(orc, (Ld, 2), 20 + r) for r in range(len(elts))])
    cts = words(data, (2, 2), 22)
    for t in range(2):
        got = orc.rotate_hoisted_qp(cts[t], elts, keys, threads=0)
        assert same(got, rotate_hoisted_qp_definition(ints(cts[t]), elts, ints(keys), p)), (kind, t)
    got = orc.rotate_hoisted_qp(cts[1], [], keys[:0], threads=0)                 # no rotation: the identity block alone
    assert same(got, rotate_hoisted_qp_definition(ints(cts[1]), [], ints(keys[:0]), p)), kind


def test_rescale_and_the_addends_are_their_definition_at_the_edge_primes(setup):
    kind, p, orc, data = setup
    L, Ld = p.n_limbs, p.n_limbs - 1
    t_qp = words(orc, (3, 2), 30)
    assert same(orc.rescale(t_qp), divide_by_last(ints(t_qp), p.moduli)), kind
    n_add = 6
    rot = words(data, (n_add, 3, 2), 31)                # [n_add][batch][2][Ld][N]: stripes in addend 0, q - 1 everywhere in addend 1
    qcol = np.array(p.moduli[:-1], object)[:, None]
    for count in (0, 1, n_add):
        want = divide_by_last(ints(t_qp), p.moduli)
        if count:
            want[:, 0] = (want[:, 0] + ints(rot[:count, :, 0]).sum(axis=0)) % qcol
            want[:, 1] = (want[:, 1] + ints(rot[0, :, 1])) % qcol
        assert same(rescale_bsgs_reference(orc, data, t_qp, rot[:count]), want), (kind, count)


def test_inverse_transform_then_automorphism_is_its_definition_at_the_edge_primes(setup):
    kind, p, orc, data = setup
    x = words(orc, (3,), 40)
    inv = orc.ntt_inv(x, threads=0)
    for g in (1, 5, 2 * N - 1):
        got = orc.apply_galois(inv, g)
        want = np.stack([sigma(intt(ints(x[:, i]), q, psi), g, q) for i, (q, psi) in enumerate(zip(p.moduli, p.psi))], axis=1)
        assert same(got, want), (kind, g)
