"""The big-integer model of ApproxAttentionScores on TRANSPARENT inputs (include/deeppowers/fhe.hpp: c1 = 0, c0 the residues of a known integer polynomial), shared
by tests/test_attention_scores_model_cpu.py and tests/test_gpu_attention_scores_words.py.

With c1 = 0 the tensor product of a pair is (a0 b0, 0, 0): every key-switch digit is zero, the key products vanish whatever the keys hold, and the division by P
is exact.  The words of pair (i, j) are therefore
    m_ij = round(q_i k_j / q_last)  in Z[X] / (X^N + 1),   then  acc <- acc + sigma_g(acc)  for g = 3^(stride 2^e), e < log2(block),
taken modulo the primes of the next level.  Packings: `one` (one head of DIMS_ONE values in a block of 16, stride 1) and `heads` (3 heads of 8 values interleaved
at stride 4, the small stand-in for GPT-2's 12 x 64 at stride 16; the fourth residue holds zeros)."""
import math

import numpy as np

import approx_layer_model as alm
import approx_poly_model as apm
from deeppowers_amd import ckks
from deeppowers_amd.params import ntt_primes

SCALE = 2.0 ** 55
POST = 0.125
PACKINGS = {"one": dict(block=16, stride=1, heads=1, dims=12), "heads": dict(block=8, stride=4, heads=3, dims=8)}
U = 2.0 ** -53


def ring(log2n):
    """(data parameters: 3 limbs, special prime, its psi) - the first four primes of the chain at this ring degree"""
    p = ntt_primes(log2n, 4)
    from deeppowers_amd.params import FheParams
    return FheParams(log2n, tuple(p.moduli[:3]), tuple(p.psi[:3])), p.moduli[3], p.psi[3]


def elements(block, stride, n):
    g, out = pow(3, stride, 2 * n), []
    while len(out) < block.bit_length() - 1:
        out.append(g)
        g = g * g % (2 * n)
    return out


def pairs_of(T, causal):
    return [(i, j) for i in range(T) for j in range(T) if not causal or j <= i]


class Case:
    def __init__(self, log2n, T, packing, causal, seed=None):
        self.log2n, self.T, self.packing, self.causal = log2n, T, packing, causal
        self.n, self.pk = 1 << log2n, PACKINGS[packing]
        self.data, self.special, self.special_psi = ring(log2n)
        rng = np.random.default_rng(seed if seed is not None else 4000 + 100 * log2n + 10 * T + len(packing) + int(causal))
        pk = self.pk
        self.q = rng.uniform(-1, 1, (T, pk["heads"], pk["dims"]))
        self.k = rng.uniform(-1, 1, (T, pk["heads"], pk["dims"]))
        self.pairs = pairs_of(T, causal)

    def slots(self, v):
        """[T][heads][dims] -> [T][N/2] slot vectors in the packing"""
        pk, row = self.pk, self.n // 2
        s = np.arange(row)
        head, dim = s % pk["stride"], (s // pk["stride"]) % pk["block"]
        ok = (head < pk["heads"]) & (dim < pk["dims"])
        out = np.zeros((self.T, row))
        out[:, ok] = v[:, head[ok], dim[ok]]
        return out

    def polynomials(self, v):
        """the integer polynomials round(SCALE m) the client would encrypt: [T] object arrays"""
        coeffs = ckks.encode_host(self.slots(v).astype(np.complex128), SCALE, self.log2n)
        return [np.array([int(c) for c in row], dtype=object) for row in coeffs]

    def scores(self):
        """float64: [pairs][heads], POST <q_i, k_j> per head, dims ascending"""
        out = np.zeros((len(self.pairs), self.pk["heads"]))
        for a, (i, j) in enumerate(self.pairs):
            for h in range(self.pk["heads"]):
                s = 0.0
                for d in range(self.pk["dims"]):
                    s += self.q[i, h, d] * self.k[j, h, d]
                out[a, h] = POST * s
        return out

    def output_scale(self):
        return (SCALE * SCALE) / float(self.data.moduli[-1]) / POST


def model(case, qp, kp):
    """-> (products [pairs] object arrays: round(q_i k_j / q_last); scores [pairs] object arrays after the ladder), integers in Z[X] / (X^N + 1)"""
    q_last = case.data.moduli[-1]
    elts = elements(case.pk["block"], case.pk["stride"], case.n)
    prods, out = [], []
    for i, j in case.pairs:
        m = np.array([apm.round_div(int(c), q_last) for c in apm.negacyclic(qp[i], kp[j])], dtype=object)
        prods.append(m)
        acc = m
        for g in elts:
            acc = acc + alm.automorphism(acc, g)
        out.append(acc)
    return prods, out


def words(polys, moduli):
    """[items] object arrays -> [items][2][L][N] uint64: c0 the residues, c1 = 0"""
    out = np.zeros((len(polys), 2, len(moduli), len(polys[0])), dtype=np.uint64)
    for t, a in enumerate(polys):
        out[t, 0] = alm.residues(a, moduli)
    return out


def keyswitch_term(Ld, N, qmax, P):
    return 21.0 * Ld * N * (qmax / P)


def error_bound(case, A, B, Bq, Bk):
    """the header's bound in Python floats, term by term (ApproxProductSum at one term, then SlotSum's with Bin = S e1, times post_factor)"""
    N, log2n = float(case.n), case.log2n
    H, u8 = (N + 1) / 2, 8 * log2n * U
    mod, P = case.data.moduli, case.special
    q, S = float(mod[-1]), (SCALE * SCALE) / float(mod[-1])
    Kr = keyswitch_term(len(mod), N, float(max(mod)), float(P))
    Da, Db, Y = N * Bq, N * Bk, A * B
    E = ((SCALE * A * Db + SCALE * B * Da + Da * Db) + N * (Kr + H)) / q + N * H + 4 * U * S * Y
    pre1 = E / S
    e1 = pre1 + u8 * N * (Y + pre1) + 2 * U * Y
    blk = float(case.pk["block"])
    K2 = keyswitch_term(len(mod) - 1, N, float(max(mod[:-1])), float(P))
    pre = N * (blk * (S * e1) + (blk - 1) * (K2 + H)) / S
    return POST * (pre + u8 * N * (blk * Y + pre) + 4 * U * blk * Y)


def decode(case, poly):
    """the client's decode of one integer polynomial at output_scale(): [N/2] complex"""
    return ckks.decode_host(np.array([[int(c) for c in poly]], dtype=np.int64), case.output_scale(), case.log2n)[0]
