"""The fused relinearise + linear combination + rescale (include/dpfhe.h dpfhe_relinearize_lincomb_rescale_hybrid's last pass; csrc/fused_rescale.h (c)) stated
with Python integers, the host twin's ctypes call, and the inputs the CPU and GPU tests share.  A plain helper like tests/fused_rescale_ref.py, whose CRT value,
round_div and edge names it uses: every division goes through the integer of its coefficient, never through the limb-by-limb formula of the library.

  t   = round(work / P) + c                          on the Ld data limbs   (the words dpfhe_relinearize_hybrid writes)
  s_l = w[0][l] t_l + sum_k w[1+k][l] z_k,l + [component 0, coefficient 0] w[K+1][l]   mod q_l
  out = round(S / q_{Ld-1}) on the first Ld - 1 limbs, S the CRT value of (s_l)

A term is [batch][2][limbs_k][N] with limbs_k >= Ld; limbs past the first Ld are never read, and the inputs here fill them with a word that is no residue."""
import ctypes as C
import math

import numpy as np

import fused_rescale_ref as fr
from deeppowers_amd import _cabi
from deeppowers_amd.params import FheParams

NOT_A_RESIDUE = np.uint64(0xDEADBEEFCAFEF00D)      # >= 2^60: above every admissible modulus
K_CASES = (0, 1, 4, 5, 15)                         # none; below, on and past the four-in-flight loop; the most


def data_params(p):
    return FheParams(p.log2_n, tuple(p.moduli[:-1]), tuple(p.psi[:-1]))


def term_limbs(K, Ld):
    """Ld and Ld + 2 mixed in one call"""
    return [Ld + 2 * (k % 2) for k in range(K)]


# ---- the integers --------------------------------------------------------------------------------------------------------------------------------------------
def relinearized(moduli, work, in3):
    """work [batch][2][L][N] over Q P, in3 [batch][3][Ld][N] -> t [batch][2][Ld][N]"""
    data = moduli[:-1]
    t = np.empty((work.shape[0], 2, len(data), work.shape[-1]), dtype=np.uint64)
    for b in range(work.shape[0]):
        for c in range(2):
            r = fr.divide_by_p(moduli, work[b, c])
            for l, q in enumerate(data):
                t[b, c, l] = np.array([(int(v) + int(a)) % q for v, a in zip(r, in3[b, c, l])], dtype=np.uint64)
    return t


def sums(data, t, terms, w, b, c):
    """the words s_l [Ld][N] of item b, component c"""
    K, n = len(terms), t.shape[-1]
    s = []
    for l, q in enumerate(data):
        acc = t[b, c, l].astype(object) * int(w[0, l])
        for k in range(K):
            acc = acc + terms[k][b, c, l].astype(object) * int(w[1 + k, l])
        if c == 0:
            acc[0] += int(w[K + 1, l])
        s.append(np.array([int(v) % q for v in acc], dtype=np.uint64))
    return np.stack(s)


def combine_reference(data, t, terms, w):
    """data: the Ld data moduli; t [batch][2][Ld][N] -> [batch][2][Ld-1][N]"""
    out = np.empty((t.shape[0], 2, len(data) - 1, t.shape[-1]), dtype=np.uint64)
    for b in range(t.shape[0]):
        for c in range(2):
            out[b, c] = fr.residues(fr.round_div(fr.crt(sums(data, t, terms, w, b, c), data), data[-1]), data[:-1])
    return out


def pass_reference(moduli, work, in3, terms, w):
    return combine_reference(moduli[:-1], relinearized(moduli, work, in3), terms, w)


# ---- the host twin -------------------------------------------------------------------------------------------------------------------------------------------
def host_args(terms):
    K = len(terms)
    ptrs = (C.c_void_p * max(K, 1))(*[t.ctypes.data for t in terms])
    limbs = (C.c_uint32 * max(K, 1))(*[t.shape[2] for t in terms])
    return ptrs, limbs


def pass_twin_rc(p, out, work, in3, terms, w, batch=None):
    ptrs, limbs = host_args(terms)
    m = (C.c_uint64 * p.n_limbs)(*p.moduli)
    return _cabi.load().dpfhe_relinearize_lincomb_rescale_pass_host(m, p.n_limbs, p.log2_n, out.ctypes.data, work.ctypes.data, in3.ctypes.data, ptrs, limbs,
                                                                    len(terms), w.ctypes.data, work.shape[0] if batch is None else batch)


def pass_twin(p, work, in3, terms, w):
    work, in3, w = (np.ascontiguousarray(a, dtype=np.uint64) for a in (work, in3, w))
    terms = [np.ascontiguousarray(t, dtype=np.uint64) for t in terms]
    out = np.full((work.shape[0], 2, p.n_limbs - 2, p.n), NOT_A_RESIDUE, dtype=np.uint64)
    _cabi.check(pass_twin_rc(p, out, work, in3, terms, w), "dpfhe_relinearize_lincomb_rescale_pass_host")
    return out


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------------------------
def invertible_weights(rng, moduli, rows):
    """[rows][len(moduli)] random canonical residues, each a unit of its limb (so that a planted word can be solved through it)"""
    w = np.empty((rows, len(moduli)), dtype=np.uint64)
    for l, q in enumerate(moduli):
        for r in range(rows):
            v = int(rng.integers(1, 1 << 62)) % q
            while math.gcd(v, q) != 1:
                v = (v + 1) % q
            w[r, l] = v
    return w


def terms_and_weights(p, K, batch, seed, full=False):
    """(terms, w): K terms at term_limbs(K, Ld) limbs, the limbs past Ld filled with NOT_A_RESIDUE; w [K + 2][Ld].  `full`: every read word and every
    weight q - 1"""
    rng = np.random.default_rng(seed)
    data = list(p.moduli[:-1])
    Ld, n = len(data), p.n
    q = np.array(data, dtype=np.uint64)
    terms = []
    for limbs in term_limbs(K, Ld):
        z = np.full((batch, 2, limbs, n), NOT_A_RESIDUE, dtype=np.uint64)
        z[:, :, :Ld] = (q - np.uint64(1))[:, None] if full else fr.random_words(rng, data, (batch, 2), n)
        terms.append(z)
    w = np.broadcast_to(q - np.uint64(1), (K + 2, Ld)).copy() if full else invertible_weights(rng, data, K + 2)
    return terms, w


def plan_of(p):
    """[(coefficient, P-limb word of the sums, target of s_last)]: the 6 x 6 edges of P and of the last data prime"""
    P, ql = p.moduli[-1], p.moduli[-2]
    return [(j, fr.edge_value(fr.P_EDGES[j // 6], P, ql), fr.edge_value(fr.T_EDGES[j % 6], P, ql)) for j in range(36)]


def aim_s_last(p, t_last, in3_last, terms, w, plan, item=0):
    """solve one free word per planted coefficient and component of `item` so that s_last lands on the plan's target: with terms, term 0's word on the last
    data limb; without, c_last of the input (t_last then moves with it).  t_last: [2][N], the intermediate words of the item on the last data limb
    (before the solve); in3_last: in3[item, :, Ld - 1] (a view: written when K = 0).  Returns t_last as it is afterwards."""
    Ld = p.n_limbs - 1
    ql, K, lo = p.moduli[Ld - 1], len(terms), Ld - 1
    t_last = t_last.copy()
    for c in range(2):
        for j, _, tgt in plan:
            rest = sum(int(w[1 + k, lo]) * int(terms[k][item, c, lo, j]) for k in range(1, K)) + (int(w[K + 1, lo]) if c == 0 and j == 0 else 0)
            if K:
                need = (tgt - rest - int(w[0, lo]) * int(t_last[c, j])) % ql
                terms[0][item, c, lo, j] = need * pow(int(w[1, lo]), -1, ql) % ql
            else:
                want_t = (tgt - rest) * pow(int(w[0, lo]), -1, ql) % ql
                in3_last[c, j] = (int(in3_last[c, j]) + want_t - int(t_last[c, j])) % ql
                t_last[c, j] = want_t
    return t_last


def pass_inputs(p, K, batch, seed, planted=True, full=False):
    """(work, in3, terms, w, plan).  `planted`: coefficients 0 .. 35 of both components of item 0 carry the plan (plan_of): the P-limb word of `work` is the
    P edge and s_last the edge of the last data prime"""
    work, in3, _ = fr.pass_a_inputs(p, batch, seed, planted=False)
    terms, w = terms_and_weights(p, K, batch, seed + 1, full=full)
    plan = []
    if full:      # t = q - 1 everywhere: round(0 / P) + (q - 1)
        work[:] = 0
        in3[:] = (np.array(p.moduli[:-1], dtype=np.uint64) - np.uint64(1))[:, None]
    elif planted:
        plan = plan_of(p)
        for j, wp, _ in plan:
            work[0, :, -1, j] = wp
        t_last = relinearized(p.moduli, work[:1], in3[:1])[0, :, -1]
        aim_s_last(p, t_last, in3[0, :, p.n_limbs - 2], terms, w, plan)
    return work, in3, terms, w, plan
