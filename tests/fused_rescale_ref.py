"""The fused rescales (include/dpfhe.h dpfhe_relinearize_rescale_hybrid's last pass, dpfhe_lincomb_rescale) stated with Python integers, the host twins'
ctypes calls, and the inputs the CPU and GPU tests share.  A plain helper like tests/class_edges.py (no conftest, no plugin).

Both references go through the CRT value of a coefficient, not through the limb-by-limb formula the library uses:
  round(X / D) = floor((2 X + D) / (2 D))   (D odd: no tie),   kept modulo limbs that divide Q / D.
"""
import ctypes as C
import functools
import math

import numpy as np

from deeppowers_amd import _cabi
from deeppowers_amd.params import PRIMES_60, FheParams, min_primitive_2n_root

P_EDGES = ("0", "1", "hP-1", "hP", "hP+1", "P-1")       # the work buffer's residue on the special limb
T_EDGES = ("0", "1", "h-1", "h", "h+1", "q_last-1")     # where t_last lands (h = floor(q_last / 2))


@functools.lru_cache(maxsize=None)
def pinned(log2n, limbs):
    """the first `limbs` pinned 60-bit primes (all 1 mod 16384) at ring degree 2^log2n, with their smallest roots"""
    qs = tuple(p[0] for p in PRIMES_60[:limbs])
    return FheParams(log2n, qs, tuple(min_primitive_2n_root(1 << log2n, q) for q in qs))


def crt(res, moduli):
    """res uint64 [L][N] -> object array of X in [0, Q)"""
    Q = math.prod(moduli)
    X = np.zeros(res.shape[-1], dtype=object)
    for l, q in enumerate(moduli):
        Ql = Q // q
        X = X + res[l].astype(object) * (Ql * pow(Ql, -1, q))
    return X % Q


def round_div(X, D):
    return (2 * X + D) // (2 * D)


def residues(X, moduli):
    return np.stack([np.array([int(v) % q for v in X], dtype=np.uint64) for q in moduli])


def divide_by_p(moduli, work_poly):
    """work_poly [L][N] over Q P -> round(X / P) as integers"""
    return round_div(crt(work_poly, moduli), moduli[-1])


def relin_rescale_pass_reference(moduli, work, in3):
    """moduli: the L = Ld + 1 limbs of the extended basis.  work [batch][2][L][N], in3 [batch][3][Ld][N] -> [batch][2][Ld-1][N]:
    t = round(work / P) + c on the Ld data limbs, out = round(t / q_{Ld-1}) on the first Ld - 1"""
    L = len(moduli)
    Ld = L - 1
    data = moduli[:Ld]
    out = np.empty((work.shape[0], 2, Ld - 1, work.shape[-1]), dtype=np.uint64)
    for b in range(work.shape[0]):
        for c in range(2):
            r = divide_by_p(moduli, work[b, c])
            t = np.stack([np.array([(int(v) + int(a)) % q for v, a in zip(r, in3[b, c, l])], dtype=np.uint64) for l, q in enumerate(data)])
            out[b, c] = residues(round_div(crt(t, data), data[-1]), data[:-1])
    return out


def lincomb_rescale_reference(moduli, x, w):
    """x [K][batch][2][L][N], w [K + 1][L] -> [batch][2][L-1][N]"""
    K, batch, L, n = x.shape[0], x.shape[1], x.shape[3], x.shape[4]
    out = np.empty((batch, 2, L - 1, n), dtype=np.uint64)
    for t in range(batch):
        for c in range(2):
            s = []
            for l, q in enumerate(moduli):
                acc = np.zeros(n, dtype=object)
                for k in range(K):
                    acc = acc + x[k, t, c, l].astype(object) * int(w[k, l])
                if c == 0:
                    acc[0] += int(w[K, l])
                s.append(np.array([int(v) % q for v in acc], dtype=np.uint64))
            out[t, c] = residues(round_div(crt(np.stack(s), moduli), moduli[-1]), moduli[:-1])
    return out


# ---- host twins --------------------------------------------------------------------------------------------------------------------------------------
def relin_rescale_pass_twin(p, work, in3):
    work = np.ascontiguousarray(work, dtype=np.uint64)
    in3 = np.ascontiguousarray(in3, dtype=np.uint64)
    out = np.full((work.shape[0], 2, p.n_limbs - 2, p.n), 0xDEADBEEFCAFEF00D, dtype=np.uint64)
    m = (C.c_uint64 * p.n_limbs)(*p.moduli)
    _cabi.check(_cabi.load().dpfhe_relinearize_rescale_pass_host(m, p.n_limbs, p.log2_n, out.ctypes.data, work.ctypes.data, in3.ctypes.data, work.shape[0]),
                "dpfhe_relinearize_rescale_pass_host")
    return out


def lincomb_rescale_twin(p, x, w):
    x = np.ascontiguousarray(x, dtype=np.uint64)
    w = np.ascontiguousarray(w, dtype=np.uint64)
    out = np.full((x.shape[1], 2, p.n_limbs - 1, p.n), 0xDEADBEEFCAFEF00D, dtype=np.uint64)
    m = (C.c_uint64 * p.n_limbs)(*p.moduli)
    _cabi.check(_cabi.load().dpfhe_lincomb_rescale_host(m, p.n_limbs, p.log2_n, out.ctypes.data, x.ctypes.data, w.ctypes.data, x.shape[0], x.shape[1]),
                "dpfhe_lincomb_rescale_host")
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------------
def random_words(rng, moduli, lead, n):
    q = np.array(moduli, dtype=np.uint64)[:, None]
    return (rng.integers(0, 1 << 63, tuple(lead) + (len(moduli), n), dtype=np.uint64) % q).astype(np.uint64)


def edge_value(name, P, qlast):
    hP, h = P // 2, qlast // 2
    return {"0": 0, "1": 1, "hP-1": hP - 1, "hP": hP, "hP+1": hP + 1, "P-1": P - 1, "h-1": h - 1, "h": h, "h+1": h + 1, "q_last-1": qlast - 1}[name]


def pass_a_inputs(p, batch, seed, planted=True):
    """(work [batch][2][L][N], in3 [batch][3][Ld][N], plan): random canonical words; with `planted`, coefficients 0 .. 35 of BOTH components of item 0 carry
    the 6 x 6 edges: the P-limb residue of `work` is P_EDGES[j // 6] and the free input word c_last is solved so that t_last = T_EDGES[j % 6].
    plan: [(coefficient, P-limb word, t_last target)]"""
    rng = np.random.default_rng(seed)
    L, Ld, n = p.n_limbs, p.n_limbs - 1, p.n
    P, ql = p.moduli[-1], p.moduli[Ld - 1]
    work = random_words(rng, p.moduli, (batch, 2), n)
    in3 = random_words(rng, p.moduli[:Ld], (batch, 3), n)
    plan = []
    if planted:
        for j in range(36):
            wp, tgt = edge_value(P_EDGES[j // 6], P, ql), edge_value(T_EDGES[j % 6], P, ql)
            work[0, :, L - 1, j] = wp
            plan.append((j, wp, tgt))
        for c in range(2):
            r = divide_by_p(p.moduli, work[0, c])
            for j, _, tgt in plan:
                in3[0, c, Ld - 1, j] = (tgt - int(r[j])) % ql
    return work, in3, plan


def t_last_of(p, work, in3, item, comp):
    """the intermediate word on the last data limb (what dpfhe_relinearize_hybrid writes there), from the integers"""
    Ld = p.n_limbs - 1
    ql = p.moduli[Ld - 1]
    r = divide_by_p(p.moduli, work[item, comp])
    return np.array([(int(v) + int(a)) % ql for v, a in zip(r, in3[item, comp, Ld - 1])], dtype=np.uint64)


def lincomb_inputs(p, K, batch, seed, full=False):
    """(x [K][batch][2][L][N], w [K + 1][L]); `full`: every operand word and every weight q - 1 (the fullest lazy sum)"""
    rng = np.random.default_rng(seed)
    q = np.array(p.moduli, dtype=np.uint64)
    if full:
        x = np.broadcast_to((q - np.uint64(1))[:, None], (K, batch, 2, p.n_limbs, p.n)).copy()
        w = np.broadcast_to(q - np.uint64(1), (K + 1, p.n_limbs)).copy()
        return x, w
    x = random_words(rng, p.moduli, (K, batch, 2), p.n)
    w = (rng.integers(0, 1 << 63, (K + 1, p.n_limbs), dtype=np.uint64) % q).astype(np.uint64)
    x[0, 0, :, :, :4] = (q - np.uint64(1))[None, :, None]      # extreme residues next to the constant's coefficient
    x[-1, 0, :, :, 4:8] = 0
    return x, w
