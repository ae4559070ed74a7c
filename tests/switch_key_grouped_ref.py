"""dpfhe_switch_key_grouped (include/dpfhe.h) in Python integers: the centred digit of every group, its residue on every limb, the exact round(X / P)
and the addend.  Only the negacyclic products go through the oracle's transform (oracle.cbind.Oracle over all L limbs), which no device code shares.
The rounding is dpfhe_scale_round's with multiplier 1 as the header states it: (X - r) / P with r the CENTRED remainder of X modulo P; P is odd, so
no remainder sits on a tie.  A plain helper (no conftest, no plugin), like tests/footprint.py."""
import numpy as np


def groups(Ld, alpha):
    return [range(d * alpha, min((d + 1) * alpha, Ld)) for d in range(-(-Ld // alpha))]


def product(qs):
    out = 1
    for q in qs:
        out *= int(q)
    return out


def crt(rows, qs):
    """rows[i][k] = X_k mod qs[i] -> the integers X_k in [0, product(qs))"""
    Q = product(qs)
    basis = [(Q // q) * pow(Q // q, -1, q) for q in map(int, qs)]
    return [sum(int(r) * b for r, b in zip(col, basis)) % Q for col in zip(*rows)]


def centred(x, Q):
    return x - Q if x > Q // 2 else x          # Q odd: (-Q / 2, Q / 2]


def digits(c, moduli, Ld, alpha):
    """c [Ld][N] -> per group the centred integers x_d, x_d = c mod D_d"""
    out = []
    for g in groups(Ld, alpha):
        qs = [moduli[i] for i in g]
        out.append([centred(x, product(qs)) for x in crt([c[i] for i in g], qs)])
    return out


def lift(c, moduli, Ld, alpha):
    """-> [groups][L][N]: every digit modulo every limb"""
    return np.array([[[x % int(q) for x in xd] for q in moduli] for xd in digits(c, moduli, Ld, alpha)], np.uint64)


def key_products(orc, lifted, key):
    """[groups][L][N] coefficient domain, key [groups][2][L][N] NTT domain -> INTT(sum_d NTT(digit_d) (.) key_d) [2][L][N]"""
    x, qcol = orc.ntt_fwd(lifted), np.array(orc.moduli, np.uint64)[:, None]
    acc = np.zeros((2,) + x.shape[1:], np.uint64)
    for d in range(x.shape[0]):
        for comp in range(2):
            acc[comp] = (acc[comp] + orc.dyadic("mul", x[d], np.ascontiguousarray(key[d, comp]))) % qcol      # (below 2^61: no wrap)
    return orc.ntt_inv(acc)


def divide_and_add(work, ct, moduli, Ld, at):
    """work [2][L][N] over Q P, ct [comps][Ld][N] -> {(comp, k): the Ld output words} at the coefficients `at`: (c0, c1 or 0) + round(X / P)"""
    P, comps, out = product(moduli[Ld:]), ct.shape[0], {}
    for comp in range(2):
        X = crt([[work[comp, i, k] for k in at] for i in range(len(moduli))], moduli)
        for k, x in zip(at, X):
            y = (x - centred(x % P, P)) // P
            add = [int(ct[comp, j, k]) if comp == 0 or comps == 3 else 0 for j in range(Ld)]
            out[comp, k] = [(y + a) % int(moduli[j]) for j, a in enumerate(add)]
    return out

