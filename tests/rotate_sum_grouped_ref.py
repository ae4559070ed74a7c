"""dpfhe_rotate_sum_hoisted_grouped (include/dpfhe.h) in Python integers, from the parts of tests/switch_key_grouped_ref.py and the oracle's automorphism: per
rotation the key products of the ROTATED lifted digits plus P sigma(c0) on component 0, summed over the rotations modulo each limb, then the exact
(X - centred(X mod P)) / P plus both components of the input.  Everything is taken in the coefficient domain: the transform is linear and NTT(sigma_g y) is
the gather perm_g of NTT(y), so these are the words of INTT(S_t).  A plain helper, like the module it builds on."""
import numpy as np

from switch_key_grouped_ref import centred, crt, key_products, lift, product


def sum_qp(orc, data, ct, elts, keys, Ld, alpha):
    """ct [2][Ld][N], keys [R][beta][2][L][N] -> INTT(S) [2][L][N] over Q P; orc spans all L limbs, data the first Ld"""
    q, P = orc.moduli, product(orc.moduli[Ld:])
    qcol, pcol = np.array(q, np.uint64)[:, None], np.array([P % m for m in q[:Ld]], np.uint64)[:, None]
    lifted, S = lift(ct[1], q, Ld, alpha), np.zeros((2, len(q), ct.shape[-1]), np.uint64)
    for g, key in zip(elts, keys):
        S = (S + key_products(orc, orc.apply_galois(lifted, g), key)) % qcol                       # (below 2^61: no wrap)
        S[0, :Ld] = (S[0, :Ld] + data.dyadic("mul", data.apply_galois(ct[0], g), np.ascontiguousarray(np.broadcast_to(pcol, ct[0].shape)))) % qcol[:Ld]
    return S


def divide_and_add(S, ct, moduli, Ld, at):
    """-> {(comp, k): the Ld output words} at the coefficients `at`: ct + round(X / P), both components"""
    P, out = product(moduli[Ld:]), {}
    for comp in range(2):
        for k, x in zip(at, crt([[S[comp, i, k] for k in at] for i in range(len(moduli))], moduli)):
            y = (x - centred(x % P, P)) // P
            out[comp, k] = [(y + int(ct[comp, j, k])) % int(moduli[j]) for j in range(Ld)]
    return out
