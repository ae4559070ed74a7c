"""Shared by the tests of the products with a shared complement factor (csrc/mul_complement.h, dpfhe_ct_mul_complement): the planted word columns and the
Python-integer reference, on tests/mul_sum_ref.py's builders (`want` is the tensor product, KINDS the landing targets).

A COLUMN is one word position of one limb of one group: the two words (b0, b1) of the denominator, the limb's kappa, and two lists of `items` canonical words
(x0, x1) - the group's numerators.  The factor is f = (kappa - b0, -b1) mod q, canonical (the negation of 0 is 0), and item k must give
    (x0_k f0,  x0_k f1 + x1_k f0,  x1_k f1) mod q.
The planted columns put the factor on its edges (f0 = 0, f0 = kappa, f0 = q - 1, f1 = 0, f1 = q - 1) and the products where a reduction can go wrong: the
largest words, and results solved to land on 0, 1, q - 1 and either side of q / 2."""
import numpy as np

import mul_sum_ref as ms

ITEMS = (1, 4, 5, 9)                      # below, at and past the load-ahead depth (4), and two blocks and a ragged item
B_KINDS = ("b0_kappa", "b0_zero", "b0_kappa_p1", "b1_zero", "b1_one", "random", "all_max")
KAPPA_KINDS = ("zero", "one", "qm1", "random")


def kappa_of(q, kind, rng):
    return {"zero": 0, "one": 1, "qm1": q - 1}.get(kind, int(rng.integers(0, q)))


def factor(q, b0, b1, kappa):
    """(kappa - b0, -b1) mod q in Python integers: canonical by construction"""
    return (int(kappa) - int(b0)) % q, (-int(b1)) % q


def want(q, x0, x1, b0, b1, kappa):
    """[items] triples in Python integers"""
    f0, f1 = factor(q, b0, b1, kappa)
    return [ms.want(q, [a], [b], [f0], [f1]) for a, b in zip(x0, x1)]


def denominator(q, kappa, kind, rng):
    rnd = lambda: int(rng.integers(0, q))
    return {"b0_kappa": (kappa, rnd()),              # f0 = 0
            "b0_zero": (0, rnd()),                   # f0 = kappa
            "b0_kappa_p1": ((kappa + 1) % q, rnd()),   # f0 = q - 1
            "b1_zero": (rnd(), 0),                   # f1 = 0: the negation must stay 0
            "b1_one": (rnd(), 1),                    # f1 = q - 1
            "random": (rnd(), rnd()),
            "all_max": (q - 1, q - 1)}[kind]


def numerators(q, items, f0, f1, rng, first=0):
    """x0, x1: `items` words each; item k is of kind ms.KINDS[(first + k) % len]: random, the largest words, or solved so that the products land on a target"""
    x0, x1 = [], []
    for k in range(items):
        kind = ms.KINDS[(first + k) % len(ms.KINDS)]
        if kind == "random":
            a, b = int(rng.integers(0, q)), int(rng.integers(0, q))
        elif kind in ("all_max", "max_times_one"):
            a, b = q - 1, q - 1
        else:
            t = {"land_0": 0, "land_1": 1, "land_qm1": q - 1, "land_half": q // 2, "land_half_p1": q // 2 + 1}[kind]
            if f0:      # d0 = x0 f0 = t and d1 = x0 f1 + x1 f0 = t
                a = t * pow(f0, -1, q) % q
                b = (t - a * f1) * pow(f0, -1, q) % q
                assert ms.want(q, [a], [b], [f0], [f1])[:2] == (t, t)
            elif f1:    # f0 = 0: d1 = x0 f1 = t and d2 = x1 f1 = t
                a = b = t * pow(f1, -1, q) % q
                assert ms.want(q, [a], [b], [f0], [f1])[1:] == (t, t)
            else:
                a, b = int(rng.integers(0, q)), int(rng.integers(0, q))
        x0.append(a); x1.append(b)
    return x0, x1


def planted_operands(moduli, n, terms, kappas, seed):
    """a [terms][2][L][n], b [2][L][n] uint64 whose word position w of limb l is the column with denominator kind B_KINDS[w % len] under kappas[l], the
    numerators' kinds starting at w, and the [terms + 1][3][L][n] words of the products, the self product b (x) f last.  What the NTT-domain form of
    dpfhe_ct_mul_complement is held to with no transform in between."""
    rng = np.random.default_rng(seed)
    L = len(moduli)
    a = np.zeros((terms, 2, L, n), dtype=np.uint64)
    b = np.zeros((2, L, n), dtype=np.uint64)
    out = np.zeros((terms + 1, 3, L, n), dtype=np.uint64)
    for l, q in enumerate(moduli):
        for w in range(n):
            b0, b1 = denominator(q, kappas[l], B_KINDS[w % len(B_KINDS)], rng)
            f0, f1 = factor(q, b0, b1, kappas[l])
            x0, x1 = numerators(q, terms, f0, f1, rng, first=w)
            b[0, l, w], b[1, l, w] = b0, b1
            if terms:
                a[:, 0, l, w], a[:, 1, l, w] = x0, x1
            out[:, :, l, w] = want(q, x0 + [b0], x1 + [b1], b0, b1, kappas[l])
    return a, b, out
