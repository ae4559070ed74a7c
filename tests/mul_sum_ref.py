"""Shared by the tests of the sum of tensor products (csrc/mul_sum.h, dpfhe_ct_mul_sum): the planted word columns and the Python-integer reference.

A COLUMN is one word position of one limb: four lists of `terms` canonical words (a0, a1, b0, b1) and the three words
    (sum a0 b0, sum (a0 b1 + a1 b0), sum a1 b1) mod q
they must give.  The planted columns put the sums where a reduction can go wrong: the largest products, and results solved to land on 0, 1, q - 1 and
either side of q / 2."""
import numpy as np

# terms: the small counts, one past a power of two, a long sum, and around every fold period of the lazy form in PRODUCTS (8 for each component: p - 1, p,
# p + 1, 2 p + 1 products are 7, 8, 9, 17 terms for the outer components and 3 / 4, 4, 4 / 5, 8 / 9 terms for the middle one, which takes two per term)
TERMS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 64)
KINDS = ("random", "all_max", "max_times_one", "land_0", "land_1", "land_qm1", "land_half", "land_half_p1")


def want(q, a0, a1, b0, b1, prev=(0, 0, 0)):
    """the three words in Python integers"""
    d0, d1, d2 = (int(v) for v in prev)
    for x0, x1, y0, y1 in zip(a0, a1, b0, b1):
        x0, x1, y0, y1 = int(x0), int(x1), int(y0), int(y1)
        d0 += x0 * y0
        d1 += x0 * y1 + x1 * y0
        d2 += x1 * y1
    return d0 % q, d1 % q, d2 % q


def column(q, terms, kind, rng):
    """(a0, a1, b0, b1): lists of `terms` Python integers in [0, q)"""
    rnd = lambda: [int(rng.integers(0, q)) for _ in range(terms)]
    if kind == "random":
        return rnd(), rnd(), rnd(), rnd()
    if kind == "all_max":
        return tuple([q - 1] * terms for _ in range(4))
    if kind == "max_times_one":
        return [q - 1] * terms, [q - 1] * terms, [1] * terms, [1] * terms
    target = {"land_0": 0, "land_1": 1, "land_qm1": q - 1, "land_half": q // 2, "land_half_p1": q // 2 + 1}[kind]
    if terms == 1:                                   # (1, 0) (x) (t, t) = (t, t, 0)
        return [1], [0], [target], [target]
    # random terms, then two solving ones: (1, 0) (x) (x, y) = (x, y, 0) and (0, 1) (x) (0, z) = (0, 0, z)
    a0, a1, b0, b1 = ([v for v in col[:terms - 2]] for col in (rnd(), rnd(), rnd(), rnd()))
    s0, s1, s2 = want(q, a0, a1, b0, b1)
    a0 += [1, 0]; a1 += [0, 1]
    b0 += [(target - s0) % q, 0]; b1 += [(target - s1) % q, (target - s2) % q]
    assert want(q, a0, a1, b0, b1) == (target, target, target)
    return a0, a1, b0, b1


def planted_operands(moduli, n, terms, seed):
    """a, b: [terms][2][L][n] uint64 whose word position w of limb l is column KINDS[w % len(KINDS)] (fresh random draws per position), and the
    [3][L][n] words of their sum of tensor products.  What the NTT-domain form of dpfhe_ct_mul_sum is held to with no transform in between."""
    rng = np.random.default_rng(seed)
    L = len(moduli)
    a = np.zeros((terms, 2, L, n), dtype=np.uint64)
    b = np.zeros((terms, 2, L, n), dtype=np.uint64)
    out = np.zeros((3, L, n), dtype=np.uint64)
    for l, q in enumerate(moduli):
        for w in range(n):
            a0, a1, b0, b1 = column(q, terms, KINDS[w % len(KINDS)], rng)
            a[:, 0, l, w], a[:, 1, l, w], b[:, 0, l, w], b[:, 1, l, w] = a0, a1, b0, b1
            out[:, l, w] = want(q, a0, a1, b0, b1)
    return a, b, out
