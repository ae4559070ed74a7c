"""Shared by the tests of the all-pairs (outer) tensor product (csrc/mul_outer.h, dpfhe_ct_mul_outer): the planted word columns, the Python-integer reference
and the output layouts.

A COLUMN is one word position of one limb: the words (a0_i, a1_i) of A queries and (b0_j, b1_j) of B keys, all canonical, and the A x B triples
    (a0_i b0_j,  a0_i b1_j + a1_i b0_j,  a1_i b1_j) mod q
they must give.  The planted columns put the operands on 0, 1 and q - 1, on the words whose 30-bit halves are largest (q - 1: high half 2^30 - 1;
2^60 - 2^30 - 1: low half 2^30 - 1 - the pair that maximises the lazy form's columns, where such a word is below q), and the keys where their product with
one query lands on 0, 1, q - 1 and either side of q / 2."""
import numpy as np

SIZES = (1, 3, 4, 5, 9)                  # below, at and past the tile (4) and the load-ahead depth (4): ragged tiles, ragged ends of the key loop, two of each
Q_KINDS = ("random", "qm1", "one", "lowmax", "zero", "mixed", "random")
K_KINDS = ("random", "qm1", "land_0", "one", "land_1", "lowmax", "land_qm1", "zero", "land_half", "mixed", "land_half_p1")
TARGETS = {"land_0": lambda q: 0, "land_1": lambda q: 1, "land_qm1": lambda q: q - 1, "land_half": lambda q: q // 2, "land_half_p1": lambda q: q // 2 + 1}


def lowmax(q):
    """the largest canonical word whose LOW 30-bit half is 2^30 - 1 (primes above 2^60 - 2^30: every fold prime), else q - 1"""
    w = (1 << 60) - (1 << 30) - 1
    return w if w < q else q - 1


def want(q, a0, a1, b0, b1):
    a0, a1, b0, b1 = int(a0), int(a1), int(b0), int(b1)
    return a0 * b0 % q, (a0 * b1 + a1 * b0) % q, a1 * b1 % q


def _plain(q, kind, rng):
    return {"qm1": (q - 1, q - 1), "one": (1, 1), "zero": (0, 0), "lowmax": (lowmax(q), lowmax(q)), "mixed": (q - 1, lowmax(q))}.get(kind) or \
        (int(rng.integers(0, q)), int(rng.integers(0, q)))


def column(q, A, B, rng, first=0):
    """(a0, a1, b0, b1): lists of A, A, B, B Python integers in [0, q).  Query i is of kind Q_KINDS[(first + i) % len], key j of K_KINDS[(first + j) % len]; a
    landing key is solved against query j % A: d0 = d1 = target, or with a0 = 0 there d1 = d2 = target"""
    a0, a1, b0, b1 = [], [], [], []
    for i in range(A):
        x, y = _plain(q, Q_KINDS[(first + i) % len(Q_KINDS)], rng)
        a0.append(x); a1.append(y)
    for j in range(B):
        kind = K_KINDS[(first + j) % len(K_KINDS)]
        if kind in TARGETS:
            t, x0, x1 = TARGETS[kind](q), a0[j % A], a1[j % A]
            if x0:
                u = t * pow(x0, -1, q) % q
                v = (t - x1 * u) * pow(x0, -1, q) % q
                assert want(q, x0, x1, u, v)[:2] == (t, t)
            elif x1:
                u = v = t * pow(x1, -1, q) % q
                assert want(q, x0, x1, u, v)[1:] == (t, t)
            else:
                u, v = _plain(q, "random", rng)
        else:
            u, v = _plain(q, kind, rng)
        b0.append(u); b1.append(v)
    return a0, a1, b0, b1


def products(q, a0, a1, b0, b1):
    """[A][B] triples in Python integers"""
    return [[want(q, x0, x1, y0, y1) for y0, y1 in zip(b0, b1)] for x0, x1 in zip(a0, a1)]


def planted_operands(moduli, n, A, B, seed):
    """a [A][2][L][n], b [B][2][L][n] uint64 whose word position w of limb l is column(first = w), and the [A][B][3][L][n] words of all their products.  What
    the NTT-domain form of dpfhe_ct_mul_outer is held to with no transform in between."""
    rng = np.random.default_rng(seed)
    L = len(moduli)
    a = np.zeros((A, 2, L, n), dtype=np.uint64)
    b = np.zeros((B, 2, L, n), dtype=np.uint64)
    out = np.zeros((A, B, 3, L, n), dtype=np.uint64)
    for l, q in enumerate(moduli):
        for w in range(n):
            a0, a1, b0, b1 = column(q, A, B, rng, first=w)
            a[:, 0, l, w], a[:, 1, l, w], b[:, 0, l, w], b[:, 1, l, w] = a0, a1, b0, b1
            out[:, :, :, l, w] = products(q, a0, a1, b0, b1)
    return a, b, out


def full_layout(prods):
    """[A][B][...] -> the entry's full form: pair (i, j) at item i * B + j"""
    return prods.reshape((-1,) + prods.shape[2:])


def causal_layout(prods):
    """[T][T][...] -> the entry's causal form: pair (i, j <= i) at item i (i + 1) / 2 + j"""
    T = prods.shape[0]
    assert prods.shape[1] == T
    return np.stack([prods[i, j] for i in range(T) for j in range(i + 1)])
