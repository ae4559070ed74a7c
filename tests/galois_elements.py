"""The Galois elements the rotation tests run, and the two maps they select, stated with Python integers (a plain helper like tests/rotate_add_ref.py: no
conftest, no plugin, no test).

The group of odd residues mod 2N is {+-3^k}.  Which branch a position map takes is decided by the 2-adic shape of g, so the edges are chosen by it:

  g = 1 mod 2^j     fixes the top j - 1 bits of every bit-reversed position: from 2^j = 2 W every wave of a one-piece gather of W = N / 1024 waves is its own
                    source region (mod 8 at N = 4096), from 2^j = 2 N1 every sub-block of a split transform its own source (3^(2^k) = 1 + 2^(k+2) mod 2^(k+3)
                    from k = 1: the slot-sum ladders run these);
  g = -1 mod 2^j    reverses the order inside the blocks instead;
  g near 2N         makes the 32-bit products g * r the largest (2^33 before the mask at N = 65536);
  the negative half {-3^k} swaps the slot rows as well: t - 1, t - 3, t - 2^j +- 1, n - 1.

sigma and src_pos are the definitions, independent of oracle.c and of the library: a scatter of monomials, and the evaluation-point identity."""

import numpy as np

EDGE_COUNTS = {8: 37, 12: 61, 14: 73, 16: 85}    # len(edge_elements(ln)): 6 ln - 11 (from ln = 13 more than one 64-element launch group)


def all_elements(ln):
    """every odd g < 2N"""
    return list(range(1, 2 << ln, 2))


def edge_elements(ln):
    n = 1 << ln
    t = 2 * n
    elts = [1, 3, pow(3, -1, t), 5, t - 1, t - 3, n - 1, n + 1, pow(3, 77, t)]
    for j in range(2, ln + 1):
        elts += [(1 << j) + 1, (1 << j) - 1, t - (1 << j) + 1, t - (1 << j) - 1]
    for k in range(ln - 1):
        elts += [pow(3, 1 << k, t), pow(3, -(1 << k), t)]
    out = []
    for g in elts:
        g %= t
        assert g & 1 and 0 < g < t
        if g not in out:
            out.append(g)
    assert len(out) == 6 * ln - 11, (ln, len(out))    # 37 at 8, 61 at 12, 73 at 14, 85 at 16
    return out


def sigma(a, g, q):
    """a(X) -> a(X^g) mod (X^N + 1, q): coefficient i goes to i g mod 2N, negated when that is >= N"""
    n = len(a)
    out = [0] * n
    for i, v in enumerate(a):
        j = i * g % (2 * n)
        out[j % n] = (-int(v)) % q if j >= n else int(v)
    return out


def brv(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def src_pos(g, p, ln):
    """forward-output position p carries the evaluation at psi^(2 brv(p) + 1): NTT(sigma_g a)[p] = NTT(a)[p'] with 2 brv(p') + 1 = g (2 brv(p) + 1) mod 2N"""
    e2 = g * (2 * brv(p, ln) + 1) % (2 << ln)
    return brv((e2 - 1) // 2, ln)


def brv_table(bits):
    """[brv(x, bits) for every x < 2^bits], int64"""
    rev = np.zeros(1 << bits, np.int64)
    for b in range(bits):
        rev |= ((np.arange(1 << bits, dtype=np.int64) >> b) & 1) << (bits - 1 - b)
    return rev


def src_pos_table(g, ln):
    """[src_pos(g, p, ln) for every p] in int64 (g (2 brv(p) + 1) < 2^35: nothing wraps); the tests hold it to src_pos itself"""
    rev = brv_table(ln)
    return rev[((int(g) * (2 * rev + 1)) % (2 << ln) - 1) >> 1]


def sigma_words(a, g, q):
    """sigma on a numpy array [..., N] of canonical residues (uint64; indices in int64); the tests hold it to sigma itself"""
    n = a.shape[-1]
    j = (np.arange(n, dtype=np.int64) * int(g)) % (2 * n)
    out = np.empty_like(a)
    neg = np.where(a == 0, a, np.uint64(q) - a)
    out[..., j % n] = np.where(j >= n, neg, a)
    return out
