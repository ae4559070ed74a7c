"""What the tests of tests/golden/sympy_anchor.json share: the fixture, the inputs its seeds stand for, and the comparison of a buffer with an anchor.

The fixture (tests/golden/make_golden.py sympy_anchor) holds, per anchored output buffer, the seed of its input, the SHA-256 of its words, the first and last
8 words and 32 sampled words.  This module imports nothing of oracle/: the splitmix64 stream and the input layouts are restated here with numpy (the CPU
test holds them to the generator's), so that the GPU test reaches its expected words through sympy's arithmetic alone.
"""
import functools
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sympy_anchor.json")
TRANSFORM_LOG2NS = (12, 13, 14, 15, 16)


@functools.lru_cache(maxsize=None)
def fixture():
    with open(GOLDEN) as f:
        return json.load(f)


def transform_records(log2n):
    return fixture()["transforms_log2n%d" % log2n]


def splitmix_words(seed, count):
    """the first `count` outputs of splitmix64(seed), vectorised: the state before output i is seed + (i + 1) gamma"""
    z = np.uint64(seed) + np.arange(1, count + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def fill(kind, seed, moduli_seq, n):
    """make_golden.anchor_fill: one polynomial of n words per entry of moduli_seq -> uint64 [len(moduli_seq)][n]"""
    qcol = np.array(list(moduli_seq), np.uint64)[:, None]
    if kind == "random":
        return splitmix_words(seed, qcol.size * n).reshape(qcol.size, n) % qcol
    if kind == "qm1":
        return np.ascontiguousarray(np.broadcast_to(qcol - np.uint64(1), (qcol.size, n)))
    if kind == "monomial":
        out = np.zeros((qcol.size, n), np.uint64)
        out[:, n - 1] = 1
        return out
    raise ValueError(kind)


def multiply_operands(rec):
    """the operands of a multiply anchor: a, b uint64 [2][L][N]"""
    n, moduli = 1 << rec["log2n"], rec["moduli"]
    L = len(moduli)
    if rec["input"] == "random":
        ab = fill("random", rec["seed"], moduli * 4, n).reshape(2, 2, L, n)
        return np.ascontiguousarray(ab[0]), np.ascontiguousarray(ab[1])
    assert rec["input"] == "extremes"
    qm1, mono = fill("qm1", 0, moduli, n), fill("monomial", 0, moduli, n)
    return np.stack([qm1, mono]), np.stack([mono, qm1])


def key_moduli(moduli, digits):
    """the prime of every polynomial of a key [digits][2][L][N]"""
    return [q for _ in range(digits) for _ in range(2) for q in moduli]


def digest(words):
    return hashlib.sha256(np.ascontiguousarray(words, dtype=np.uint64).astype("<u8").tobytes()).hexdigest()


def mismatches(rec, words, n):
    """[] if `words` is the anchored buffer; otherwise where the kept words differ: the digest says that something is wrong, the per-polynomial digests and
    the sampled words say where"""
    w = np.ascontiguousarray(words, dtype=np.uint64).ravel()
    if w.size != rec["words"]:
        return ["%d words, the anchor has %d" % (w.size, rec["words"])]
    if digest(w) == rec["sha256"]:
        return []
    bad = []
    for i, want in enumerate(rec.get("poly_sha256", ())):
        if digest(w[i * n:(i + 1) * n]) != want:
            bad.append("polynomial %d" % i)
    positions = list(range(8)) + list(range(w.size - 8, w.size)) + fixture()["positions"][str(w.size)]
    for pos, want in zip(positions, rec["head"] + rec["tail"] + rec["samples"]):
        if int(w[pos]) != want:
            bad.append("word %d: %d, the anchor has %d" % (pos, int(w[pos]), want))
    return bad or ["the SHA-256 differs (every kept word agrees)"]


def assert_anchor(rec, words, n, label=""):
    bad = mismatches(rec, words, n)
    assert not bad, (label, rec.get("name", rec.get("op")), rec.get("input"), bad[:12])


# ---- the Galois identity: (sigma_g a)(rho) = a(rho^g) at sampled primitive 2N-th roots rho = psi^odd --------------------------------------------------
GALOIS_POINTS = 32


def horner(coeffs, point, q):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * point + c) % q
    return acc


def galois_identity_failures(a, rotated, g, q, psi, seed):
    """a, rotated: one polynomial each (N words, coefficient domain); the sampled points at which rotated(rho) != a(rho^g), rho = psi^e, e odd, evaluated
    by Horner's rule on Python integers"""
    a, rotated = [int(v) for v in a], [int(v) for v in rotated]
    n = len(a)
    exps = 2 * (splitmix_words(seed, GALOIS_POINTS) % np.uint64(n)) + np.uint64(1)
    bad = []
    for e in (int(v) for v in exps):
        rho = pow(psi, e, q)
        if horner(rotated, rho, q) != horner(a, pow(rho, g, q), q):
            bad.append(e)
    return bad


def galois_elements(n):
    return (3, 5, n + 1, 2 * n - 1)
