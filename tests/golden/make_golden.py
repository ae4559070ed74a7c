"""Generates tests/golden/*.json from the Python big-int oracle (oracle/pyoracle.py) - and two fixtures from sympy alone, a third,
builder-independent route to the same words: sympy_restatement (whole vectors at N = 64 and 256) and sympy_anchor (digests and sampled words at the
metric rings N = 4096 ... 65536: transforms, the tensor product, rescale / base extension / scale-and-round, key switching; minutes to run).

The reference holds no golden vectors for this path ("Golden vectors /
known-answer tests: none of any kind"), so these are known answers of the mathematical definition,
produced by pure-Python big-int schoolbook / O(N^2) direct evaluation - code that shares nothing
with the C oracle or the HIP kernels.  Run from the repo root:  python tests/golden/make_golden.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import pyoracle as po  # noqa: E402
from deeppowers_amd.params import PRIMES_60, PRIME_30, PSI_30_N1024  # noqa: E402


def sha(words):
    return hashlib.sha256(po.words_to_bytes(words)).hexdigest()


def small_ntt_vectors():
    """Full forward-NTT vectors at N=16, 64 by direct O(N^2) evaluation (several primes)."""
    out = []
    for log2n in (3, 4, 6):
        n = 1 << log2n
        for q, psi8192 in ((PRIME_30, None), (PRIMES_60[0][0], PRIMES_60[0][2]), (PRIMES_60[3][0], PRIMES_60[3][2])):
            if psi8192 is None:
                psi = pow(PSI_30_N1024, 1024 // n, q)
            else:
                psi = pow(psi8192, 8192 // n, q)
            assert po.is_primitive_2n_root(psi, n, q)
            g = po.SplitMix64(1000 * log2n + (q & 0xFF))
            a = g.words_mod(n, q)
            ahat = po.ntt_forward_definition(a, q, psi)
            assert po.ntt_forward(a, q, psi) == ahat and po.ntt_inverse(ahat, q, psi) == a
            out.append({"log2n": log2n, "q": q, "psi": psi, "a": a, "ntt": ahat})
    return out


def config1_ct_mul():
    """SURVEY.md Appendix B config-1 vector: N=1024, q=1073707009, splitmix64(seed=1), a0,a1,b0,b1."""
    q, n = PRIME_30, 1024
    g = po.SplitMix64(1)
    a0, a1, b0, b1 = (g.words_mod(n, q) for _ in range(4))
    c = po.ct_mul_schoolbook([[a0], [a1]], [[b0], [b1]], [q])
    c0, c1, c2 = c[0][0], c[1][0], c[2][0]
    return {
        "log2n": 10, "q": q, "psi": PSI_30_N1024, "seed": 1,
        "a0_head": a0[:4], "c0_head": c0[:4], "c1_head": c1[:4], "c2_head": c2[:4],
        "sha256": {"c0": sha(c0), "c1": sha(c1), "c2": sha(c2), "c0c1c2": sha(c0 + c1 + c2)},
        "c0": c0, "c1": c1, "c2": c2,
    }


def rns_ct_mul_small():
    """A 2-limb, N=64, batch=2 ct x ct product with 60-bit primes (layout [batch][comp][limb][N])."""
    log2n, n = 6, 64
    moduli = [PRIMES_60[0][0], PRIMES_60[1][0]]
    psis = [pow(PRIMES_60[0][2], 8192 // n, moduli[0]), pow(PRIMES_60[1][2], 8192 // n, moduli[1])]
    g = po.SplitMix64(42)
    batch = 2
    A, B, Cc = [], [], []
    for _ in range(batch):
        a = [[g.words_mod(n, q) for q in moduli] for _ in range(2)]
        b = [[g.words_mod(n, q) for q in moduli] for _ in range(2)]
        c = po.ct_mul_schoolbook(a, b, moduli)
        assert po.ct_mul_ntt(a, b, moduli, psis) == c
        A += po.flatten_ct(a); B += po.flatten_ct(b); Cc += po.flatten_ct(c)
    return {"log2n": log2n, "moduli": moduli, "psi": psis, "batch": batch, "a": A, "b": B, "c": Cc}


def rns_ct_mul_n256():
    """2 limbs (one fold-eligible 60-bit prime, the 30-bit prime), N=256, batch=3: smallest size the
    HIP C-ABI dispatches (log2_n >= 8), so the GPU tests can replay a pure big-int vector."""
    log2n, n = 8, 256
    moduli = [PRIMES_60[2][0], PRIME_30]
    psis = [pow(PRIMES_60[2][2], 8192 // n, moduli[0]), pow(PSI_30_N1024, 1024 // n, moduli[1])]
    g = po.SplitMix64(256)
    batch = 3
    A, B, Cc = [], [], []
    for _ in range(batch):
        a = [[g.words_mod(n, q) for q in moduli] for _ in range(2)]
        b = [[g.words_mod(n, q) for q in moduli] for _ in range(2)]
        c = po.ct_mul_schoolbook(a, b, moduli)
        A += po.flatten_ct(a); B += po.flatten_ct(b); Cc += po.flatten_ct(c)
    ntt_a0 = [po.ntt_forward(A[l * n:(l + 1) * n], moduli[l], psis[l]) for l in range(2)]
    return {"log2n": log2n, "moduli": moduli, "psi": psis, "batch": batch, "a": A, "b": B,
            "c_sha256": sha(Cc), "c_head": Cc[:8], "c_tail": Cc[-8:], "ntt_a0_limb0_head": ntt_a0[0][:8],
            "ntt_a0_sha256": sha(ntt_a0[0] + ntt_a0[1])}


def identities():
    """Hand-checkable products + NTT(delta_0), NTT(X)."""
    n, q = 8, 17
    out = {
        "n8_q17_a": list(range(1, 9)), "n8_q17_b": list(range(8, 0, -1)),
        "n8_q17_ab": po.negacyclic_schoolbook(list(range(1, 9)), list(range(8, 0, -1)), q),
        "n8_q17_1pX_times_X7": po.negacyclic_schoolbook([1, 1, 0, 0, 0, 0, 0, 0], [0] * 7 + [1], q),
    }
    q, psi, n = PRIMES_60[0][0], PRIMES_60[0][1], 4096
    out["ntt_X_n4096_q0_head"] = po.ntt_forward([0, 1] + [0] * (n - 2), q, psi)[:8]
    out["ntt_X_n4096_q0_sha256"] = sha(po.ntt_forward([0, 1] + [0] * (n - 2), q, psi))
    return out


def n4096_ntt_digest():
    """One full-size residue polynomial per limb of the metric configuration: digest of NTT(a)."""
    n = 4096
    res = []
    for l in range(4):
        q, psi = PRIMES_60[l][0], PRIMES_60[l][1]
        a = po.SplitMix64(2000 + l).words_mod(n, q)
        ah = po.ntt_forward(a, q, psi)
        assert po.ntt_inverse(ah, q, psi) == a
        res.append({"limb": l, "q": q, "psi": psi, "seed": 2000 + l, "a_head": a[:4], "ntt_head": ah[:4], "ntt_sha256": sha(ah)})
    return res


def sympy_restatement():
    """A THIRD restatement, written by neither this build's oracle authors nor its kernel authors: sympy's polynomial ring over GF(q) and sympy's
    number-theoretic transform (sympy 1.14, already in the image; tests/test_params.py uses it for primality).  Nothing of oracle/ is called to
    PRODUCE these values (pyoracle only draws the inputs and is compared afterwards):
      * N = 256, two limbs (a pinned 60-bit prime and the 30-bit prime): the ct x ct tensor product as sympy Poly products over GF(q) reduced by X^N + 1;
      * N = 64, the same two primes: the forward negacyclic NTT (i) by evaluating the sympy polynomial at psi^(2 brv(k) + 1) and (ii) through
        sympy.discrete.transforms.ntt of the psi-twisted sequence, re-indexed from sympy's root of unity to ours."""
    import sympy
    from sympy import GF, Poly, symbols
    from sympy.discrete.transforms import ntt as sympy_ntt
    from sympy.ntheory import primitive_root
    x = symbols("x")

    def poly(c, q):
        return Poly(list(reversed(c)), x, domain=GF(q, symmetric=False))

    def coeffs(pl, n, q):
        c = [int(v) % q for v in reversed(pl.all_coeffs())]
        return c + [0] * (n - len(c))

    out = {"sympy_version": sympy.__version__}
    # ---- ct x ct at N = 256, two limbs, batch 2 ----
    log2n, n = 8, 256
    moduli = [PRIMES_60[2][0], PRIME_30]
    g = po.SplitMix64(2560)
    A, B, Cc = [], [], []
    for _ in range(2):
        a = [[g.words_mod(n, q) for q in moduli] for _ in range(2)]
        b = [[g.words_mod(n, q) for q in moduli] for _ in range(2)]
        c = [[None] * len(moduli) for _ in range(3)]
        for l, q in enumerate(moduli):
            m = Poly(x**n + 1, x, domain=GF(q, symmetric=False))
            a0, a1, b0, b1 = (poly(v[l], q) for v in (a[0], a[1], b[0], b[1]))
            c[0][l] = coeffs((a0 * b0).rem(m), n, q)
            c[1][l] = coeffs((a0 * b1 + a1 * b0).rem(m), n, q)
            c[2][l] = coeffs((a1 * b1).rem(m), n, q)
        A += po.flatten_ct(a); B += po.flatten_ct(b); Cc += po.flatten_ct(c)
    out["ct_mul_n256"] = {"log2n": log2n, "moduli": moduli, "psi": [pow(PRIMES_60[2][2], 8192 // n, moduli[0]), pow(PSI_30_N1024, 1024 // n, moduli[1])],
                          "batch": 2, "a": A, "b": B, "c": Cc}
    # ---- forward NTT at N = 64 ----
    log2n, n = 6, 64
    vecs = []
    for q, psi in ((PRIMES_60[2][0], pow(PRIMES_60[2][2], 8192 // n, PRIMES_60[2][0])), (PRIME_30, pow(PSI_30_N1024, 1024 // n, PRIME_30))):
        a = po.SplitMix64(640 + (q & 0xFF)).words_mod(n, q)
        pa = poly(a, q)
        brv = lambda k: int(format(k, "0%db" % log2n)[::-1], 2)
        by_eval = [int(pa.eval(pow(psi, 2 * brv(k) + 1, q))) % q for k in range(n)]
        # (ii) cyclic transform of the twisted sequence with sympy's own root rt = g^((q-1)/n); ours is omega = psi^2 = rt^t
        twisted = [a[j] * pow(psi, j, q) % q for j in range(n)]
        cyc = [int(v) % q for v in sympy_ntt(twisted, prime=q)]
        rt = pow(primitive_root(q), (q - 1) // n, q)
        omega = psi * psi % q
        t = next(t for t in range(1, n, 2) if pow(rt, t, q) == omega)      # omega^(j k) = rt^(j (t k)):  ours[k] = sympy[t k mod n]
        by_ntt = [cyc[(t * brv(k)) % n] for k in range(n)]
        assert by_eval == by_ntt, "sympy's two routes disagree"
        vecs.append({"log2n": log2n, "q": q, "psi": psi, "a": a, "ntt": by_eval})
    out["ntt_n64"] = vecs
    return out


# ---- the second sympy-only fixture: anchors at the metric rings ----------------------------------------------------------------------------------
ANCHOR_POSITION_SEED = 0x5A17C4
ANCHOR_SAMPLES = 32
ANCHOR_CHEAP = ("transforms_log2n12", "integer")     # the sections tests/test_sympy_anchor_cpu.py re-runs


def anchor_positions(length):
    """the 32 sampled word positions of an anchored buffer of `length` words: drawn once per length from a fixed seed, sorted, distinct"""
    g, seen = po.SplitMix64(ANCHOR_POSITION_SEED + length), []
    while len(seen) < ANCHOR_SAMPLES:
        v = g.next() % length
        if v not in seen:
            seen.append(v)
    return sorted(seen)


def anchor_fill(kind, seed, moduli_seq, n):
    """the input buffer of an anchor: one polynomial of n words per entry of moduli_seq, back to back.  'random': one SplitMix64(seed) stream,
    each word reduced modulo its polynomial's prime; 'qm1': q - 1 in every word; 'monomial': X^(N-1) in every polynomial."""
    if kind == "random":
        g = po.SplitMix64(seed)
        return [w for q in moduli_seq for w in g.words_mod(n, q)]
    if kind == "qm1":
        return [q - 1 for q in moduli_seq for _ in range(n)]
    if kind == "monomial":
        return [w for _ in moduli_seq for w in [0] * (n - 1) + [1]]
    raise ValueError(kind)


def anchor_record(words, n, **meta):
    """what the fixture keeps of an output buffer: SHA-256 of all its words (little-endian u64) and of each polynomial of n words, the first 8 and
    the last 8 words, and the words at anchor_positions(len(words))"""
    def digest(w):
        return hashlib.sha256(b"".join(int(v).to_bytes(8, "little") for v in w)).hexdigest()
    rec = dict(meta)
    rec["words"] = len(words)
    rec["sha256"] = digest(words)
    if len(words) > n:
        rec["poly_sha256"] = [digest(words[i:i + n]) for i in range(0, len(words), n)]
    rec["head"], rec["tail"] = list(words[:8]), list(words[-8:])
    rec["samples"] = [words[i] for i in anchor_positions(len(words))]
    return rec


def sympy_anchor(only=None):
    """The builder-independent anchor at the metric rings (tests/golden/sympy_anchor.json), written like sympy_restatement(): every expected word comes
    from sympy (Poly over ZZ / GF(q), sympy.discrete.transforms.ntt / intt, sympy.ntheory.modular.crt) and plain Python integers.  From oracle/pyoracle.py
    only SplitMix64 (to draw inputs) is used; the primes and roots are constants (deeppowers_amd/params.py, the catalogue of tests/class_edges.py) that
    sympy re-checks here (isprime, psi^N = -1).  Full-size vectors do not fit a committed file: an anchored buffer is kept as its input seed, the SHA-256
    of its words, its first and last 8 words and 32 sampled words (anchor_record).  Runs by hand (minutes); `only` names sections to run
    (ANCHOR_CHEAP: what tests/test_sympy_anchor_cpu.py re-runs against the committed file).

    Routes.  Transforms: sympy's cyclic transform of the psi-twisted sequence re-indexed from sympy's root to ours (inverse: intt, re-indexed, untwisted),
    cross-checked at 16 sampled indices per ring degree against Poly.eval.  Products: Poly products over ZZ, folded by X^N + 1 on the coefficient list
    (c[i] - c[i + N]; checked against Poly.rem at N = 1024), reduced mod q.  Integer operations: per coefficient the integer X from crt, then Python
    integer rounding floor((2 m X + D) / (2 D)).  Two facts make those unambiguous: D (a product of odd primes) is odd, so m X / D is never a
    half-integer and no tie rule is involved; and round(m (X - Q) / D) = round(m X / D) - m Q / D with Q / D the product of the kept limbs, so the result
    modulo the kept limbs is the same whether X is read centred or in [0, Q).  (dpfhe_base_extend has no division: there X is the centred value, as
    include/dpfhe.h states.)  Key switching: from the header's formulas, a digit [c]_{q_j} being limb j of c read as integers in [0, q_j); sympy brings
    the (arbitrary, uniform) keys to the coefficient domain, the products are taken over ZZ, and for the hybrid form round(sum / P) is taken over the
    integer crt reconstructs from all limbs."""
    import sympy
    from sympy import GF, ZZ, Poly, isprime, symbols
    from sympy.discrete.transforms import intt as sympy_intt, ntt as sympy_ntt
    from sympy.ntheory import primitive_root
    from sympy.ntheory.modular import crt
    sys.path.insert(0, os.path.dirname(HERE))
    import class_edges                      # (the catalogue of class-edge primes: constants, found with deeppowers_amd.params)
    from deeppowers_amd.params import FheParams, min_primitive_2n_root
    x = symbols("x")
    want = lambda name: only is None or name in only
    out = {"sympy_version": sympy.__version__, "positions": {}}

    def record(words, n, **meta):
        out["positions"].setdefault(str(len(words)), anchor_positions(len(words)))
        return anchor_record(words, n, **meta)

    def checked(q, psi, n):
        assert isprime(q) and (q - 1) % (2 * n) == 0 and pow(psi, n, q) == q - 1, (q, psi, n)
        return q, psi

    def brv(k, bits):
        return int(format(k, "0%db" % bits)[::-1], 2)

    roots = {}

    def sympy_root(q, n):
        """sympy's n-th root of unity rt = g^((q-1)/n) and the odd t with psi^2 = rt^t is found by the caller"""
        if q not in roots:
            roots[q] = primitive_root(q)
        return pow(roots[q], (q - 1) // n, q)

    def root_exponent(q, psi, n):
        rt, omega = sympy_root(q, n), psi * psi % q
        cur, step = rt, rt * rt % q
        for t in range(1, n, 2):
            if cur == omega:
                return t
            cur = cur * step % q
        raise AssertionError("psi^2 is no power of sympy's root")

    def powers(base, n, q):
        pw = [1] * n
        for j in range(1, n):
            pw[j] = pw[j - 1] * base % q
        return pw

    def fwd(a, q, psi):
        """natural in, bit-reversed out: ahat[k] = sum_j a[j] psi^((2 brv(k) + 1) j)"""
        n = len(a)
        bits = n.bit_length() - 1
        pw = powers(psi, n, q)
        cyc = [int(v) % q for v in sympy_ntt([a[j] * pw[j] % q for j in range(n)], prime=q)]
        t = root_exponent(q, psi, n)                        # omega^(j k) = rt^(j (t k)):  ours[k] = sympy[t brv(k) mod n]
        return [cyc[(t * brv(k, bits)) % n] for k in range(n)]

    def inv(ahat, q, psi):
        """bit-reversed in, natural out, N^-1 included: a[j] = N^-1 psi^-j sum_m ahat[brv(m)] omega^(-m j)"""
        n = len(ahat)
        bits = n.bit_length() - 1
        t = root_exponent(q, psi, n)
        seq = [0] * n
        for m in range(n):
            seq[(t * m) % n] = ahat[brv(m, bits)]           # intt(seq)[j] = N^-1 sum_m' seq[m'] rt^(-m' j) = N^-1 sum_m ahat[brv(m)] omega^(-m j)
        b = [int(v) % q for v in sympy_intt(seq, prime=q)]
        ipw = powers(pow(psi, q - 2, q), n, q)
        return [b[j] * ipw[j] % q for j in range(n)]

    def eval_check(a, ahat, q, psi, seed):
        """the second sympy route: Poly.eval of the coefficient polynomial at psi^(2 brv(k) + 1), 16 sampled k"""
        n = len(a)
        bits = n.bit_length() - 1
        pa = Poly(list(reversed(a)), x, domain=GF(q, symmetric=False))
        g = po.SplitMix64(seed)
        for k in [0, n - 1] + [g.next() % n for _ in range(14)]:
            assert int(pa.eval(pow(psi, 2 * brv(k, bits) + 1, q))) % q == ahat[k], "sympy's two routes disagree"

    def zz(c):
        return Poly(list(reversed(c)), x, domain=ZZ) if any(c) else Poly(0, x, domain=ZZ)

    def folded(pl, n):
        """the coefficients of an integer polynomial of degree < 2N - 1 reduced by X^N + 1: c[i] - c[i + N]"""
        c = [int(v) for v in reversed(pl.all_coeffs())]
        c += [0] * (2 * n - len(c))
        return [c[i] - c[i + n] for i in range(n)]

    def negacyclic(a, b, n):
        """a b mod X^N + 1 over the integers (not yet reduced mod q)"""
        return folded(zz(a) * zz(b), n)

    def split(words, n):
        return [words[i:i + n] for i in range(0, len(words), n)]

    def tensor(a, b, moduli, n):
        """a, b flat [2][L][N] -> c flat [3][L][N] = (a0 b0, a0 b1 + a1 b0, a1 b1) per limb"""
        L = len(moduli)
        A, B = split(a, n), split(b, n)
        c = [None] * (3 * L)
        for l, q in enumerate(moduli):
            a0, a1, b0, b1 = A[l], A[L + l], B[l], B[L + l]
            c[l] = [v % q for v in negacyclic(a0, b0, n)]
            c[L + l] = [(u + v) % q for u, v in zip(negacyclic(a0, b1, n), negacyclic(a1, b0, n))]
            c[2 * L + l] = [v % q for v in negacyclic(a1, b1, n)]
        return [w for pl in c for w in pl]

    pinned = lambda i, log2n: checked(PRIMES_60[i][0], PRIMES_60[i][1] if log2n == 12 else PRIMES_60[i][2] if log2n == 13
                                      else min_primitive_2n_root(1 << log2n, PRIMES_60[i][0]), 1 << log2n)
    CLASS_ENTRIES = (("fold", "fold_edge"), ("f64", "f64_edge"), ("fold_scaled", "fscaled_edge_59"), ("f64_wide", "f64_wide_edge"), ("shoup", "shoup60"))

    # ---- a. transforms, forward and inverse ------------------------------------------------------------------------------------------------------
    def transforms(log2n):
        """one prime of each class (log2 N = 12, 13), the pinned primes that admit the ring (all four of the metric configuration at 12 and 13; limbs 1, 2
        and 4 of the pinned six at 14: the others are not 1 mod 2N there; limb 4 at 15 and 16) and, at 15 and 16, the catalogue's first generic prime"""
        n = 1 << log2n
        primes = []
        if log2n in (12, 13):
            cat = class_edges.catalogue(log2n)
            for cls, entry in CLASS_ENTRIES:
                q, psi = checked(*cat[entry][0], n)
                assert class_edges.expected_class(q) == cls
                primes.append((cls, q, psi))
        for i in {12: (0, 1, 2, 3), 13: (0, 1, 2, 3), 14: (1, 2, 4), 15: (4,), 16: (4,)}[log2n]:
            primes.append(("pinned%d" % i,) + pinned(i, log2n))
        if log2n in (15, 16):
            primes.append(("shoup",) + checked(*class_edges.catalogue(log2n)["shoup60"][0], n))
        recs = []
        for pi, (name, q, psi) in enumerate(primes):
            kinds = ("random", "qm1", "monomial") if log2n == 12 and pi < len(CLASS_ENTRIES) else ("random",)
            for kind in kinds:
                for direction, f in (("fwd", fwd), ("inv", inv)):
                    seed = 120000 + 1000 * log2n + 10 * pi + (direction == "inv")
                    a = anchor_fill(kind, seed, [q], n)
                    got = f(a, q, psi)
                    if pi == 0 and kind == "random":
                        eval_check(a, got, q, psi, seed) if direction == "fwd" else eval_check(got, a, q, psi, seed)
                    recs.append(record(got, n, name=name, log2n=log2n, q=q, psi=psi, direction=direction, input=kind, seed=seed))
        return recs

    for log2n in (12, 13, 14, 15, 16):
        if want("transforms_log2n%d" % log2n):
            out["transforms_log2n%d" % log2n] = transforms(log2n)

    # ---- b. the tensor product -------------------------------------------------------------------------------------------------------------------
    if want("multiply"):
        # the fold on the coefficient list against Poly.rem, once, at N = 1024 (BASELINE configuration 1: the case below takes its remainder by Poly.rem)
        n, q = 1024, PRIME_30
        a = anchor_fill("random", 1, [q] * 4, n)                      # config 1's own vector: splitmix64(seed = 1), a0, a1, b0, b1
        a0, a1, b0, b1 = split(a, n)
        gf = lambda c: Poly(list(reversed(c)), x, domain=GF(q, symmetric=False))
        m = Poly(x**n + 1, x, domain=GF(q, symmetric=False))
        coeffs = lambda pl: (lambda c: c + [0] * (n - len(c)))([int(v) % q for v in reversed(pl.all_coeffs())])
        by_rem = coeffs((gf(a0) * gf(b0)).rem(m)) + coeffs((gf(a0) * gf(b1) + gf(a1) * gf(b0)).rem(m)) + coeffs((gf(a1) * gf(b1)).rem(m))
        assert by_rem == tensor(a0 + a1, b0 + b1, [q], n), "the fold by X^N + 1 disagrees with Poly.rem"
        cases = [record(by_rem, n, name="config1_n1024", log2n=10, moduli=[q], psi=[PSI_30_N1024], input="random", seed=1)]

        def mul_case(name, log2n, primes, kind, seed, with_transforms=False):
            n = 1 << log2n
            moduli, psis = [p[0] for p in primes], [p[1] for p in primes]
            if kind == "random":
                ab = anchor_fill("random", seed, moduli * 4, n)       # [a | b], each [2][L][N]
                a, b = ab[:len(ab) // 2], ab[len(ab) // 2:]
            else:                                                     # the extremes: a = (q - 1 everywhere, X^(N-1)), b = (X^(N-1), q - 1 everywhere)
                a = anchor_fill("qm1", 0, moduli, n) + anchor_fill("monomial", 0, moduli, n)
                b = anchor_fill("monomial", 0, moduli, n) + anchor_fill("qm1", 0, moduli, n)
            c = tensor(a, b, moduli, n)
            rec = record(c, n, name=name, log2n=log2n, moduli=moduli, psi=psis, input=kind, seed=seed)
            if with_transforms:                                       # the DPFHE_IN_NTT / DPFHE_OUT_NTT forms: the transforms of the operands and of the product
                ntt_of = lambda w: [v for i, pl in enumerate(split(w, n)) for v in fwd(pl, moduli[i % len(moduli)], psis[i % len(moduli)])]
                rec["ntt_a"], rec["ntt_b"], rec["ntt_c"] = (record(ntt_of(w), n) for w in (a, b, c))
            return rec

        metric = [pinned(i, 12) for i in range(4)]
        cases.append(mul_case("metric_n4096_pair0", 12, metric, "random", 4096001, with_transforms=True))
        cases.append(mul_case("metric_n4096_pair1", 12, metric, "random", 4096002))
        cases.append(mul_case("metric_n4096_extremes", 12, metric, "extremes", 0))
        gp = FheParams.generic_n4096_l4()                             # limbs of 59, 50, 40 and 33 bits: fold_scaled, fold_scaled, f64, f64
        cases.append(mul_case("mixed_n4096", 12, [checked(q, w, 4096) for q, w in zip(gp.moduli, gp.psi)], "random", 4096003))
        cases.append(mul_case("n8192_pinned_f64", 13, [pinned(0, 13), checked(*class_edges.catalogue(13)["f64_edge"][0], 8192)], "random", 8192001))
        out["multiply"] = cases

    # ---- c. integer operations at N = 4096 on the metric configuration -----------------------------------------------------------------------------
    if want("integer"):
        n = 4096
        metric = [pinned(i, 12) for i in range(4)]
        moduli = [p[0] for p in metric]
        prod = lambda qs: int(sympy.prod(qs))

        def lift(columns, qs, k):
            """the integer in [0, prod qs) with residue columns[i][k] modulo qs[i]"""
            return int(crt(qs, [c[k] for c in columns], check=False)[0])

        def rounded(num, den):
            """round(num / den) for odd den (no tie): floor((2 num + den) / (2 den))"""
            assert den % 2 == 1
            return (2 * num + den) // (2 * den)

        recs = []
        for kind, seed in (("random", 4096101), ("qm1", 0)):
            xs = split(anchor_fill(kind, seed, moduli, n), n)
            # dpfhe_rescale, 4 limbs -> 3: round(X / q_3) modulo limbs 0..2
            y = [rounded(lift(xs, moduli, k), moduli[3]) for k in range(n)]
            recs.append(record([v % q for q in moduli[:3] for v in y], n, op="rescale", input=kind, seed=seed))
            # dpfhe_base_extend, source limbs [0, 2) -> destination limbs [0, 4): the centred X in (-Qs/2, Qs/2]
            Qs = prod(moduli[:2])
            X = [lift(xs[:2], moduli[:2], k) for k in range(n)]
            X = [v - Qs if v > Qs // 2 else v for v in X]
            recs.append(record([v % q for q in moduli for v in X], n, op="base_extend", src_limb0=0, n_src=2, dst_limb0=0, n_dst=4, input=kind, seed=seed))
            # dpfhe_scale_round, multiplier 65537, dropping limbs [0, 2), keeping limbs [2, 4)
            y = [rounded(65537 * lift(xs, moduli, k), Qs) for k in range(n)]
            recs.append(record([v % q for q in moduli[2:] for v in y], n, op="scale_round", multiplier=65537, drop_limb0=0, n_drop=2, keep_limb0=2, n_keep=2,
                               input=kind, seed=seed))
        out["integer"] = {"log2n": 12, "moduli": moduli, "psi": [p[1] for p in metric], "cases": recs}

    # ---- d. key switching at N = 4096 on the metric configuration ------------------------------------------------------------------------------------
    if want("keyswitch"):
        n = 4096
        metric = [pinned(i, 12) for i in range(4)]
        moduli, psis = [p[0] for p in metric], [p[1] for p in metric]
        L = 4

        def key_sums(digits, key, Ld):
            """t[comp][i] = sum_j digit_j key_j[comp][i] in Z[X]/(X^N + 1), not yet reduced mod q_i: digit_j = limb j of the switched component, its words
            read as integers in [0, q_j); key flat [Ld][2][L][N] in the NTT domain, brought to the coefficient domain by sympy"""
            K = split(key, n)
            t = [[[0] * n for _ in range(L)] for _ in range(2)]
            for j in range(Ld):
                d = zz(digits[j])
                for comp in range(2):
                    for i in range(L):
                        kc = inv(K[(j * 2 + comp) * L + i], moduli[i], psis[i])
                        t[comp][i] = [u + v for u, v in zip(t[comp][i], folded(d * zz(kc), n))]
            return t

        recs = []
        for kind, seed in (("random", 4096201), ("qm1", 4096202)):
            # dpfhe_relinearize, 4 limbs: (c0, c1) + sum_j [c2]_{q_j} evk_j
            ct = split(anchor_fill(kind, seed, moduli * 3, n), n)                      # [3][L][N]
            evk = anchor_fill("random", seed + 50, [moduli[i] for _ in range(L) for _ in range(2) for i in range(L)], n)
            t = key_sums(ct[2 * L:3 * L], evk, L)
            res = [[(ct[comp * L + i][k] + t[comp][i][k]) % moduli[i] for k in range(n)] for comp in range(2) for i in range(L)]
            recs.append(record([w for pl in res for w in pl], n, op="relinearize", input=kind, seed=seed, key_seed=seed + 50))
            # dpfhe_switch_key_hybrid, 3 data limbs + P = limb 3: (c0, 0) + round(sum_j [c1]_{q_j} key_j / P)
            Ld, P = 3, moduli[3]
            ct = split(anchor_fill(kind, seed + 10, moduli[:Ld] * 2, n), n)            # [2][Ld][N]
            key = anchor_fill("random", seed + 60, [moduli[i] for _ in range(Ld) for _ in range(2) for i in range(L)], n)
            t = key_sums(ct[Ld:2 * Ld], key, Ld)
            res = []
            for comp in range(2):
                cols = [[v % moduli[i] for v in t[comp][i]] for i in range(L)]
                y = [(2 * int(crt(moduli, [c[k] for c in cols], check=False)[0]) + P) // (2 * P) for k in range(n)]   # round(T / P), P odd
                for i in range(Ld):
                    res.append([(y[k] + (ct[i][k] if comp == 0 else 0)) % moduli[i] for k in range(n)])
            recs.append(record([w for pl in res for w in pl], n, op="switch_key_hybrid", input=kind, seed=seed + 10, key_seed=seed + 60))
        out["keyswitch"] = {"log2n": 12, "moduli": moduli, "psi": psis, "cases": recs}
    return out


if __name__ == "__main__":
    data = {
        "small_ntt": small_ntt_vectors(),
        "config1_ct_mul": config1_ct_mul(),
        "rns_ct_mul_small": rns_ct_mul_small(),
        "identities": identities(),
        "rns_ct_mul_n256": rns_ct_mul_n256(),
        "n4096_ntt_digest": n4096_ntt_digest(),
        "sympy_restatement": sympy_restatement(),
        "sympy_anchor": sympy_anchor(),
    }
    for k, v in data.items():
        with open(os.path.join(HERE, k + ".json"), "w") as f:
            json.dump(v, f, separators=(",", ":"))
        print(k, os.path.getsize(os.path.join(HERE, k + ".json")), "bytes")
