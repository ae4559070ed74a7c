"""The last pass of a rotate-and-add step (include/dpfhe.h dpfhe_rotate_add_hybrid, dpfhe_rotate_add_pass_host; csrc/rotate_add.h) stated with Python
integers, the host twin's ctypes call, and the inputs the CPU and GPU tests share.  A plain helper like tests/fused_rescale_ref.py (no conftest, no plugin).

  out.c0 = round(work.c0 / P) + c0 + sigma_g(c0),   out.c1 = round(work.c1 / P) + c1      on every data limb

round(X / P) goes through the CRT integer of the coefficient (fused_rescale_ref.divide_by_p); sigma_g is the ring automorphism a(X) -> a(X^g) mod X^N + 1
written as a scatter of monomials (coefficient i goes to i g mod 2N, negated past N) - not the gather by g^-1 the library uses."""
import ctypes as C
import itertools

import numpy as np

import fused_rescale_ref as fr
from deeppowers_amd import _cabi

WORDS = ("0", "1", "q-1")     # what round(work / P) mod q_i, c0[k] and the gathered word are planted on


def elements(n):
    """the elements the tests run: the first rotation, a far one, the row swap (every position but 0 negated) and its neighbour"""
    return (3, pow(3, n // 4, 2 * n), 2 * n - 1, 2 * n - 3)


def automorphism(a, g, q):
    """a [N] residues mod q -> a(X^g) mod (X^N + 1, q)"""
    n = len(a)
    out = [0] * n
    for i, v in enumerate(a):
        j = i * g % (2 * n)
        if j < n:
            out[j] = (out[j] + int(v)) % q
        else:
            out[j - n] = (out[j - n] - int(v)) % q
    return np.array(out, dtype=np.uint64)


def pass_reference(moduli, work, in2, g):
    """moduli: the L = Ld + 1 limbs of the extended basis.  work [batch][2][L][N], in2 [batch][2][Ld][N] -> [batch][2][Ld][N]"""
    data = moduli[:-1]
    out = np.empty_like(in2)
    for b in range(work.shape[0]):
        for c in range(2):
            r = fr.divide_by_p(moduli, work[b, c])
            for l, q in enumerate(data):
                rot = automorphism(in2[b, 0, l], g, q) if c == 0 else np.zeros(in2.shape[-1], np.uint64)
                out[b, c, l] = np.array([(int(v) + int(a) + int(s)) % q for v, a, s in zip(r, in2[b, c, l], rot)], dtype=np.uint64)
    return out


def pass_twin(p, work, in2, g):
    work = np.ascontiguousarray(work, dtype=np.uint64)
    in2 = np.ascontiguousarray(in2, dtype=np.uint64)
    out = np.full(in2.shape, 0xDEADBEEFCAFEF00D, dtype=np.uint64)
    m = (C.c_uint64 * p.n_limbs)(*p.moduli)
    _cabi.check(_cabi.load().dpfhe_rotate_add_pass_host(m, p.n_limbs, p.log2_n, out.ctypes.data, work.ctypes.data, in2.ctypes.data, g, work.shape[0]),
                "dpfhe_rotate_add_pass_host")
    return out


def word(name, q):
    return {"0": 0, "1": 1, "q-1": q - 1}[name]


def gather_source(k, g, n):
    """(index, negated) of the word sigma_g(a)[k] is made of"""
    j = k * pow(g, -1, 2 * n) % (2 * n)
    return j % n, j >= n


def plan_positions(g, n):
    """[(k, rescaled, direct, gathered, negated)]: one coefficient k per combination of the three planted words and of the gather's sign, chosen so that no
    two combinations ask different words of one coefficient of c0.  An element may not offer every combination (2N - 1 negates everywhere but at 0): what
    fits is returned, the tests say what they expect."""
    taken, used, plan = {}, set(), []
    for negated in (False, True):
        for r, d, s in itertools.product(WORDS, repeat=3):
            for k in range(n):
                src, neg = gather_source(k, g, n)
                if k in used or neg != negated or taken.get(k, d) != d or taken.get(src, s) != s or (src == k and d != s):
                    continue
                used.add(k)
                taken[k], taken[src] = d, s
                plan.append((k, r, d, s, negated))
                break
    return plan


def pass_inputs(p, batch, seed, g, planted=True):
    """(work [batch][2][L][N], in2 [batch][2][Ld][N], plan): random canonical words; with `planted`, item 0 carries plan_positions(g): at coefficient k of
    component 0, on EVERY data limb i, round(work / P) mod q_i, c0[k] and the word the gather reads are the planned ones of {0, 1, q_i - 1}, and the special-limb
    residue of `work` there cycles through fused_rescale_ref.P_EDGES (entry j of the plan takes edge j % 6); component 1 gets the same rescaled words against
    c1[k] = the plan's direct word."""
    rng = np.random.default_rng(seed)
    L, Ld, n = p.n_limbs, p.n_limbs - 1, p.n
    P = p.moduli[-1]
    Q = 1
    for q in p.moduli[:Ld]:
        Q *= q
    work = fr.random_words(rng, p.moduli, (batch, 2), n)
    in2 = fr.random_words(rng, p.moduli[:Ld], (batch, 2), n)
    plan = plan_positions(g, n) if planted else []
    for j, (k, r, d, s, _) in enumerate(plan):
        delta = fr.edge_value(fr.P_EDGES[j % 6], P, 3)
        R = {"0": 0, "1": 1, "q-1": Q - 1}[r] - (1 if delta > P // 2 else 0)    # round((R P + delta) / P) = R + [delta > P / 2]
        X = (R * P + delta) % (Q * P)
        src, _ = gather_source(k, g, n)
        for l, q in enumerate(p.moduli):
            work[0, :, l, k] = X % q
        for l, q in enumerate(p.moduli[:Ld]):
            in2[0, 0, l, src] = word(s, q)
        for l, q in enumerate(p.moduli[:Ld]):      # (after the sources: src == k only where both words agree)
            in2[0, :, l, k] = word(d, q)
    return work, in2, plan


def reached(p, work, in2, g, plan):
    """what the integers make of the planted coefficients of item 0, component 0: {(rescaled, direct, gathered, negated, special-limb edge)} by name, with a word
    named only when it is the SAME named word on every data limb"""
    Ld, n = p.n_limbs - 1, p.n
    P = p.moduli[-1]
    r = fr.divide_by_p(p.moduli, work[0, 0])
    edge_names = {fr.edge_value(e, P, 3): e for e in fr.P_EDGES}

    def name(values):
        names = {next((w for w in WORDS if word(w, q) == int(v)), None) for v, q in zip(values, p.moduli[:Ld])}
        return names.pop() if len(names) == 1 else None
    got = set()
    rotated = [automorphism(in2[0, 0, l], g, q) for l, q in enumerate(p.moduli[:Ld])]
    for k, *_ in plan:
        src, neg = gather_source(k, g, n)
        # the automorphism of the reference, not the gather: the word that lands on k is +-c0[src]
        for l, q in enumerate(p.moduli[:Ld]):
            assert int(rotated[l][k]) == ((-int(in2[0, 0, l, src])) % q if neg else int(in2[0, 0, l, src]))
        got.add((name([int(r[k]) % q for q in p.moduli[:Ld]]), name(in2[0, 0, :, k]), name(in2[0, 0, :, src]), neg, edge_names.get(int(work[0, 0, -1, k]))))
    return got
