"""Shared by the tests of the hoisted slot sums' lane (csrc/rotate_sum.h QpSumLane, dpfhe_rotate_sum_hoisted): the planted term columns, the Python-integer
reference, and the Dot30 columns restated in Python integers.

A COLUMN is one word pair (halves h = 0, 1) of one limb of one tile: for each of the R J terms u = (r, j) the gathered words x[u][row][h] of the live rows
and, for a digit term, the key words keys[u] = (e0.a, e0.b, e1.a, e1.b); the last term of each rotation is the P c0 term on a data limb (has_p).  It must give
    c0[row][h] = sum_u x[u][row][h] * (keys[u][h] | P)      c1[row][h] = sum_{digit u} x[u][row][h] * keys[u][2 + h]      mod q.
The planted columns put the operands on 0, 1 and q - 1 and on the words whose 30-bit halves are largest (q - 1: high half 2^30 - 1; 2^60 - 2^30 - 1: low half
2^30 - 1 - the pair that maximises the lazy form's columns, where such a word is below q)."""
ROTATIONS = (1, 2, 9, 64)
TERMS_PER_ROTATION = (1, 2, 4, 8, 9, 15, 41)      # J: below, at and one past the fold period of 8; 14+ and 40 digits
KINDS = ("zero", "one", "qm1", "lowmax", "random")
PERIOD = 8                                        # modarith.h FoldArith::kDot30Period (the emulator test holds the header to it)
MASK30 = (1 << 30) - 1


def lowmax(q):
    """the largest canonical word whose LOW 30-bit half is 2^30 - 1 (primes above 2^60 - 2^30: every fold prime), else q - 1"""
    w = (1 << 60) - (1 << 30) - 1
    return w if w < q else q - 1


def word(q, kind, rng):
    return int(rng.integers(0, q)) if kind == "random" else {"zero": 0, "one": 1, "qm1": q - 1, "lowmax": lowmax(q)}[kind]


def column(q, n_rot, J, rows, rng, first=0):
    """(x [R J][rows][2], keys [R J][4]) Python integers in [0, q): the kind of a gathered word moves by 1 per term, 2 per row and 1 per half, a key word's by
    3 per term and 1 per word - within five terms every kind of one meets every kind of the other"""
    total = n_rot * J
    x = [[[word(q, KINDS[(first + u + 2 * i + h) % 5], rng) for h in range(2)] for i in range(rows)] for u in range(total)]
    keys = [[word(q, KINDS[(first + 3 * u + c) % 5], rng) for c in range(4)] for u in range(total)]
    return x, keys


def saturated_column(q, n_rot, J, rows, x_pattern, key_pattern):
    """every gathered word and every key word on q - 1 or lowmax: pattern 0 / 1 = all q - 1 / all lowmax, 2 / 3 = alternating by term, starting on either"""
    big = (q - 1, lowmax(q))
    pick = lambda pattern, u: big[pattern] if pattern < 2 else big[(u + pattern) & 1]
    total = n_rot * J
    return [[[pick(x_pattern, u)] * 2 for _ in range(rows)] for u in range(total)], [[pick(key_pattern, u)] * 4 for u in range(total)]


def want(q, p_special, J, has_p, x, keys):
    """[rows][4] = (c0 half 0, c0 half 1, c1 half 0, c1 half 1) in Python integers"""
    Ld = J - 1 if has_p else J
    rows = len(x[0])
    out = [[0, 0, 0, 0] for _ in range(rows)]
    for u, (xu, ku) in enumerate(zip(x, keys)):
        digit = u % J < Ld
        for i in range(rows):
            for h in range(2):
                out[i][h] += xu[i][h] * (ku[h] if digit else p_special)
                if digit:
                    out[i][2 + h] += xu[i][h] * ku[2 + h]
    return [[v % q for v in row] for row in out]


def dot30_columns(pairs, wrap=True):
    """the three Dot30 columns of sum a b over `pairs`, each factor split at bit 30: (S0, S1, S2), every column modulo 2^64 when `wrap` - what 64-bit
    multiply-add chains hold - so that S0 + S1 2^30 + S2 2^60 is the sum exactly when no column wrapped"""
    s0 = s1 = s2 = 0
    for a, b in pairs:
        a0, a1, b0, b1 = a & MASK30, a >> 30, b & MASK30, b >> 30
        s0, s1, s2 = s0 + a0 * b0, s1 + a0 * b1 + a1 * b0, s2 + a1 * b1
    if wrap:
        s0, s1, s2 = s0 % (1 << 64), s1 % (1 << 64), s2 % (1 << 64)
    return s0, s1, s2


def lazy_sum(q, pairs, period):
    """sum a b mod q as a schedule that folds its wrapping Dot30 columns every `period` terms computes it"""
    r = 0
    for k in range(0, len(pairs), period):
        s0, s1, s2 = dot30_columns(pairs[k:k + period])
        r = (r + s0 + (s1 << 30) + (s2 << 60)) % q
    return r
