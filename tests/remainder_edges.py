"""Inputs whose modular PRODUCTS land on the edges of the remainder range (helper, no tests).

Every arithmetic class decides the last step of a modular product by looking at the remainder: a conditional subtract after a floor quotient, a sign fix
after a nearest-integer quotient, a rounding tie.  A missing or inverted correction shows only when the exact product is a multiple of q plus or minus a
word or two, or within a word or two of q / 2.  For an odd prime q with h = (q - 1) / 2 the target set is

    T(q) = {0, 1, 2, q - 2, q - 1, h - 1, h, h + 1, h + 2}

and the builders here choose operands so that the products a kernel takes - and the sums it adds them into - have their remainder in T: the second
operand is solved from the first through word-wise inverses.  Everything is done with the C oracle's word-wise operations on whole numpy arrays
(dyadic, ntt_fwd, ntt_inv, root_powers, class_edges.inverse_words).  Every builder returns (inputs, n_untargeted): the number of words whose given
operand was 0 while the target was not, so that no solution exists and the word keeps its free value.

The transform builders model a transform as the textbook radix-2 stages oracle/pyoracle.py ntt_forward / ntt_inverse walk (Cooley-Tukey forward,
Gentleman-Sande inverse, N^-1 folded into the last inverse stage): item s puts every butterfly of stage s on an edge.  The kernels run the same butterflies
in another order and on lazy representatives, so the residue CLASSES their products take are these."""
import numpy as np

from class_edges import inverse_words

N_TARGETS = 9
U1 = np.uint64(1)


def target_set(q):
    """T(q), in the order the emulator's note hook numbers it (modarith.h DPFHE_EMU_NOTE)"""
    h = (q - 1) // 2
    return (0, 1, 2, q - 2, q - 1, h - 1, h, h + 1, h + 2)


def _limb_table(orc, values):
    return np.array([values(q) for q in orc.moduli], np.uint64)


def _cycle(orc, table, lead, phase, step_limb, step_item, drift=0):
    """[*lead][L][N]: table[l][(k + step_limb l + step_item item + phase) mod period] along the coefficient index k; drift: the phase moves by that much
    more after every full period, so that two cycles of one period meet in every combination"""
    items = int(np.prod(lead, dtype=np.int64))
    period = table.shape[1]
    k = np.arange(orc.n)
    idx = ((k + drift * (k // period))[None, None, :] + step_limb * np.arange(orc.L)[None, :, None] + step_item * np.arange(items)[:, None, None] + phase) % period
    return np.ascontiguousarray(table[np.arange(orc.L)[None, :, None], idx].reshape(tuple(lead) + (orc.L, orc.n)))


def targets(orc, lead, phase, drift=0):
    """[*lead][L][N] words of T(q_l), cycling along the coefficient index, the phase moved by 2 per limb and by 5 per item (both coprime to 9)"""
    return _cycle(orc, _limb_table(orc, target_set), lead, phase, 2, 5, drift)


def free_operands(orc, lead, seed):
    """[*lead][L][N] non-zero words: 1, 2, q - 1, q - 2, h, h + 1 and two random words, a cycle of 8 (coprime to the targets' 9: within 72 coefficients
    every operand extreme meets every remainder extreme)"""
    items = int(np.prod(lead, dtype=np.int64))
    fixed = _cycle(orc, _limb_table(orc, lambda q: (1, 2, q - 1, q - 2, (q - 1) // 2, (q + 1) // 2, 0, 0)), lead, seed, 3, 1)
    rnd = orc.fill(items, seed).reshape(fixed.shape)
    return np.where(fixed == 0, np.where(rnd == 0, U1, rnd), fixed)


def constant(orc, lead, value):
    """[*lead][L][N] with value(q_l) mod q_l in every word of limb l"""
    col = np.array([value(q) % q for q in orc.moduli], np.uint64)[:, None]
    return np.ascontiguousarray(np.broadcast_to(col, tuple(lead) + (orc.L, orc.n)))


def _flat(orc, a):
    return np.ascontiguousarray(a).reshape(-1, orc.L, orc.n)


def mul(orc, a, b):
    return orc.dyadic("mul", _flat(orc, a), _flat(orc, b), threads=0).reshape(a.shape)


def add(orc, a, b):
    return orc.dyadic("add", _flat(orc, a), _flat(orc, b), threads=0).reshape(a.shape)


def sub(orc, a, b):
    return orc.dyadic("sub", _flat(orc, a), _flat(orc, b), threads=0).reshape(a.shape)


def solve(orc, y, tgt, fallback=None, seed=0):
    """z with y z = tgt (mod q_l), word by word.  Where y = 0 the word is `fallback`'s (random words of `seed` by default); it counts as untargeted
    unless the target is 0 as well (then every z solves it).  -> (z, n_untargeted)"""
    y, tgt = np.ascontiguousarray(y), np.ascontiguousarray(tgt)
    assert y.shape == tgt.shape and y.shape[-2:] == (orc.L, orc.n)
    zero = y == 0
    z = mul(orc, tgt, inverse_words(orc, _flat(orc, np.where(zero, U1, y))).reshape(y.shape))
    if zero.any():
        if fallback is None:
            fallback = orc.fill(y.size // (orc.L * orc.n), seed).reshape(y.shape)
        z = np.where(zero, fallback, z)
    return np.ascontiguousarray(z), int((zero & (tgt != 0)).sum())


# ---- the dyadic family ---------------------------------------------------------------------------------------------------------------------------------------
def dyadic_inputs(orc, lead, seed):
    """a, b, acc [*lead][L][N] with a b = R1 in T and acc + a b = R2 in T (acc = R2 - R1) -> ((a, b, acc), 0)"""
    a = free_operands(orc, lead, seed)
    r1, r2 = targets(orc, lead, seed), targets(orc, lead, 4 * seed + 1)
    b, miss = solve(orc, a, r1)
    return (a, b, sub(orc, r2, r1)), miss


def plain_product_inputs(orc, batch, seed):
    """ct [batch][2][L][N], pt [L][N] with every ct word times its pt word in T (multiply_plain: one plaintext for every item and component)"""
    pt = free_operands(orc, (1,), seed)
    ct, miss = solve(orc, np.broadcast_to(pt[0], (batch, 2, orc.L, orc.n)), targets(orc, (batch, 2), seed))
    return (ct, pt[0]), miss


def _step_inside(orc, t):
    """t in T -> a neighbour of t that is in T as well: t + 1, or t - 1 at the upper ends 2 and h + 2 of the two runs"""
    top = (t == constant(orc, t.shape[:-2], lambda q: 2)) | (t == constant(orc, t.shape[:-2], lambda q: (q - 1) // 2 + 2))
    one = constant(orc, t.shape[:-2], lambda q: 1)
    return np.where(top, sub(orc, t, one), add(orc, t, one))


def _row_targets(orc, rows, cols, phase, forced_zero=None, nonzero_last=False):
    """[rows][cols][L][N]: the targets of the terms of each row, the last column's replaced by (a target for the row's TOTAL) - (the other terms).
    forced_zero [cols][L][N]: words whose term is 0 whatever the solved operand (the given operand is 0): their target is 0 (with one column that is the
    total's).  nonzero_last: the total's target steps to a neighbour in T where the last column's term would be 0, so that this term can serve as a divisor"""
    t = targets(orc, (rows, cols), phase)
    if forced_zero is not None:
        t[:, : cols - 1] = np.where(forced_zero[None, : cols - 1], np.uint64(0), t[:, : cols - 1])
    total = targets(orc, (rows,), phase + 7, drift=1)
    if forced_zero is not None and cols == 1:
        total = np.where(forced_zero[None, 0], np.uint64(0), total)
    rest = constant(orc, (rows,), lambda q: 0)
    for j in range(cols - 1):
        rest = add(orc, rest, t[:, j])
    if nonzero_last:
        total = np.where(total == rest, _step_inside(orc, total), total)
    t[:, cols - 1] = sub(orc, total, rest)
    return t


def matvec_plain_inputs(orc, rows, cols, comps, seed):
    """W [rows][cols][L][N], x [cols][comps][L][N] for y[i][c] = sum_j W[i][j] x[j][c].  A matrix word meets `comps` vector words, so not every term can be
    chosen.  Row 0 of W is free (non-zero) and EVERY component of x is solved against it: each term but the last column's in T, the last column solved so
    that the total is in T.  The other rows are solved against component 0 in the same way; where that vector word is 0 (its target was) the term is 0,
    which is in T, and the last of several columns' word never is 0.  So every row's total is in T under component 0, row 0's under every component."""
    L, n = orc.L, orc.n
    W0 = free_operands(orc, (cols,), seed)
    t = np.stack([_row_targets(orc, 1, cols, seed + 3 * c, nonzero_last=(c == 0 and cols > 1))[0] for c in range(comps)], axis=1)
    x, miss = solve(orc, np.broadcast_to(W0[:, None], (cols, comps, L, n)), t)
    W = np.empty((rows, cols, L, n), np.uint64)
    W[0] = W0
    if rows > 1:
        x0 = np.ascontiguousarray(x[:, 0])
        W[1:], m = solve(orc, np.broadcast_to(x0[None], (rows - 1, cols, L, n)), _row_targets(orc, rows - 1, cols, seed + 1, forced_zero=(x0 == 0)),
                         fallback=free_operands(orc, (rows - 1, cols), seed + 2))
        miss += m
    return (W, x), miss


def matvec_scalar_inputs(orc, rows, cols, comps, seed):
    """w [rows][cols][L] (one scalar per limb), x [cols][comps][L][N] for y[i][c] = sum_j w[i][j] x[j][c]: every vector word is solved against row 0's
    scalar (terms in T, the last column making row 0's total a target); the other rows run the operand extremes against the same words"""
    w = np.ascontiguousarray(free_operands(orc, (rows, cols), seed)[..., 0])
    w0 = np.ascontiguousarray(np.broadcast_to(w[0][:, None, :, None], (cols, comps, orc.L, orc.n)))
    t = np.stack([_row_targets(orc, 1, cols, seed + 3 * c)[0] for c in range(comps)], axis=1)
    x, miss = solve(orc, w0, t)
    return (w, x), miss


# ---- the tensor product ----------------------------------------------------------------------------------------------------------------------------------------
def fold_scaled_factors(moduli):
    """per limb the factor s = 2^(60-k) a fold_scaled limb (q = 2^k - d0) carries its words by, 1 for every other class: the lazy products of the fused
    multiply hold s a b modulo q there (modarith.h FoldScaledArith), so it is s a b that has to land on the edges"""
    from class_edges import expected_class
    return [1 << (60 - q.bit_length()) if expected_class(q) == "fold_scaled" else 1 for q in moduli]


def unscale(orc, a, factors):
    """a with every word of limb l multiplied by factors[l]^-1"""
    if factors is None:
        return a
    inv = [pow(f, -1, q) for f, q in zip(factors, orc.moduli)]
    return mul(orc, a, constant(orc, a.shape[:-2], lambda q: inv[orc.moduli.index(q)]))


def tensor_inputs(orc, batch, seed, factors=None):
    """(a, b) coefficient domain and (A, B) NTT domain, each [batch][2][L][N], for (c0, c1, c2) = (A0 B0, A0 B1 + A1 B0, A1 B1).

    A0 B0 A1 B1 = A0 B1 A1 B0, so three of the four products can be chosen per word.  Always A0 B1 = R1 and A1 B0 = R2 - R1 (c1 = R2 in T, both of its
    products on an edge when R2 - R1 is).  Even coefficients: A0 B0 in T as well (A0 free; where that target is 0, B0 = 0 and R2 = R1 there).  Odd
    coefficients: A1 B1 in T instead (A1 free).  factors (fold_scaled_factors): s (product) is put on the edges instead, limb by limb.
    -> (((a, b), (A, B)), n_untargeted)"""
    L, n = orc.L, orc.n
    lead = (batch,)
    free = free_operands(orc, lead, seed)
    pa, r1, r2 = (unscale(orc, t, factors) for t in (targets(orc, lead, seed), targets(orc, lead, seed + 3, drift=1), targets(orc, lead, 2 * seed + 5, drift=2)))
    odd = (np.arange(n) & 1).astype(bool)
    # the chosen square product P = X Y with X free; then X Y' = R1 and X' Y = R2 - R1 for the other pair (X', Y')
    r2 = np.where(pa == 0, r1, r2)
    Y, m0 = solve(orc, free, pa)
    Yo, m1 = solve(orc, free, r1)
    Xo, m2 = solve(orc, Y, sub(orc, r2, r1), fallback=free_operands(orc, lead, seed + 11))
    # even: X = A0, Y = B0, Y' = B1, X' = A1.   odd: X = A1, Y = B1, and A1 B0 = R1', A0 B1 = R2 - R1' - the same shape with the roles swapped
    A = np.stack([np.where(odd, Xo, free), np.where(odd, free, Xo)], axis=1)
    B = np.stack([np.where(odd, Yo, Y), np.where(odd, Y, Yo)], axis=1)
    inv = lambda v: orc.ntt_inv(v.reshape(-1, L, n), threads=0).reshape(v.shape)
    A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
    return ((inv(A), inv(B)), (A, B)), m0 + m1 + m2


def _sqrt_mod(a, q):
    """a square root of a modulo the prime q, or None (Tonelli-Shanks on Python integers: one call per limb and target)"""
    a %= q
    if a == 0:
        return 0
    if pow(a, (q - 1) // 2, q) != 1:
        return None
    s, e = q - 1, 0
    while s % 2 == 0:
        s, e = s // 2, e + 1
    z = next(v for v in range(2, q) if pow(v, (q - 1) // 2, q) == q - 1)
    c, x, t = pow(z, s, q), pow(a, (s + 1) // 2, q), pow(a, s, q)
    while t != 1:
        i, u = 0, t
        while u != 1:
            u, i = u * u % q, i + 1
        b = pow(c, 1 << (e - i - 1), q)
        x, c, e = x * b % q, b * b % q, i
        t = t * c % q
    return x


def square_roots(q):
    """the square roots of the elements of T(q) that have one, both signs: the values A0 may take with A0^2 in T"""
    roots = [r for r in (_sqrt_mod(t, q) for t in target_set(q)) if r is not None]
    return sorted({r for r in roots} | {(q - r) % q for r in roots})


def squaring_inputs(orc, batch, seed):
    """(a, A) [batch][2][L][N] for a ciphertext multiplied by itself: A0 cycles through the square roots of the targets that are squares modulo q_l
    (0, 1, q - 1 always are; q = 1 mod 8 makes 2, q - 2, h and h + 1 squares too), so A0^2 in T, and A0 A1 in T (c1 = 2 A0 A1).  Where A0 = 0 that product is 0 and A1 is free."""
    L, n = orc.L, orc.n
    roots = [square_roots(q) for q in orc.moduli]
    period = min(len(r) for r in roots)
    a0 = _cycle(orc, np.array([r[:period] for r in roots], np.uint64), (batch,), seed, 1, 1)
    a1, miss = solve(orc, a0, np.where(a0 == 0, np.uint64(0), targets(orc, (batch,), seed + 2, drift=1)), fallback=free_operands(orc, (batch,), seed + 1))
    A = np.ascontiguousarray(np.stack([a0, a1], axis=1))
    return (orc.ntt_inv(A.reshape(-1, L, n), threads=0).reshape(A.shape), A), miss


# ---- the transforms, stage by stage ----------------------------------------------------------------------------------------------------------------------------
class Stages:
    """Radix-2 stages on whole [items][L][N] arrays.  Stage s (0 .. log2 N - 1) has m = 2^s groups of 2 t words, t = N / 2m: word j of the first half of
    group i (the `u` leg) meets word j + t (the `v` leg) under the twiddle table[m + i] of the bit-reversed root table ntt_forward walks.  The inverse
    transform's stage k has the layout of s = log2 N - 1 - k with the inverse table."""

    def __init__(self, orc):
        self.orc, self.log = orc, orc.log2_n
        tabs = [orc.root_powers(l) for l in range(orc.L)]
        self.rp, self.irp = np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs])
        self.half = constant(orc, (1,), lambda q: (q + 1) // 2)          # 2^-1
        self.n_words = constant(orc, (1,), lambda q: orc.n)              # N

    def v_leg(self, s):
        return ((np.arange(self.orc.n) >> (self.log - 1 - s)) & 1).astype(bool)

    def partner(self, a, s):
        t = self.orc.n >> (s + 1)
        return a.reshape(a.shape[:-1] + (-1, 2, t))[..., ::-1, :].reshape(a.shape)

    def twiddles(self, s, inverse):
        """[1][L][N]: the stage's twiddle on every v leg, 1 on every u leg"""
        m, t = 1 << s, self.orc.n >> (s + 1)
        out = np.ones((1, self.orc.L, m, 2, t), np.uint64)
        out[0, :, :, 1, :] = (self.irp if inverse else self.rp)[:, m:2 * m, None]
        return out.reshape(1, self.orc.L, self.orc.n)

    def _times(self, a, c):
        return mul(self.orc, a, np.ascontiguousarray(np.broadcast_to(c, a.shape)))

    def cooley_tukey(self, a, s):
        """(u, v) -> (u + v w, u - v w)"""
        p = self._times(a, self.twiddles(s, False))
        ps = np.ascontiguousarray(self.partner(p, s))
        return np.where(self.v_leg(s), sub(self.orc, ps, p), add(self.orc, p, ps))

    def gentleman_sande(self, a, s):
        """(u, v) -> (u + v, (u - v) w^-1)"""
        ap = np.ascontiguousarray(self.partner(a, s))
        return np.where(self.v_leg(s), self._times(sub(self.orc, ap, a), self.twiddles(s, True)), add(self.orc, a, ap))

    def halve(self, a):
        return self._times(a, self.half)

    # cooley_tukey(s) then gentleman_sande(s), or the other way round, doubles every word: each undoes the other up to the halving


def forward_stage_inputs(orc, seed):
    """[log2 N][L][N]: item s is the input under which, at EVERY butterfly of forward stage s, v w = R in T and u + v w = R' in T (v = R w^-1,
    u = R' - R); the stages before s are undone with inverse butterflies.  Twiddles are units: nothing is untargeted."""
    st = Stages(orc)
    out = []
    for s in range(st.log):
        r, r2 = targets(orc, (1,), seed + s), targets(orc, (1,), 2 * seed + s + 4)
        e = np.where(st.v_leg(s), st._times(r, st.twiddles(s, True)), sub(orc, r2, np.ascontiguousarray(st.partner(r, s))))
        for j in range(s - 1, -1, -1):
            e = st.halve(st.gentleman_sande(np.ascontiguousarray(e), j))
        out.append(e[0])
    return np.ascontiguousarray(np.stack(out)), 0


def inverse_stage_inputs(orc, seed):
    """[log2 N][L][N]: item k is the input under which, at every butterfly of Gentleman-Sande stage k, (u - v) w = R in T and u + v = R' in T; at the
    last stage, which carries N^-1, (u + v) N^-1 = R' and (u - v) w N^-1 = R.  The stages before k are undone with forward butterflies."""
    st = Stages(orc)
    out = []
    for k in range(st.log):
        s = st.log - 1 - k
        r, r2 = targets(orc, (1,), seed + k), targets(orc, (1,), 2 * seed + k + 4)
        e = np.where(st.v_leg(s), r, r2)            # the stage's OUTPUT: the sums on the u legs, the twiddled differences on the v legs
        if k == st.log - 1:
            e = st._times(e, st.n_words)
        e = st.halve(st.cooley_tukey(np.ascontiguousarray(e), s))
        for kk in range(k - 1, -1, -1):
            e = st.halve(st.cooley_tukey(np.ascontiguousarray(e), st.log - 1 - kk))
        out.append(e[0])
    return np.ascontiguousarray(np.stack(out)), 0


# ---- key material -------------------------------------------------------------------------------------------------------------------------------------------------
def digit_transforms(orc, digits, galois_elt=None):
    """digits [nd][N] (limb j of an item's last component, words below q_j) -> x [nd][L][N], x[j][i] = NTT_i(digits[j] mod q_i): what a key-switching kernel
    multiplies with key word [j][comp][i].  galois_elt: the hoisted rotations' order - lifted first, then sigma_g modulo q_i (oracle.c orc_rotate_hoisted)."""
    qcol = np.array(orc.moduli, np.uint64)[:, None]
    lifted = np.ascontiguousarray(digits[:, None, :] % qcol[None])
    if galois_elt is not None:
        lifted = orc.apply_galois(lifted, galois_elt)
    return orc.ntt_fwd(lifted, threads=0)


def key_for_targets(orc, x, tgt, fallback):
    """key [nd][2][L][N] with x[j] key[j][c] = tgt[j][c] word by word; where x = 0 the word is fallback's -> (key, zero [nd][L][N])"""
    zero = x == 0
    inv = inverse_words(orc, np.where(zero, U1, x))
    key = np.stack([np.where(zero, fallback[:, c], mul(orc, np.ascontiguousarray(tgt[:, c]), inv)) for c in range(2)], axis=1)
    return np.ascontiguousarray(key), zero


def targeted_key(orc, x, seed, per_limb=False):
    """A key under which every product x[j] key[j][c] of the transformed digits x [nd][L][N] is in T, and so is their SUM over the digits: the last
    digit's targets are (a target for the sum) - (the other digits' targets); with one digit the product is the sum.  Where a digit's transform holds a 0
    no key word reaches a non-zero target: those (digit, component, word) places are counted.  -> (key [nd][2][L][N], n_untargeted)"""
    nd = x.shape[0]
    tgt = np.ascontiguousarray(targets(orc, (nd, 2), seed))
    total = targets(orc, (2,), seed + 4)
    for j in range(nd - 1):
        total = sub(orc, total, np.ascontiguousarray(tgt[j]))
    tgt[nd - 1] = total
    key, zero = key_for_targets(orc, x, tgt, orc.fill(nd * 2, seed).reshape(nd, 2, orc.L, orc.n))
    miss = zero[:, None] & (tgt != 0)
    return key, (miss.sum(axis=(0, 1, 3)) if per_limb else int(miss.sum()))


def rotation_elements(n):
    return (3, pow(3, 9, 2 * n), 2 * n - 1)


def relin_inputs(orc, batch, seed, per_limb=False):
    """c3 [batch][3][L][N] and an RNS-digit key [L][2][L][N] targeted at item 0's digits (limb j of its last component) -> ((c3, evk), n_untargeted);
    the same key and c3[:, 1:] serve switch_key"""
    c3 = orc.fill(batch * 3, seed).reshape(batch, 3, orc.L, orc.n)
    evk, miss = targeted_key(orc, digit_transforms(orc, c3[0, 2]), seed + 1, per_limb)
    return (c3, evk), miss


def hybrid_inputs(orc, data, batch, seed, per_limb=False):
    """orc: the extended context (last limb = the special prime), data: its first L - 1 limbs.  {comps: ct [batch][comps][L-1][N]} for 2 and 3 components,
    item 0's last component the same digits in both, and the key [L-1][2][L][N] targeted at them -> ((cts, key), n_untargeted)"""
    Ld, n = data.L, data.n
    digits = data.fill(1, seed)[0]
    key, miss = targeted_key(orc, digit_transforms(orc, digits), seed + 1, per_limb)
    cts = {}
    for comps in (2, 3):
        cts[comps] = data.fill(batch * comps, seed + comps).reshape(batch, comps, Ld, n)
        cts[comps][0, comps - 1] = digits
    return (cts, key), miss


def hoisted_inputs(orc, data, elts, tokens, seed, per_limb=False):
    """cts [tokens][2][L-1][N] and one key per Galois element [k][L-1][2][L][N], each targeted at token 0's digits as the hoisted rotation multiplies
    them: lifted, then rotated (digit_transforms with galois_elt) -> ((cts, keys), n_untargeted)"""
    cts = data.fill(tokens * 2, seed).reshape(tokens, 2, data.L, data.n)
    made = [targeted_key(orc, digit_transforms(orc, cts[0, 1], g), seed + 1 + i, per_limb) for i, g in enumerate(elts)]
    return (cts, np.ascontiguousarray(np.stack([k for k, _ in made]))), sum(m for _, m in made)


# ---- rescale --------------------------------------------------------------------------------------------------------------------------------------------------------
def rescale_inputs(orc, lead, seed):
    """x [*lead][L][N] with x_i = R q_last + x_last (mod q_i) on the limbs below the last: (x_i - x_last) q_last^-1 = R in T.  The rounding adds
    floor(q_last / 2) to both sides first; x_last runs through the operand extremes, h and h + 1 - the two sides of that rounding's wrap - among them."""
    ql = orc.moduli[-1]
    x_last = free_operands(orc, lead, seed)[..., -1:, :]
    qcol = np.array(orc.moduli, np.uint64)[:, None]
    acc = np.ascontiguousarray(np.broadcast_to(x_last, tuple(lead) + (orc.L, orc.n)) % qcol)
    x = orc.dyadic("mul_add", _flat(orc, targets(orc, lead, seed)), _flat(orc, constant(orc, lead, lambda q: ql)), acc=_flat(orc, acc), threads=0).reshape(acc.shape)
    x[..., -1, :] = x_last[..., 0, :]
    return np.ascontiguousarray(x), 0
