"""An exact integer model of ApproxPackedLinear on a TRANSPARENT input (include/deeppowers/fhe.hpp).

Feed the layer a ciphertext (c0, 0) whose c0 holds the residues of a known integer polynomial m.  Every key-switch digit is then zero, so every key inner
product is zero and every division by P divides P * (...) exactly: the layer is a deterministic integer function of m, W, b and the scales.  In
Z[X] / (X^N + 1), with sigma_g a(X) = a(X^g):

    S_i  = sum_{j < n1} p[o][i][j] * sigma_{3^j}(m)                     (o: output ciphertext)
    M_o  = sum_{i < n2} sigma_{3^(i n1)}(S_i)
    for s = m, 2m, ... < n:  M_o += sigma_{3^s}(M_o)                    (wide-input fold)
    c0_o = round(M_o / q_last) + bias_o   mod q_l, l < L - 1;   c1_o = 0

p[o][i][j] is the int64 coefficient vector the encoder's host twin (deeppowers_amd.ckks.encode_host, real form) gives for the diagonal's slot vector at
weight_scale; bias_o is the twin's complex-form encoding at output_scale().  Nothing here is taken from the library's packed-layer code: the geometry
below is restated from the slot semantics, and the split n1 x n2 is an input (the words depend on it only through which vectors get encoded).

  Slot semantics.  X -> X^(3^s) rotates the N/2 slots LEFT by s.  The input repeats with period n = the padded in_dim.  Position r' of diagonal
  k = i n1 + j multiplies slot r' of the input rotated by j, i.e. x[(r' + j) mod n], and the giant step moves the product to slot r = r' - i n1: so it
  must hold W[R(r), (r + k) mod n], R(r) the row the OUTPUT holds at slot r, zero where there is no row or the column is >= in_dim.  Summed over the
  m diagonals slot r holds the part of (W x)_R over the columns r .. r + m - 1 (mod n); m = n covers every column, m < n (wide input: m = the padded
  out_dim) needs the n / m windows r, r + m, ... folded together, and R(r + m) = R(r) makes that the full row sum.
  R: the slot row has N/2 / n windows of n slots.  One block of m rows: every window holds it (R = r mod m).  More blocks (then m = n): window c of
  output ciphertext o holds block o * windows + c.

Model A runs this on Python integers (negacyclic products by Kronecker substitution, automorphisms by index); model B runs the same formula limb by limb
on oracle.cbind.Oracle (for N = 32768, where one big-integer product takes seconds).  tests/test_approx_layer_model_cpu.py holds them to each other and
model A to the float64 W x + b; tests/test_gpu_approx_layer_words.py holds the device's words to them.
"""
import math
import struct

import numpy as np

import cpp_build
from deeppowers_amd import ckks
from deeppowers_amd.params import FheParams, ntt_primes

MAGIC = 0x31574C5041      # "APLW1"
NOISE = 21                # |e| of a fresh ciphertext (deeppowers_amd/csrc/fhe_sampler.h)


def pow2_at_least(v):
    x = 2
    while x < v:
        x <<= 1
    return x


class Geometry:
    """n, m, windows, blocks, output ciphertexts, the row of a slot and the slot vectors - from the slot semantics above"""

    def __init__(self, log2n, out_dim, in_dim, n1, n2):
        self.row = (1 << log2n) // 2
        self.out_dim, self.in_dim = out_dim, in_dim
        self.n = pow2_at_least(in_dim)                          # input period
        assert self.n <= self.row
        self.m = min(pow2_at_least(out_dim), self.n)            # diagonals per output ciphertext
        self.windows = self.row // self.n
        self.blocks = -(-out_dim // self.m)
        self.passes = 1 if self.blocks == 1 else -(-self.blocks // self.windows)
        self.folds = []
        s = self.m
        while s < self.n:
            self.folds.append(s)
            s <<= 1
        self.n1, self.n2 = n1, n2
        assert n1 * n2 == self.m, (n1, n2, self.m)

    def row_of_slot(self, o, r):
        block = 0 if self.blocks == 1 else o * self.windows + r // self.n
        R = block * self.m + r % self.m
        return R if R < self.out_dim else -1

    def rows(self):
        """[passes][N/2]: the row every slot holds, -1 for none"""
        return np.array([[self.row_of_slot(o, r) for r in range(self.row)] for o in range(self.passes)], dtype=np.int64)

    def diagonal_slots(self, W, o, i, j):
        """the pre-rotated diagonal i n1 + j of output ciphertext o: float64 [N/2]"""
        k, out = i * self.n1 + j, np.zeros(self.row)
        for rp in range(self.row):
            r = (rp - i * self.n1) % self.row
            R, col = self.row_of_slot(o, r), (r + k) % self.n
            if R >= 0 and col < self.in_dim:
                out[rp] = W[R, col]
        return out

    def bias_slots(self, b, o, tpc):
        out = np.zeros(self.row, dtype=np.complex128)
        for r in range(self.row):
            R = self.row_of_slot(o, r)
            if R >= 0:
                out[r] = complex(b[R], b[R] if tpc == 2 else 0.0)
        return out

    def pack(self, xa, xb=None):
        out = np.zeros(self.row, dtype=np.complex128)
        for s in range(self.row):
            c = s % self.n
            if c < self.in_dim:
                out[s] = complex(xa[c], xb[c] if xb is not None else 0.0)
        return out


def output_scale(input_scale, weight_scale, q_last):
    return input_scale * weight_scale / float(q_last)


def encoded_layer(log2n, geo, W, b, weight_scale, out_scale, tpc, bias_scale=None):
    """the twin's encodings: p int64 [passes][n2][n1][N], bias int64 [passes][N] or None"""
    N = 1 << log2n
    p = np.empty((geo.passes, geo.n2, geo.n1, N), dtype=np.int64)
    for o in range(geo.passes):
        for i in range(geo.n2):
            slots = np.stack([geo.diagonal_slots(W, o, i, j) for j in range(geo.n1)])
            p[o, i] = ckks.encode_host(slots, weight_scale, log2n)
    bias = None
    if b is not None:
        slots = np.stack([geo.bias_slots(b, o, tpc) for o in range(geo.passes)])
        bias = np.array(ckks.encode_host(slots, out_scale if bias_scale is None else bias_scale, log2n), dtype=np.int64)
    return p, bias


# ---- model A: big integers ---------------------------------------------------------------------------------------------------------------------
def automorphism(a, g):
    """sigma_g on a coefficient list / object array: a_k X^k -> a_k X^(k g), X^N = -1"""
    N = len(a)
    out = np.empty(N, dtype=object)
    for k in range(N):
        e = k * g % (2 * N)
        out[e % N] = a[k] if e < N else -a[k]
    return out


def _pack(values, slot_bits):
    """sum values[k] 2^(slot_bits k) for signed Python / numpy integers below 2^63 in magnitude"""
    v = np.array([int(x) for x in values], dtype=object)
    words = slot_bits // 64

    def side(nonneg):
        a = np.zeros((len(v), words), dtype="<u8")
        a[:, 0] = np.array(nonneg, dtype=np.uint64)
        return int.from_bytes(a.tobytes(), "little")
    return side([x if x > 0 else 0 for x in v]) - side([-x if x < 0 else 0 for x in v])


def _unpack_negacyclic(value, N, slot_bits):
    """the 2N signed digits of `value` in base 2^slot_bits, folded with X^N = -1 -> object array [N]"""
    half = 1 << (slot_bits - 1)
    offset = half * (((1 << (slot_bits * 2 * N)) - 1) // ((1 << slot_bits) - 1))      # `half` in every digit: all digits become non-negative
    raw = (value + offset).to_bytes(slot_bits // 8 * 2 * N + 8, "little")
    words = slot_bits // 64
    d = np.frombuffer(raw, dtype="<u8", count=2 * N * words).reshape(2 * N, words)
    digits = np.zeros(2 * N, dtype=object)
    for w in range(words):
        digits += d[:, w].astype(object) << (64 * w)
    digits -= half
    return digits[:N] - digits[N:]


def centred(residues, moduli):
    """[L][N] canonical residues -> the centred CRT value, object array [N]"""
    Q = math.prod(moduli)
    acc = np.zeros(residues.shape[-1], dtype=object)
    for l, q in enumerate(moduli):
        Ql = Q // q
        acc += residues[l].astype(object) * (Ql * pow(Ql, -1, q))
    acc %= Q
    return np.where(acc > Q // 2, acc - Q, acc)


def residues(a, moduli):
    return np.stack([np.array([int(x) % q for x in a], dtype=np.uint64) for q in moduli])


def model_a(log2n, moduli, geo, p, bias, ms):
    """ms: T integer polynomials (object arrays [N]) -> the layer's output words uint64 [passes * T][2][L - 1][N]"""
    N, L, T = 1 << log2n, len(moduli), len(ms)
    Q, q_last = math.prod(moduli), moduli[-1]
    pmax = max(1, int(np.abs(p).max()))
    mmax = max(1, max(int(abs(v)) for m in ms for v in m))
    slot_bits = -(-(pmax.bit_length() + mmax.bit_length() + log2n + geo.n1.bit_length() + 2) // 64) * 64
    rot = [[_pack(automorphism(m, pow(3, j, 2 * N)), slot_bits) for j in range(geo.n1)] for m in ms]
    out = np.zeros((geo.passes * T, 2, L - 1, N), dtype=np.uint64)
    for o in range(geo.passes):
        M = [np.zeros(N, dtype=object) for _ in range(T)]
        for i in range(geo.n2):
            packed = [_pack(p[o, i, j], slot_bits) for j in range(geo.n1)]
            for t in range(T):
                S = _unpack_negacyclic(sum(packed[j] * rot[t][j] for j in range(geo.n1)), N, slot_bits)
                M[t] = M[t] + automorphism(S, pow(3, i * geo.n1, 2 * N))
        for t in range(T):
            Mo = M[t]
            for s in geo.folds:
                Mo = Mo + automorphism(Mo, pow(3, s, 2 * N))
            Mo = Mo % Q
            Mo = np.where(Mo > Q // 2, Mo - Q, Mo)
            c0 = (2 * Mo + q_last) // (2 * q_last)            # round: q_last is odd, no tie
            if bias is not None:
                c0 = c0 + bias[o].astype(object)
            out[o * T + t, 0] = residues(c0, moduli[:-1])
    return out


# ---- model B: the same formula limb by limb on the oracle -----------------------------------------------------------------------------------------
def model_b(log2n, moduli, psi, geo, p, bias, c0_words):
    """c0_words: uint64 [T][L][N] -> uint64 [passes * T][2][L - 1][N]"""
    from oracle.cbind import Oracle
    N, L, T = 1 << log2n, len(moduli), c0_words.shape[0]
    orc = Oracle(log2n, moduli, psi)
    qcol = np.array(moduli, dtype=np.int64)[:, None]
    qnext = np.array(moduli[:-1], dtype=np.uint64)[:, None]
    lift = lambda a: np.ascontiguousarray(np.mod(a[..., None, :], qcol).astype(np.uint64))      # int64 [..][N] -> residues [..][L][N]
    babies = [orc.ntt_fwd(np.stack([orc.apply_galois(np.ascontiguousarray(c0_words[t][None]), pow(3, j, 2 * N))[0] for j in range(geo.n1)]))
              for t in range(T)]
    out = np.zeros((geo.passes * T, 2, L - 1, N), dtype=np.uint64)
    for o in range(geo.passes):
        diag = [orc.ntt_fwd(lift(p[o, i])) for i in range(geo.n2)]
        for t in range(T):
            M = np.zeros((1, L, N), dtype=np.uint64)
            for i in range(geo.n2):
                prod = orc.dyadic("mul", diag[i], babies[t])
                acc = np.ascontiguousarray(prod[0][None])
                for j in range(1, geo.n1):
                    acc = orc.dyadic("add", acc, np.ascontiguousarray(prod[j][None]))
                S = orc.apply_galois(orc.ntt_inv(acc), pow(3, i * geo.n1, 2 * N))
                M = orc.dyadic("add", M, S)
            for s in geo.folds:
                M = orc.dyadic("add", M, orc.apply_galois(M, pow(3, s, 2 * N)))
            c0 = orc.rescale(M)[0]
            if bias is not None:
                c0 = (c0 + np.mod(bias[o][None, :], qcol[:-1]).astype(np.uint64)) % qnext
            out[o * T + t, 0] = c0
    return out


# ---- the bound of include/deeppowers/fhe.hpp with K = 0 (no key-switch error on a transparent input), term by term ---------------------------------
def error_bound(log2n, geo, W, b, Dx, Dw, q_last, tpc, X, Bin):
    """a bound on |decoded output row R - (W x + b)_R|: `pre` + the client's decode D; X = max|x_i|, Bin = the input's coefficient error"""
    N, two = float(1 << log2n), math.sqrt(2.0) if tpc == 2 else 1.0
    u8 = 8.0 * log2n * 2.0 ** -53
    Do = Dx * Dw / float(q_last)
    w_max, w_row1 = float(np.abs(W).max()), float(np.abs(W).sum(axis=1).max())
    B = (float(np.abs(b).max()) if b is not None else 0.0) * two
    X, n, n2, H = X * two, float(geo.n), float(geo.n2), (N + 1) / 2
    G = N * (0.5 + u8 * Dw * w_max)                      # a diagonal's slot, off its weight
    S = N * Bin                                          # a baby step's slot, off Dx x (K = 0)
    products = Dw * w_row1 * S + Dx * X * n * G + n * G * S
    e0 = n2 * H + (H if geo.n2 > 1 else 0.0)             # the divisions by P round nothing here, but the bound is the header's: its T3 terms stay
    windows = n / float(geo.m)
    eF = windows * e0 + (windows - 1) * H
    pre = (products + N * eF) / (Dx * Dw) + N * H / Do
    if b is not None:
        pre += N * (0.5 + u8 * Do * B) / Do
    Z = w_row1 * X + B
    return pre + u8 * N * (Z + pre)


def fresh_noise_bound(log2n, Dx, X, tpc):
    """Bin of a fresh ciphertext: |e| <= 21, the rounding 1/2 and E_x = u8 Dx X (slots of modulus <= sqrt(tpc) X)"""
    return NOISE + 0.5 + 8.0 * log2n * 2.0 ** -53 * Dx * X * math.sqrt(float(tpc))


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------
class Layer:
    def __init__(self, out_dim, in_dim, n1, n2, bias, weight_scale=2.0 ** 58):
        self.out_dim, self.in_dim, self.n1, self.n2, self.bias, self.weight_scale = out_dim, in_dim, n1, n2, bias, weight_scale


class Case:
    """One row of the issue's table.  n1 x n2 is the split the library is expected to choose (the GPU test holds the printed one to it)."""

    def __init__(self, name, log2n, layers, T, tpc, seed, chain="fold60", model="A"):
        self.name, self.log2n, self.layers, self.T, self.tpc, self.seed, self.chain, self.model = name, log2n, layers, T, tpc, seed, chain, model
        self.input_scale = 2.0 ** 50

    def params(self):
        """(data chain, special prime, its psi)"""
        k = len(self.layers)
        if self.chain == "fold60":          # 3 data limbs + P (4 + P chained) of the largest 60-bit primes
            p = ntt_primes(self.log2n, 3 + k)
        elif self.chain == "fold60_2":      # tests/test_gpu_large_ring_pipeline.py params("fold", 15): 2 data limbs + P
            p = ntt_primes(self.log2n, 3)
        elif self.chain == "mixed45":       # two fold limbs, then the largest prime below 2^45 (class f64) as the rescaling prime; P a fold prime
            f, s = ntt_primes(self.log2n, 3), ntt_primes(self.log2n, 1, 45)
            p = FheParams(self.log2n, f.moduli[:2] + s.moduli + f.moduli[2:], f.psi[:2] + s.psi + f.psi[2:])
        else:
            raise ValueError(self.chain)
        return p.drop_last_limb(), p.moduli[-1], p.psi[-1]

    def draw(self):
        """W, b of every layer, x [T * tpc][in_dim] uniform on [-1, 1] and e [T][N] uniform on [-21, 21], from the seed alone"""
        rng = np.random.default_rng(self.seed)
        Ws = [rng.uniform(-1.0, 1.0, (l.out_dim, l.in_dim)) for l in self.layers]
        bs = [rng.uniform(-1.0, 1.0, l.out_dim) for l in self.layers]
        x = rng.uniform(-1.0, 1.0, (self.T * self.tpc, self.layers[0].in_dim))
        e = rng.integers(-NOISE, NOISE + 1, (self.T, 1 << self.log2n))
        return Ws, [b if l.bias else None for b, l in zip(bs, self.layers)], x, e

    def input_polynomials(self, x, e):
        """m = twin(pack(x), input_scale) + e: int64 [T][N] - what a fresh ciphertext's phase would be"""
        l0 = self.layers[0]
        geo = Geometry(self.log2n, l0.out_dim, l0.in_dim, l0.n1, l0.n2)
        slots = np.stack([geo.pack(x[t * self.tpc], x[t * self.tpc + 1] if self.tpc == 2 else None) for t in range(self.T)])
        return np.array(ckks.encode_host(slots, self.input_scale, self.log2n), dtype=np.int64) + e


def L1(*a, **k):
    return [Layer(*a, **k)]


CASES = [
    Case("n10_2x2_bias", 10, L1(2, 2, 2, 1, True), 1, 1, 101),
    Case("n10_2x2", 10, L1(2, 2, 2, 1, False), 1, 1, 802),      # (seeds 102 .. 702 draw max|y| < 1)
    Case("n10_1x3_bias", 10, L1(1, 3, 2, 1, True), 2, 1, 103),
    Case("n10_16x16_bias", 10, L1(16, 16, 8, 2, True), 3, 1, 104),
    Case("n10_16x16", 10, L1(16, 16, 8, 2, False), 3, 1, 105),
    Case("n10_77x24_bias", 10, L1(77, 24, 16, 2, True), 3, 1, 106),
    Case("n10_12x100_pair_bias", 10, L1(12, 100, 8, 2, True), 2, 2, 107),
    Case("n10_12x100_pair", 10, L1(12, 100, 8, 2, False), 2, 2, 108),
    Case("n10_600x200_bias", 10, L1(600, 200, 32, 8, True), 2, 1, 109),
    Case("n11_16x16_pair_bias_mixed45", 11, L1(16, 16, 8, 2, True, weight_scale=2.0 ** 45), 2, 2, 110, chain="mixed45"),
    Case("n10_16x16_chained_bias", 10, [Layer(16, 16, 8, 2, True), Layer(16, 16, 8, 2, True)], 2, 1, 111),
    Case("n15_16x16_pair_bias", 15, L1(16, 16, 8, 2, True), 2, 2, 112, chain="fold60_2", model="B"),
]
SMALL = [c for c in CASES if c.model == "A"]


class Run:
    """the model of one case, layer after layer: geometry, encodings, scales and the words after each layer"""

    def __init__(self, case, model=None, perturb=None):
        """perturb: None, ("weight", layer, R, col, factor) or ("bias_scale_2_60", layer) - planted errors in the model's own inputs"""
        self.case = case
        data, self.special, self.special_psi = case.params()
        self.data = data
        Ws, bs, self.x, e = case.draw()
        if perturb and perturb[0] == "weight":
            Ws[perturb[1]] = Ws[perturb[1]].copy()
            Ws[perturb[1]][perturb[2], perturb[3]] *= perturb[4]
        self.Ws, self.bs = Ws, bs
        self.m = case.input_polynomials(self.x, e)
        self.c0 = np.stack([np.mod(self.m[t][None, :], np.array(data.moduli, dtype=np.int64)[:, None]).astype(np.uint64) for t in range(case.T)])
        model = model or case.model
        self.geos, self.scales, self.words, self.encodings = [], [case.input_scale], [], []
        moduli, psi, cur = list(data.moduli), list(data.psi), self.c0
        for k, (l, W, b) in enumerate(zip(case.layers, Ws, bs)):
            geo = Geometry(case.log2n, l.out_dim, l.in_dim, l.n1, l.n2)
            Do = output_scale(self.scales[-1], l.weight_scale, moduli[-1])
            bias_scale = self.scales[-1] * l.weight_scale / 2.0 ** 60 if perturb and perturb[0] == "bias_scale_2_60" and perturb[1] == k else None
            p, bias = encoded_layer(case.log2n, geo, W, b, l.weight_scale, Do, case.tpc, bias_scale)
            if model == "A":
                ms = [centred(cur[t], moduli) for t in range(case.T)]
                out = model_a(case.log2n, moduli, geo, p, bias, ms)
            else:
                out = model_b(case.log2n, moduli, psi, geo, p, bias, cur)
            self.geos.append(geo)
            self.scales.append(Do)
            self.words.append(out)
            self.encodings.append((p, bias))
            moduli, psi = moduli[:-1], psi[:-1]
            assert geo.passes == 1 or k + 1 == len(case.layers)
            cur = np.ascontiguousarray(out[:, 0])          # the next layer's transparent input: [T][L - 1][N]

    def decoded(self, k):
        """layer k's output decoded at its output scale: complex [passes * T][N/2]"""
        moduli = list(self.data.moduli)[:len(self.data.moduli) - 1 - k]
        coeffs = np.stack([centred(self.words[k][i, 0], moduli).astype(np.int64) for i in range(self.words[k].shape[0])])
        return ckks.decode_host(coeffs, self.scales[k + 1], self.case.log2n)

    def write_case_file(self, path):
        c, d = self.case, self.data
        u, f = lambda *v: struct.pack(f"<{len(v)}Q", *v), lambda *v: struct.pack(f"<{len(v)}d", *v)
        with open(path, "wb") as fh:
            fh.write(u(MAGIC, c.log2n, len(d.moduli), *d.moduli, *d.psi, self.special, self.special_psi, c.T, c.tpc, len(c.layers)) + f(c.input_scale))
            for l, W, b in zip(c.layers, self.Ws, self.bs):
                fh.write(u(l.out_dim, l.in_dim, 1 if l.bias else 0) + f(l.weight_scale))
                fh.write(np.ascontiguousarray(W, dtype="<f8").tobytes())
                if l.bias:
                    fh.write(np.ascontiguousarray(b, dtype="<f8").tobytes())
            fh.write(np.ascontiguousarray(self.c0, dtype="<u8").tobytes())


def build_words_program():
    return cpp_build.build_program("approx_layer_words")
