"""An exact integer model of ApproxPolynomial on a TRANSPARENT input (include/deeppowers/fhe.hpp): with c1 = 0 every relinearisation digit is zero, every
division by P is exact, and the polynomial is a deterministic integer function of the input polynomial mu_1, the coefficients and the scales:

    mu_k = round(mu_i (*) mu_j / q_r),   i = 2^(r-1), j = k - i, r = ceil(log2 k), q_r the last prime of depth r - 1, (*) the product in Z[X] / (X^N + 1)
    M    = sum_{k=1..d} c_k mu_k + c_0 X^0,        out = round(M / q*),  q* the last prime of depth r* = ceil(log2 d)
    s_1 = input_scale,  s_k = (s_i * s_j) / float(q_r),  c_k = llround(a_k * ((S * float(q*)) / s_k)),  c_0 = llround(a_0 * S) * q*  (an exact integer)

in Python integers and doubles (IEEE, the same operations in the same order as the library; llround rounds half away from zero, Python's round does not).
Every division is by an odd prime, so round(x / q) = floor((2 x + q) / (2 q)) has no tie.  A plain helper like tests/approx_layer_model.py, whose big-integer
tools it borrows; tests/test_approx_poly_model_cpu.py holds the model to the float64 p(x), tests/test_gpu_approx_poly_words.py holds the device to the model."""
import functools
import math
import struct

import numpy as np

import approx_layer_model as alm
import cpp_build
from deeppowers_amd import ckks
from deeppowers_amd.params import ntt_primes

MAGIC = int.from_bytes(b"APPW1", "little")
INPUT_SCALE, OUTPUT_SCALE, X_MAX = 2.0 ** 59, 2.0 ** 50, 2.0


def ceil_log2(k):
    return (k - 1).bit_length()


def llround(v):
    """C's llround: the nearest integer, halves away from zero (|v| - floor|v| is exact in doubles)"""
    a = abs(v)
    r = math.floor(a)
    if a - r >= 0.5:
        r += 1
    return int(r) if v >= 0 else -int(r)


def power_scales(d, input_scale, drop):
    """s[1..d]; drop[r - 1] = the prime a product at level r drops"""
    s = [0.0, float(input_scale)] + [0.0] * (d - 1)
    for k in range(2, d + 1):
        r = ceil_log2(k)
        i = 1 << (r - 1)
        s[k] = (s[i] * s[k - i]) / float(drop[r - 1])
    return s


def weights(coeffs, s, out_scale, q_star):
    top = out_scale * float(q_star)
    return [llround(coeffs[0] * out_scale) * q_star] + [llround(coeffs[k] * (top / s[k])) for k in range(1, len(coeffs))]


def _pack(values, slot_bits):
    nb = slot_bits // 8
    zero = bytes(nb)
    pos = b"".join(int(v).to_bytes(nb, "little") if v > 0 else zero for v in values)
    neg = b"".join(int(-v).to_bytes(nb, "little") if v < 0 else zero for v in values)
    return int.from_bytes(pos, "little") - int.from_bytes(neg, "little")


def negacyclic(a, b):
    """a (*) b in Z[X] / (X^N + 1) for object arrays of Python integers, by Kronecker substitution"""
    N = len(a)
    bound = N * max(1, max(abs(int(v)) for v in a)) * max(1, max(abs(int(v)) for v in b))
    slot_bits = 64 * -(-(bound.bit_length() + 2) // 64)
    return alm._unpack_negacyclic(_pack(a, slot_bits) * _pack(b, slot_bits), N, slot_bits)


def round_div(x, q):
    return (2 * x + q) // (2 * q)


def powers(mu, d, drop):
    """mu_1 .. mu_d (index 0 unused) of one input polynomial"""
    m = [None, np.array([int(v) for v in mu], dtype=object)]
    for k in range(2, d + 1):
        r = ceil_log2(k)
        i = 1 << (r - 1)
        m.append(round_div(negacyclic(m[i], m[k - i]), drop[r - 1]))
    return m


def model(moduli, coeffs, input_scale, out_scale, mus):
    """moduli: the input level's data limbs (>= ceil(log2 d) + 2).  mus: T integer polynomials -> (words uint64 [T][2][L_out][N], s, c)"""
    d = len(coeffs) - 1
    rstar = ceil_log2(d)
    L0 = len(moduli)
    drop = [moduli[L0 - 1 - r] for r in range(rstar)]
    q_star = moduli[L0 - 1 - rstar]
    out_moduli = moduli[:L0 - rstar - 1]
    s = power_scales(d, input_scale, drop)
    c = weights(coeffs, s, out_scale, q_star)
    N = len(mus[0])
    words = np.zeros((len(mus), 2, len(out_moduli), N), dtype=np.uint64)
    for t, mu in enumerate(mus):
        m = powers(mu, d, drop)
        M = np.zeros(N, dtype=object)
        for k in range(1, d + 1):
            M = M + c[k] * m[k]
        M[0] += c[0]
        words[t, 0] = alm.residues(round_div(M, q_star), out_moduli)
    return words, s, c


def error_bound(log2n, moduli, specials, coeffs, input_scale, out_scale, X, Bin, keyswitch=True):
    """ApproxPolynomial::error_bound (include/deeppowers/fhe.hpp), restated; keyswitch=False: K_r = 0, the transparent input's bound"""
    d, rstar, L0 = len(coeffs) - 1, len(specials), len(moduli)
    N, u = float(1 << log2n), 2.0 ** -53
    H, u8 = (N + 1) / 2, 8.0 * log2n * u
    drop = [moduli[L0 - 1 - r] for r in range(rstar)]
    K = [21.0 * (L0 - r) * N * (max(moduli[:L0 - r]) / specials[r]) if keyswitch else 0.0 for r in range(rstar)]
    s = power_scales(d, input_scale, drop)
    D = [0.0, N * Bin] + [0.0] * (d - 1)
    for k in range(2, d + 1):
        r = ceil_log2(k)
        i = 1 << (r - 1)
        j = k - i
        D[k] = (s[i] * X ** i * D[j] + s[j] * X ** j * D[i] + D[i] * D[j] + N * (K[r - 1] + H)) / float(drop[r - 1]) + N * H + 4 * u * s[k] * X ** k
    top = out_scale * float(moduli[L0 - rstar - 1])
    total, A = float(moduli[L0 - rstar - 1]) * (0.5 + 2 * u * abs(coeffs[0]) * out_scale), abs(coeffs[0])
    for k in range(1, d + 1):
        ak = abs(coeffs[k])
        R = 0.5 + 4 * u * ak * top / s[k]
        total += R * s[k] * X ** k + ak * (top / s[k]) * D[k] + R * D[k]
        A += ak * X ** k
    pre = total / top + N * H / out_scale
    return pre + u8 * N * (A + pre)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------
class Case:
    """degree d at ring degree 2^log2n, T tokens: the largest 60-bit primes, ceil(log2 d) + 2 data limbs and the special prime"""

    def __init__(self, log2n, d, T, seed):
        self.log2n, self.d, self.T, self.seed = log2n, d, T, seed
        self.name = f"n{1 << log2n}_d{d}_T{T}"

    def params(self):
        p = ntt_primes(self.log2n, ceil_log2(self.d) + 3)
        return p.drop_last_limb(), p.moduli[-1], p.psi[-1]

    def draw(self):
        """a_0 = 2 and sum_{k >= 1} |a_k| X^k <= 0.9, so 1.1 <= p(x) <= 2.9 on [-X, X]; x [T][N/2] uniform on [-X, X]; e [T][N] uniform on [-21, 21]"""
        rng = np.random.default_rng(self.seed)
        a = [2.0] + [float(rng.uniform(0.5, 1.0) * rng.choice([-1.0, 1.0]) * 0.9 / (self.d * X_MAX ** k)) for k in range(1, self.d + 1)]
        x = rng.uniform(-X_MAX, X_MAX, (self.T, (1 << self.log2n) // 2))
        e = rng.integers(-alm.NOISE, alm.NOISE + 1, (self.T, 1 << self.log2n))
        return a, x, e


@functools.lru_cache(maxsize=None)
def run(log2n, d, T, seed):
    return Run(Case(log2n, d, T, seed))


class Run:
    def __init__(self, case):
        self.case = case
        self.data, self.special, self.special_psi = case.params()
        self.coeffs, self.x, e = case.draw()
        self.m = np.array(ckks.encode_host(self.x, INPUT_SCALE, case.log2n), dtype=np.int64) + e
        mods = np.array(self.data.moduli, dtype=np.int64)[:, None]
        self.c0 = np.stack([np.mod(self.m[t][None, :], mods).astype(np.uint64) for t in range(case.T)])
        self.words, self.s, self.c = model(list(self.data.moduli), self.coeffs, INPUT_SCALE, OUTPUT_SCALE, [self.m[t] for t in range(case.T)])
        self.want = sum(a * self.x ** k for k, a in enumerate(self.coeffs))        # float64 p(x) [T][N/2]

    def decoded(self):
        out_moduli = list(self.data.moduli)[:self.words.shape[2]]
        coeffs = np.stack([alm.centred(self.words[t, 0], out_moduli).astype(np.int64) for t in range(self.case.T)])
        return ckks.decode_host(coeffs, OUTPUT_SCALE, self.case.log2n)

    def write_case_file(self, path, tokens=None):
        """the case of tests/cpp/approx_poly_words.cpp, with the first `tokens` tokens (default: all)"""
        c, d = self.case, self.data
        T = c.T if tokens is None else tokens
        u, f = lambda *v: struct.pack(f"<{len(v)}Q", *v), lambda *v: struct.pack(f"<{len(v)}d", *v)
        with open(path, "wb") as fh:
            fh.write(u(MAGIC, c.log2n, len(d.moduli), *d.moduli, *d.psi, self.special, self.special_psi, T, c.d) + f(INPUT_SCALE, OUTPUT_SCALE, *self.coeffs))
            fh.write(np.ascontiguousarray(self.c0[:T], dtype="<u8").tobytes())


def build_words_program():
    return cpp_build.build_program("approx_poly_words")


def build_api_test():
    return cpp_build.build_program("test_approx_poly_api", gate=True)
