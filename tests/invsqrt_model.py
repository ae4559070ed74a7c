"""An exact integer model of ApproxInvSqrt on TRANSPARENT inputs (include/deeppowers/fhe.hpp): with c1 = 0 every relinearisation digit is zero, every
division by P is exact, and K Newton steps y <- 1.5 y - 0.5 (v y)(y y) are a deterministic integer function of the input polynomials mu_v and mu_0:

    mu_a = round(mu_v (*) mu_n / q_a),   mu_b = round(mu_n (*) mu_n / q_a),   mu_{n+1} = round((w_n mu_n - mu_a (*) mu_b) / q_b)
    q_a, q_b the last primes of levels 2 n and 2 n + 1 (level r = the input's limbs without the last r), (*) the product in Z[X] / (X^N + 1)
    s_0 = guess_scale;  s_a = (v_scale * s_n) / float(q_a);  s_b = (s_n * s_n) / float(q_a);  top = 2.0 * (s_a * s_b);  w_n = llround(1.5 * (top / s_n));
    s_{n+1} = top / float(q_b)

in Python integers and doubles (IEEE, the same operations in the same order as the library).  A plain helper like tests/approx_poly_model.py, whose big-integer
tools it borrows; tests/test_invsqrt_model_cpu.py holds the model to the float64 iteration, tests/test_gpu_invsqrt_words.py holds the device to the model."""
import functools
import math
import os
import struct

import numpy as np

import approx_layer_model as alm
import approx_poly_model as apm
import cpp_build
from deeppowers_amd import ckks
from deeppowers_amd.params import ntt_primes

MAGIC = int.from_bytes(b"AISW1", "little")
V_SCALE = 2.0 ** 60
V_MIN, V_MAX = 0.1, 1.0                 # the variance range of the cases
GUESS_OFF = 0.1                         # the cases' guesses are (1 +- GUESS_OFF) / sqrt(v)
SCALE_MIN, SCALE_MAX = 2.0 ** 20, 2.0 ** 62


def balanced_guess_scale(v_scale, q_a, q_b):
    return math.sqrt((float(q_a) * float(q_a)) * (float(q_b) / (2.0 * v_scale)))


def step_scales(drop, v_scale, guess_scale):
    """drop[r] = the last prime of level r (2 K of them) -> (s [K + 1], steps [(s_a, s_b, top, w_n)])"""
    s, steps = [float(guess_scale)], []
    for n in range(len(drop) // 2):
        q_a, q_b = float(drop[2 * n]), float(drop[2 * n + 1])
        s_a = (v_scale * s[n]) / q_a
        s_b = (s[n] * s[n]) / q_a
        top = 2.0 * (s_a * s_b)
        steps.append((s_a, s_b, top, apm.llround(1.5 * (top / s[n]))))
        s.append(top / q_b)
    return s, steps


def float_iteration(v, y0, K):
    """[y_0, .., y_K] in float64, in the operations the bound is stated against"""
    ys = [np.asarray(y0, dtype=np.float64)]
    for _ in range(K):
        y = ys[-1]
        ys.append(1.5 * y - 0.5 * ((v * y) * (y * y)))
    return ys


def model(moduli, K, v_scale, guess_scale, mu_v, mu_y):
    """moduli: the input level's data limbs (>= 2 K + 1).  mu_v, mu_y: T integer polynomials each -> (words uint64 [T][2][L - 2 K][N], s, w)"""
    L0 = len(moduli)
    drop = [moduli[L0 - 1 - r] for r in range(2 * K)]
    out_moduli = moduli[:L0 - 2 * K]
    s, steps = step_scales(drop, v_scale, guess_scale)
    N = len(mu_v[0])
    words = np.zeros((len(mu_v), 2, len(out_moduli), N), dtype=np.uint64)
    for t in range(len(mu_v)):
        mv = np.array([int(x) for x in mu_v[t]], dtype=object)
        m = np.array([int(x) for x in mu_y[t]], dtype=object)
        for n in range(K):
            q_a, q_b, w = drop[2 * n], drop[2 * n + 1], steps[n][3]
            a = apm.round_div(apm.negacyclic(mv, m), q_a)
            b = apm.round_div(apm.negacyclic(m, m), q_a)
            m = apm.round_div(w * m - apm.negacyclic(a, b), q_b)
        words[t, 0] = alm.residues(m, out_moduli)
    return words, s, [st[3] for st in steps]


def error_bound(log2n, moduli, specials, v_scale, guess_scale, V, Y, Bv, By, keyswitch=True):
    """ApproxInvSqrt::error_bound (include/deeppowers/fhe.hpp), restated; keyswitch=False: K_r = 0, the transparent inputs' bound"""
    depth, L0 = len(specials), len(moduli)
    N, u = float(1 << log2n), 2.0 ** -53
    H, u8 = (N + 1) / 2, 8.0 * log2n * u
    drop = [moduli[L0 - 1 - r] for r in range(depth)]
    Kr = [21.0 * (L0 - r) * N * (max(moduli[:L0 - r]) / specials[r]) if keyswitch else 0.0 for r in range(depth)]
    s, steps = step_scales(drop, v_scale, guess_scale)
    Dv, E, F = N * Bv, N * By, 0.0
    g, f = 1.5 * (1 + V * Y * Y), 8 * u * (1.5 * Y + 0.5 * V * Y ** 3)
    for n in range(depth // 2):
        s_a, s_b, top, _ = steps[n]
        q_a, q_b = float(drop[2 * n]), float(drop[2 * n + 1])
        Da = (v_scale * V * E + s[n] * Y * Dv + Dv * E + N * (Kr[2 * n] + H)) / q_a + N * H + 4 * u * s_a * V * Y
        Db = (2 * s[n] * Y * E + E * E + N * (Kr[2 * n] + H)) / q_a + N * H + 4 * u * s_b * Y * Y
        R = 0.5 + 4 * u * 1.5 * (top / s[n])
        w = 1.5 * (top / s[n]) + R
        E = (s_a * V * Y * Db + s_b * Y * Y * Da + Da * Db + N * (Kr[2 * n + 1] + H) + w * E + R * s[n] * Y + u * top * V * Y ** 3) / q_b + N * H + 2 * u * s[n + 1] * Y
        F = g * F + f
    pre = E / s[-1]
    return pre + u8 * N * (Y + pre) + F


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------
class Case:
    """K steps at ring degree 2^log2n, T tokens: the largest 60-bit primes, 2 K + 2 data limbs (two are left at the output) and the special prime;
    v_scale = 2^60 and the balanced guess scale"""

    def __init__(self, log2n, K, T, seed):
        self.log2n, self.K, self.T, self.seed = log2n, K, T, seed
        self.name = f"n{1 << log2n}_K{K}_T{T}"

    def params(self):
        p = ntt_primes(self.log2n, 2 * self.K + 3)
        return p.drop_last_limb(), p.moduli[-1], p.psi[-1]

    def draw(self):
        """v [T][N/2] uniform on [V_MIN, V_MAX]; the guess (1 + d) / sqrt(v), d uniform on [-GUESS_OFF, GUESS_OFF]; e_v, e_y [T][N] uniform on [-21, 21]"""
        rng = np.random.default_rng(self.seed)
        shape = (self.T, (1 << self.log2n) // 2)
        v = rng.uniform(V_MIN, V_MAX, shape)
        y0 = (1.0 + rng.uniform(-GUESS_OFF, GUESS_OFF, shape)) / np.sqrt(v)
        e = rng.integers(-alm.NOISE, alm.NOISE + 1, (2, self.T, 1 << self.log2n))
        return v, y0, e[0], e[1]


@functools.lru_cache(maxsize=None)
def run(log2n, K, T, seed):
    return Run(Case(log2n, K, T, seed))


class Run:
    def __init__(self, case):
        self.case = case
        self.data, self.special, self.special_psi = case.params()
        q = self.data.moduli
        self.guess_scale = balanced_guess_scale(V_SCALE, q[-1], q[-2])
        self.v, self.y0, e_v, e_y = case.draw()
        self.m_v = np.array(ckks.encode_host(self.v, V_SCALE, case.log2n), dtype=np.int64) + e_v
        self.m_y = np.array(ckks.encode_host(self.y0, self.guess_scale, case.log2n), dtype=np.int64) + e_y
        mods = np.array(q, dtype=np.int64)[:, None]
        res = lambda m: np.stack([np.mod(m[t][None, :], mods).astype(np.uint64) for t in range(case.T)])
        self.c0_v, self.c0_y = res(self.m_v), res(self.m_y)
        T = range(case.T)
        self.words, self.s, self.w = model(list(q), case.K, V_SCALE, self.guess_scale, [self.m_v[t] for t in T], [self.m_y[t] for t in T])
        self.iterates = float_iteration(self.v, self.y0, case.K)
        self.want = self.iterates[-1]

    def magnitudes(self):
        """(V, Y): max|v| and a bound on every iterate (float64 and real: a hair above the float64 maximum)"""
        return float(np.abs(self.v).max()), float(max(np.abs(y).max() for y in self.iterates)) * (1 + 2.0 ** -40)

    def noise_bounds(self):
        V, _ = self.magnitudes()
        return (alm.fresh_noise_bound(self.case.log2n, V_SCALE, V, 1), alm.fresh_noise_bound(self.case.log2n, self.guess_scale, float(np.abs(self.y0).max()), 1))

    def decoded(self):
        out_moduli = list(self.data.moduli)[:self.words.shape[2]]
        coeffs = np.stack([alm.centred(self.words[t, 0], out_moduli).astype(np.int64) for t in range(self.case.T)])
        return ckks.decode_host(coeffs, self.s[-1], self.case.log2n)

    def write_case_file(self, path, tokens=None):
        """the case of tests/cpp/newton/invsqrt_words.cpp, with the first `tokens` tokens (default: all)"""
        c, d = self.case, self.data
        T = c.T if tokens is None else tokens
        u, f = lambda *v: struct.pack(f"<{len(v)}Q", *v), lambda *v: struct.pack(f"<{len(v)}d", *v)
        with open(path, "wb") as fh:
            fh.write(u(MAGIC, c.log2n, len(d.moduli), *d.moduli, *d.psi, self.special, self.special_psi, T, c.K) + f(V_SCALE, self.guess_scale))
            fh.write(np.ascontiguousarray(self.c0_v[:T], dtype="<u8").tobytes())
            fh.write(np.ascontiguousarray(self.c0_y[:T], dtype="<u8").tobytes())


def _build(name, **needs):
    """tests/cpp/newton/<name>.cpp -> tests/cpp/bin/newton/<name> through tests/cpp_build.py, which makes tests/cpp/bin but no directory below it"""
    os.makedirs(os.path.join(cpp_build.BIN_DIR, "newton"), exist_ok=True)
    return cpp_build.build_program("newton/" + name, **needs)


def build_words_program():
    return _build("invsqrt_words")


def build_api_test():
    return _build("test_invsqrt_api", gate=True)
