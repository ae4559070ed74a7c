"""An exact integer model of ApproxDivide on TRANSPARENT inputs (include/deeppowers/fhe.hpp): with c1 = 0 every relinearisation digit is zero, every division
by P is exact, and K Goldschmidt steps F = 2 - D; n_j <- n_j F; D <- D F are a deterministic integer function of the input polynomials mu_D and mu_j:

    mu_F = kappa_n X^0 - mu_D  (kappa_n on coefficient 0),   mu_j' = round(mu_j (*) mu_F / q_n),   mu_D' = round(mu_D (*) mu_F / q_n)
    q_n the last prime of level n (level n = the input's limbs without the last n), (*) the product in Z[X] / (X^N + 1); the last step computes no mu_D'
    sigma_0 = den_scale, nu_0 = num_scale;  kappa_n = llround(2.0 * sigma_n);  sigma_{n+1} = (sigma_n * sigma_n) / float(q_n);  nu_{n+1} = (nu_n * sigma_n) / float(q_n)

in Python integers and doubles (IEEE, the same operations in the same order as the library).  A plain helper like tests/invsqrt_model.py, whose big-integer
tools (tests/approx_poly_model.py) it borrows; tests/test_divide_model_cpu.py holds the model to the float64 iteration, tests/test_gpu_divide_words.py holds the
device to the model."""
import functools
import math
import os
import struct

import numpy as np

import approx_layer_model as alm
import approx_poly_model as apm
import cpp_build
from deeppowers_amd import ckks
from deeppowers_amd.params import FheParams, ntt_primes

MAGIC = int.from_bytes(b"ADVW1", "little")
NUM_SCALE = 2.0 ** 50
D_LO, D_HI = 0.6, 1.4                   # the cases' denominators as read at den_scale: D_0 = c d with the constant guess folded in
NUM_MAX = 1.0
SCALE_MIN, SCALE_MAX = 2.0 ** 20, 2.0 ** 62


def guess(lo, hi):
    return 2.0 / (lo + hi)


def residual(lo, hi, K):
    r = (hi - lo) / (hi + lo)
    for _ in range(K):
        r = r * r
    return r


def step_scales(drop, num_scale, den_scale):
    """drop[n] = the last prime of level n (K of them) -> (sigma [K + 1], nu [K + 1], kappa [K])"""
    sigma, nu, kappa = [float(den_scale)], [float(num_scale)], []
    for n, q in enumerate(drop):
        kappa.append(apm.llround(2.0 * sigma[n]))
        sigma.append((sigma[n] * sigma[n]) / float(q))
        nu.append((nu[n] * sigma[n]) / float(q))
    return sigma, nu, kappa


def invalid(drop, num_scale, den_scale):
    """the constructor's INVALID_ARGUMENT conditions that need no device: None when the scales are admissible, otherwise which one is not"""
    if not drop:
        return "no steps"
    if not (math.isfinite(num_scale) and num_scale > 0 and math.isfinite(den_scale) and den_scale > 0):
        return "scale not finite and positive"
    sigma, nu = float(den_scale), float(num_scale)
    for q in drop:
        if not (SCALE_MIN <= sigma < SCALE_MAX and SCALE_MIN <= nu < SCALE_MAX):
            return "scale outside [2^20, 2^62)"
        if not 2.0 * sigma < 2.0 ** 62:
            return "kappa reaches 2^62"
        sigma, nu = (sigma * sigma) / float(q), (nu * sigma) / float(q)
    return None if SCALE_MIN <= sigma < SCALE_MAX and SCALE_MIN <= nu < SCALE_MAX else "scale outside [2^20, 2^62)"


def float_iteration(num, den, K):
    """num [G][T][...], den [G][...] -> ([n_0, .., n_K], [D_0, .., D_K]) in float64, in the operations the bound is stated against"""
    ns, ds = [np.asarray(num, dtype=np.float64)], [np.asarray(den, dtype=np.float64)]
    for _ in range(K):
        F = 2.0 - ds[-1]
        ns.append(ns[-1] * F[:, None])
        ds.append(ds[-1] * F)
    return ns, ds


def model(moduli, K, num_scale, den_scale, mu_num, mu_den):
    """moduli: the input level's data limbs (>= K + 1).  mu_num: G lists of T integer polynomials, mu_den: G integer polynomials ->
    (words uint64 [G * T][2][L - K][N], sigma, nu, kappa)"""
    L0 = len(moduli)
    drop = [moduli[L0 - 1 - n] for n in range(K)]
    out_moduli = moduli[:L0 - K]
    sigma, nu, kappa = step_scales(drop, num_scale, den_scale)
    G, T, N = len(mu_den), len(mu_num[0]), len(mu_den[0])
    words = np.zeros((G * T, 2, len(out_moduli), N), dtype=np.uint64)
    for g in range(G):
        D = np.array([int(x) for x in mu_den[g]], dtype=object)
        ms = [np.array([int(x) for x in m], dtype=object) for m in mu_num[g]]
        for n in range(K):
            F = -D
            F[0] += kappa[n]
            ms = [apm.round_div(apm.negacyclic(m, F), drop[n]) for m in ms]
            if n + 1 < K:
                D = apm.round_div(apm.negacyclic(D, F), drop[n])
        for j in range(T):
            words[g * T + j, 0] = alm.residues(ms[j], out_moduli)
    return words, sigma, nu, kappa


def error_bound(log2n, moduli, specials, num_scale, den_scale, Dm, X, Bd, Bn, keyswitch=True):
    """ApproxDivide::error_bound (include/deeppowers/fhe.hpp), restated; keyswitch=False: K_n = 0, the transparent inputs' bound"""
    K, L0 = len(specials), len(moduli)
    N, u = float(1 << log2n), 2.0 ** -53
    H, u8 = (N + 1) / 2, 8.0 * log2n * u
    drop = [moduli[L0 - 1 - n] for n in range(K)]
    Kn = [21.0 * (L0 - n) * N * (max(moduli[:L0 - n]) / specials[n]) if keyswitch else 0.0 for n in range(K)]
    sigma, nu, _ = step_scales(drop, num_scale, den_scale)
    assert 0 <= Dm <= 2                       # every D_n in [0, Dm]: |F_n| = |2 - D_n| <= Fm = 2
    Fm = 2.0
    E, G, Psi, Phi = N * Bd, N * Bn, 0.0, 0.0
    for n in range(K):
        q, f, relin = float(drop[n]), E + 0.5, N * (Kn[n] + H)
        G1 = (nu[n] * X * f + sigma[n] * Fm * G + G * f + relin) / q + N * H + 4 * u * nu[n + 1] * X
        E1 = (sigma[n] * (Dm * f + Fm * E) + E * f + relin) / q + N * H + 4 * u * sigma[n + 1] * Dm
        Phi, Psi = Fm * Phi + X * Psi + 4 * u * X * Fm, (Fm + Dm) * Psi + 4 * u * Dm * Fm
        E, G = E1, G1
    pre = G / nu[-1]
    return pre + u8 * N * (X + pre) + Phi


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------
class Case:
    """K steps at ring degree 2^log2n, G groups of T numerators: the largest 60-bit primes, K + 2 data limbs (two are left at the output: a quotient near 1 at
    a scale near the primes needs them) and the special prime - or the given parameters (data limbs and the special prime last); the numerators at 2^50, the
    denominator at the last prime's size, where sigma_n stays"""

    def __init__(self, log2n, K, G, T, seed, params=None, num_scale=NUM_SCALE):
        self.log2n, self.K, self.G, self.T, self.seed, self.given, self.num_scale = log2n, K, G, T, seed, params, num_scale
        self.name = f"n{1 << log2n}_K{K}_{G}x{T}"

    def params(self):
        p = self.given if self.given is not None else ntt_primes(self.log2n, self.K + 3)
        return p.drop_last_limb(), p.moduli[-1], p.psi[-1]

    def draw(self):
        """den [G][N/2] uniform on [D_LO, D_HI]; num [G][T][N/2] uniform on [-NUM_MAX, NUM_MAX]; e_d [G][N], e_n [G][T][N] uniform on [-21, 21]"""
        rng = np.random.default_rng(self.seed)
        row, N = (1 << self.log2n) // 2, 1 << self.log2n
        den = rng.uniform(D_LO, D_HI, (self.G, row))
        num = rng.uniform(-NUM_MAX, NUM_MAX, (self.G, self.T, row))
        return num, den, rng.integers(-alm.NOISE, alm.NOISE + 1, (self.G, self.T, N)), rng.integers(-alm.NOISE, alm.NOISE + 1, (self.G, N))


@functools.lru_cache(maxsize=None)
def run(log2n, K, G, T, seed):
    return Run(Case(log2n, K, G, T, seed))


class Run:
    def __init__(self, case):
        self.case = case
        self.data, self.special, self.special_psi = case.params()
        q = self.data.moduli
        c = case
        self.num_scale, self.den_scale = c.num_scale, float(q[-1])
        self.num, self.den, e_n, e_d = c.draw()
        N = 1 << c.log2n
        self.m_n = np.array(ckks.encode_host(self.num.reshape(c.G * c.T, -1), self.num_scale, c.log2n), dtype=np.int64).reshape(c.G, c.T, N) + e_n
        self.m_d = np.array(ckks.encode_host(self.den, self.den_scale, c.log2n), dtype=object) + e_d
        mods = [int(v) for v in q]
        self.c0_n = np.stack([alm.residues(self.m_n[g, j], mods) for g in range(c.G) for j in range(c.T)])
        self.c0_d = np.stack([alm.residues(self.m_d[g], mods) for g in range(c.G)])
        self.words, self.sigma, self.nu, self.kappa = model(mods, c.K, self.num_scale, self.den_scale, [[self.m_n[g, j] for j in range(c.T)] for g in range(c.G)],
                                                            [self.m_d[g] for g in range(c.G)])
        self.n_iter, self.d_iter = float_iteration(self.num, self.den, c.K)
        self.want = self.n_iter[-1]

    def magnitudes(self):
        """(Dm, X): bounds on every |D_n| and every numerator iterate (float64 and real: a hair above the float64 maxima)"""
        hair = 1 + 2.0 ** -40
        return float(max(np.abs(d).max() for d in self.d_iter)) * hair, float(max(np.abs(n).max() for n in self.n_iter)) * hair

    def noise_bounds(self):
        """(Bd, Bn)"""
        return (alm.fresh_noise_bound(self.case.log2n, self.den_scale, float(np.abs(self.den).max()), 1),
                alm.fresh_noise_bound(self.case.log2n, self.num_scale, float(np.abs(self.num).max()), 1))

    def decoded(self):
        """the model's output words decoded at nu_K: complex [G][T][N/2]"""
        c = self.case
        out_moduli = [int(v) for v in self.data.moduli][:self.words.shape[2]]
        coeffs = np.stack([alm.centred(self.words[i, 0], out_moduli).astype(np.int64) for i in range(c.G * c.T)])
        return ckks.decode_host(coeffs, self.nu[-1], c.log2n).reshape(c.G, c.T, -1)

    def write_case_file(self, path):
        """the case of tests/cpp/divide/divide_words.cpp"""
        c, d = self.case, self.data
        u, f = lambda *v: struct.pack(f"<{len(v)}Q", *v), lambda *v: struct.pack(f"<{len(v)}d", *v)
        with open(path, "wb") as fh:
            fh.write(u(MAGIC, c.log2n, len(d.moduli), *d.moduli, *d.psi, self.special, self.special_psi, c.G, c.T, c.K) + f(self.num_scale, self.den_scale))
            fh.write(np.ascontiguousarray(self.c0_n, dtype="<u8").tobytes())
            fh.write(np.ascontiguousarray(self.c0_d, dtype="<u8").tobytes())


def _build(name, **needs):
    """tests/cpp/divide/<name>.cpp -> tests/cpp/bin/divide/<name> through tests/cpp_build.py, which makes tests/cpp/bin but no directory below it"""
    os.makedirs(os.path.join(cpp_build.BIN_DIR, "divide"), exist_ok=True)
    return cpp_build.build_program("divide/" + name, **needs)


def build_words_program():
    return _build("divide_words")


def build_api_test():
    return _build("test_divide_api", gate=True)
