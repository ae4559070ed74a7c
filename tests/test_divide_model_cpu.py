"""The exact integer model of ApproxDivide on transparent inputs (tests/divide_model.py), held on the CPU before the GPU test relies on it:
  - at N = 256, K = 1, 3 and 5 Goldschmidt steps, 2 groups of 3 numerators, the model's output decodes to the float64 iteration F = 2 - D; n = n F; D = D F from
    the values encoded in every slot within the header's bound evaluated with K_n = 0 (transparent inputs have no key-switch error) - derived, not measured;
    every case has max|n / D| >= 1 and a bound below 2^-20 of it;
  - the closed form D_K = 1 - (1 - D_0)^(2^K) and n_K = (n_0 / D_0) D_K in float64, and residual / guess;
  - the scales and constants are the rule's double operations against exact rationals within the stated number of roundings, and a mismatch of the
    denominator's scale grows like (1 + delta)^(2^n);
  - every INVALID_ARGUMENT condition of the constructor that needs no device, in the model and - through the static error_bound, which runs the same rule - in
    the library (tests/cpp/divide/test_divide_api.cpp ref), whose bound the model's restatement equals;
  - the model has the resolution claimed: a constant off by 2^-40 of itself changes words, a scale rule that divides by 2^60 instead of the prime changes
    scales, and a group's words do not depend on its neighbours."""
import math
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import approx_poly_model as apm
import divide_model as dm

STEPS = (1, 3, 5)


@pytest.mark.parametrize("K", STEPS)
def test_model_decodes_to_the_float64_iteration_within_the_derived_bound(K):
    r = dm.run(8, K, 2, 3, 400 + K)
    q = [int(v) for v in r.data.moduli]
    assert len(q) == K + 2 and r.words.shape == (6, 2, 2, 256) and not r.words[:, 1].any()
    assert r.sigma[0] == r.den_scale == float(q[-1]) and r.nu[0] == dm.NUM_SCALE
    assert all(k < 2 ** 62 for k in r.kappa) and all(dm.SCALE_MIN <= s < dm.SCALE_MAX for s in r.sigma + r.nu)
    assert all(abs(s / r.den_scale - 1) < 2.0 ** -16 for s in r.sigma)            # at the primes sigma_n stays there (they differ by less than 2^-24 each)
    Dm, X = r.magnitudes()
    Bd, Bn = r.noise_bounds()
    bound = dm.error_bound(8, q, [r.special] * K, r.num_scale, r.den_scale, Dm, X, Bd, Bn, keyswitch=False)
    full = dm.error_bound(8, q, [r.special] * K, r.num_scale, r.den_scale, Dm, X, Bd, Bn)
    z = r.decoded()
    worst = max(float(np.abs(z.real - r.want).max()), float(np.abs(z.imag).max()))
    quotient = r.num / r.den[:, None]
    qmax = float(np.abs(quotient).max())
    closed = np.abs(1.0 - r.den) ** (2 ** K)
    off = np.abs(z.real - quotient)
    print(f"{r.case.name}: max|n/D| {qmax:.3f}, max error 2^{math.log2(max(worst, 1e-300)):.2f}, bound (K_n = 0) 2^{math.log2(bound):.2f}, "
          f"with key switches 2^{math.log2(full):.2f}, off the quotient 2^{math.log2(float(off.max())):.2f}, residual 2^{math.log2(float(closed.max())):.2f}")
    assert qmax >= 1.0 and full >= bound and full <= 2.0 ** -20 * qmax and worst <= bound
    assert (off <= bound + np.abs(quotient) * closed[:, None] * (1 + 1e-9)).all()


def test_closed_form_in_float64():
    rng = np.random.default_rng(5)
    den = rng.uniform(dm.D_LO, dm.D_HI, (3, 64))
    num = rng.uniform(-1, 1, (3, 4, 64))
    for K in (1, 2, 4, 5):
        ns, ds = dm.float_iteration(num, den, K)
        want_d = 1.0 - (1.0 - den) ** (2 ** K)
        assert np.abs(ds[-1] - want_d).max() <= 64 * 2.0 ** -53                     # a few roundings per step, values of order one
        assert np.abs(ns[-1] - (num / den[:, None]) * want_d[:, None]).max() <= 64 * 2.0 ** -53 * (1 / dm.D_LO)
        assert np.abs(ns[-1] - num / den[:, None]).max() <= (1 / dm.D_LO) * dm.residual(dm.D_LO, dm.D_HI, K) + 64 * 2.0 ** -53
    assert dm.guess(0.5, 1.5) == 1.0 and dm.guess(1.0, 3.0) == 0.5
    assert dm.residual(1.0, 3.0, 0) == 0.5 and dm.residual(1.0, 3.0, 2) == 0.0625
    assert dm.residual(dm.D_LO, dm.D_HI, 5) == 0.4 ** 32 or abs(dm.residual(dm.D_LO, dm.D_HI, 5) / 0.4 ** 32 - 1) < 1e-12
    # a denominator range [lo, hi] under the constant guess lands on [1 - rho, 1 + rho]
    lo, hi = 3.0, 8.0
    c = dm.guess(lo, hi)
    assert abs(c * lo - (1 - (hi - lo) / (hi + lo))) < 1e-15 and abs(c * hi - (1 + (hi - lo) / (hi + lo))) < 1e-15


def test_scale_rule_against_exact_rationals():
    """sigma_n takes 2 roundings per step on top of twice the relative error it started from (the conversion of q_n is exact below 2^53 only: one more);
    nu_n takes 2 per step plus sigma's; kappa_n is llround of an exact doubling"""
    q = [int(v) for v in dm.run(8, 5, 2, 3, 405).data.moduli]
    drop = [q[-1 - n] for n in range(5)]
    u = Fraction(1, 2 ** 53)
    for den_scale in (float(q[-1]), float(q[-1]) * 1.003, 2.0 ** 59.9):
        sigma, nu, kappa = dm.step_scales(drop, dm.NUM_SCALE, den_scale)
        es, en = Fraction(den_scale), Fraction(dm.NUM_SCALE)
        rel_s = rel_n = Fraction(0)
        for n in range(5):
            assert kappa[n] == apm.llround(2.0 * sigma[n]) and abs(Fraction(kappa[n]) - 2 * Fraction(sigma[n])) <= Fraction(1, 2)
            en, es = en * es / drop[n], es * es / drop[n]
            step = (1 + u) ** 2 * (1 + 2 * u)              # the product's and the quotient's roundings, the conversion of q_n (in the divisor: 1 / (1 - u))
            rel_n, rel_s = (1 + rel_n) * (1 + rel_s) * step - 1, (1 + rel_s) ** 2 * step - 1
            assert abs(Fraction(sigma[n + 1]) / es - 1) <= rel_s and abs(Fraction(nu[n + 1]) / en - 1) <= rel_n
        assert rel_n < 2.0 ** -44 and rel_s < 2.0 ** -44
    # a mismatch sigma_0 / q = 1 + delta grows like (1 + delta)^(2^n)
    delta = 0.01
    sigma, _, _ = dm.step_scales(drop[:4], dm.NUM_SCALE, float(q[-1]) * (1 + delta))
    for n in range(5):
        assert abs(sigma[n] / float(q[-1]) / (1 + delta) ** (2 ** n) - 1) < 2.0 ** -20


def test_constructor_conditions_that_need_no_device():
    q = [int(v) for v in dm.run(8, 3, 2, 3, 403).data.moduli]
    drop, ns, qs = [q[-1 - n] for n in range(3)], dm.NUM_SCALE, float(q[-1])
    assert dm.invalid(drop, ns, qs) is None
    assert dm.invalid([], ns, qs) == "no steps"
    for bad in (0.0, -1.0, math.inf, math.nan):
        assert dm.invalid(drop, bad, qs) == dm.invalid(drop, ns, bad) == "scale not finite and positive"
    assert dm.invalid(drop[:1], ns, 2.0 ** 61) == "kappa reaches 2^62" and dm.invalid(drop[:1], ns, 2.0 ** 60.9) is None
    assert dm.invalid(drop[:1], ns, 2.0 ** 62) == "scale outside [2^20, 2^62)"
    assert dm.invalid(drop[:1], 2.0 ** 19, qs) == "scale outside [2^20, 2^62)" and dm.invalid(drop[:1], 2.0 ** 20, qs) is None
    assert dm.invalid(drop[:1], ns, 1.5 * qs) is None and dm.invalid(drop[:2], ns, 1.5 * qs) == "kappa reaches 2^62"
    assert dm.invalid(drop[:2], ns, qs / 64) is None and dm.invalid(drop, ns, qs / 64) == "scale outside [2^20, 2^62)"


def test_library_bound_equals_the_models_and_its_scale_conditions_hold():
    """no device: the facade's program prints each encrypted case's chain, magnitudes and static error_bound by their bits; the model's restatement gives the
    same number to a few roundings, and the program's own checks (the constructor's conditions through the static bound, guess, residual) pass"""
    out = subprocess.run([dm.build_api_test(), "ref"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("division reference OK"), out.stdout + out.stderr
    rows = re.findall(r"^case log2n (\d+) K (\d+) special (\d+) moduli ([\d ]+) args (.*) bound (\S+)$", out.stdout, re.M)
    assert [(int(r[0]), int(r[1])) for r in rows] == [(12, 3), (13, 4)], out.stdout
    for log2n, K, special, moduli, args, bound in rows:
        ns, ds, Dm, X, Bd, Bn = (float.fromhex(v) for v in args.split())
        q = [int(v) for v in moduli.split()]
        assert len(q) == int(K) + 2 and ds == float(q[-1])
        mine = dm.error_bound(int(log2n), q, [int(special)] * int(K), ns, ds, Dm, X, Bd, Bn)
        assert abs(mine / float.fromhex(bound) - 1) < 1e-12
    rows = re.findall(r"^steps (\d+): max\|n/D\| = ([0-9.]+) error_bound = 2\^(-?[0-9.]+)", out.stdout, re.M)
    assert len(rows) == 2 and all(float(qmax) >= 1.0 and float(b) <= -10.0 for _, qmax, b in rows), out.stdout
    assert subprocess.run([dm.build_api_test()], capture_output=True, text=True, timeout=120).returncode == 2


def test_model_rejects_planted_errors():
    r = dm.run(8, 3, 2, 3, 403)
    q = [int(v) for v in r.data.moduli]
    mu_n, mu_d = [[r.m_n[g, j] for j in range(3)] for g in range(2)], [r.m_d[g] for g in range(2)]
    again, sigma, nu, kappa = dm.model(q, 3, r.num_scale, r.den_scale, mu_n, mu_d)
    assert np.array_equal(again, r.words) and (sigma, nu, kappa) == (r.sigma, r.nu, r.kappa)
    # a scale rule that divides by 2^60 instead of the prime: other scales
    assert dm.step_scales([1 << 60] * 3, r.num_scale, r.den_scale)[0] != r.sigma
    # a constant off by 2^21 (2^-40 of itself) moves an output coefficient by about 2^21 mu / q = 2^11: other words.  (Off by one it moves them by 2^-10 of a
    # unit: numerators at 2^50 under 60-bit primes do not resolve that, and neither does the division.)
    real = dm.step_scales

    def off_by_a_little(drop, num_scale, den_scale):
        s, n, k = real(drop, num_scale, den_scale)
        return s, n, [v + (1 << 21) for v in k]
    dm.step_scales = off_by_a_little
    try:
        assert not np.array_equal(dm.model(q, 3, r.num_scale, r.den_scale, mu_n, mu_d)[0], r.words)
    finally:
        dm.step_scales = real
    # groups do not leak into each other: group 1 alone gives group 1's words
    alone = dm.model(q, 3, r.num_scale, r.den_scale, mu_n[1:], mu_d[1:])[0]
    assert np.array_equal(alone, r.words[3:])
