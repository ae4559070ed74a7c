"""The exact integer model of ApproxPolynomial on a transparent input (tests/approx_poly_model.py), held on the CPU before the GPU test relies on it:
  - at N = 256, d = 2, 3, 4, 7 the model's output decodes to the float64 p(x) in every slot of every token within the header's bound evaluated with K = 0
    (a transparent input has no key-switch error) - derived, not measured; every case has a bound <= 2^-20 against max|p(x)| >= 1;
  - llround rounds halves away from zero; the scale rule and the weights are the stated double operations; the Kronecker product is the schoolbook one;
  - the model has the resolution claimed: one coefficient off by 2^-30 relative, or a scale rule that divides by 2^60 instead of q, changes words."""
import math

import numpy as np
import pytest

import approx_layer_model as alm
import approx_poly_model as apm

DEGREES = (2, 3, 4, 7)


def test_llround_rounds_halves_away_from_zero():
    assert [apm.llround(v) for v in (0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999999999999994, -0.49999999999999994, 2.0 ** 61 + 512.0)] == \
        [1, 2, 3, -1, -2, -3, 0, 0, 2 ** 61 + 512]
    assert round(0.5) == 0 and round(2.5) == 2          # what Python's round would have done


def test_negacyclic_product_is_the_schoolbook_one():
    rng = np.random.default_rng(1)
    N = 16
    a = np.array([int(v) << 40 for v in rng.integers(-2 ** 62, 2 ** 62, N)], dtype=object)
    b = np.array([int(v) for v in rng.integers(-2 ** 62, 2 ** 62, N)], dtype=object)
    want = [0] * N
    for i in range(N):
        for j in range(N):
            k = i + j
            want[k % N] += int(a[i]) * int(b[j]) * (1 if k < N else -1)
    assert [int(v) for v in apm.negacyclic(a, b)] == want


@pytest.mark.parametrize("d", DEGREES)
def test_model_decodes_to_the_float64_polynomial_within_the_derived_bound(d):
    r = apm.run(8, d, 2, 300 + d)
    case = r.case
    rstar = apm.ceil_log2(d)
    assert len(r.data.moduli) == rstar + 2 and r.words.shape == (2, 2, 1, 256) and not r.words[:, 1].any()
    # the scale rule, spelled out for this chain
    q = r.data.moduli
    assert r.s[1] == apm.INPUT_SCALE and r.s[2] == (r.s[1] * r.s[1]) / float(q[-1])
    if d >= 3:
        assert r.s[3] == (r.s[2] * r.s[1]) / float(q[-2])
    if d >= 7:
        assert r.s[7] == (r.s[4] * r.s[3]) / float(q[-3])
    top = apm.OUTPUT_SCALE * float(q[-1 - rstar])
    assert r.c[0] == apm.llround(r.coeffs[0] * apm.OUTPUT_SCALE) * q[-1 - rstar] and r.c[d] == apm.llround(r.coeffs[d] * (top / r.s[d]))
    assert all(abs(c) < 2 ** 62 for c in r.c[1:]) and abs(r.c[0]) // q[-1 - rstar] < 2 ** 62
    Bin = alm.fresh_noise_bound(case.log2n, apm.INPUT_SCALE, apm.X_MAX, 1)
    bound = apm.error_bound(case.log2n, list(q), [r.special] * rstar, r.coeffs, apm.INPUT_SCALE, apm.OUTPUT_SCALE, apm.X_MAX, Bin, keyswitch=False)
    z = r.decoded()
    worst = max(float(np.abs(z.real - r.want).max()), float(np.abs(z.imag).max()))
    pmax = float(np.abs(r.want).max())
    print(f"{case.name}: max|p(x)| {pmax:.3f}, max error 2^{math.log2(max(worst, 1e-300)):.2f}, bound (K = 0) 2^{math.log2(bound):.2f}, "
          f"with key switches 2^{math.log2(apm.error_bound(case.log2n, list(q), [r.special] * rstar, r.coeffs, apm.INPUT_SCALE, apm.OUTPUT_SCALE, apm.X_MAX, Bin)):.2f}")
    assert pmax >= 1.0 and bound <= 2.0 ** -20 and worst <= bound


def test_model_rejects_planted_errors():
    r = apm.run(8, 4, 2, 304)
    mus = [r.m[t] for t in range(2)]
    mods = list(r.data.moduli)
    off = list(r.coeffs)
    off[3] *= 1.0 + 2.0 ** -30
    assert not np.array_equal(apm.model(mods, off, apm.INPUT_SCALE, apm.OUTPUT_SCALE, mus)[0], r.words)
    # a scale rule that divides by 2^60 instead of the prime: other weights, other words
    s = apm.power_scales(4, apm.INPUT_SCALE, [1 << 60, 1 << 60])
    assert s != r.s and apm.weights(r.coeffs, s, apm.OUTPUT_SCALE, mods[-3]) != r.c
    assert np.array_equal(apm.model(mods, r.coeffs, apm.INPUT_SCALE, apm.OUTPUT_SCALE, mus)[0], r.words)
