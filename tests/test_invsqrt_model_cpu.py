"""The exact integer model of ApproxInvSqrt on transparent inputs (tests/invsqrt_model.py), held on the CPU before the GPU test relies on it:
  - at N = 256 and N = 1024, K = 1 and 2 Newton steps, the model's output decodes to the float64 iteration y <- 1.5 y - 0.5 (v y)(y y) from the values encoded
    in every slot of every token within the header's bound evaluated with K_r = 0 (transparent inputs have no key-switch error) - derived, not measured;
    every case has min|Y_K| >= 1/2 and a bound <= 2^-20 of it;
  - the scales and weights are the rule's double operations, bit for bit, and the balanced guess scale keeps s_1 = s_0 to a rounding;
  - the iteration does what it is for: from a guess 10 % off, two steps are within 2e-3 of 1 / sqrt(v) (Newton's 1.5 e^2 twice);
  - the model has the resolution claimed: a weight off by one, or a scale rule that divides by 2^60 instead of the prime, changes words."""
import math

import numpy as np
import pytest

import approx_poly_model as apm
import invsqrt_model as ism

CASES = [(log2n, K) for log2n in (8, 10) for K in (1, 2)]


@pytest.mark.parametrize("log2n,K", CASES)
def test_model_decodes_to_the_float64_iteration_within_the_derived_bound(log2n, K):
    r = ism.run(log2n, K, 2, 900 + 10 * log2n + K)
    q = list(r.data.moduli)
    assert len(q) == 2 * K + 2 and r.words.shape == (2, 2, 2, 1 << log2n) and not r.words[:, 1].any()
    # the scale rule, spelled out for this chain, bit for bit
    s0 = r.guess_scale
    assert r.s[0] == s0 == math.sqrt((float(q[-1]) * float(q[-1])) * (float(q[-2]) / (2.0 * ism.V_SCALE)))
    s_a, s_b = (ism.V_SCALE * s0) / float(q[-1]), (s0 * s0) / float(q[-1])
    top = 2.0 * (s_a * s_b)
    assert r.w[0] == apm.llround(1.5 * (top / s0)) and r.s[1] == top / float(q[-2])
    if K == 2:
        s1 = r.s[1]
        top1 = 2.0 * (((ism.V_SCALE * s1) / float(q[-3])) * ((s1 * s1) / float(q[-3])))
        assert r.w[1] == apm.llround(1.5 * (top1 / s1)) and r.s[2] == top1 / float(q[-4])
    assert all(abs(w) < 2 ** 62 for w in r.w) and all(ism.SCALE_MIN <= s < ism.SCALE_MAX for s in r.s)
    assert all(abs(s / s0 - 1) < 2.0 ** -20 for s in r.s)                       # balanced: every s_n stays at s_0 (the primes differ by less than 2^-20)
    V, Y = r.magnitudes()
    Bv, By = r.noise_bounds()
    bound = ism.error_bound(log2n, q, [r.special] * (2 * K), ism.V_SCALE, s0, V, Y, Bv, By, keyswitch=False)
    full = ism.error_bound(log2n, q, [r.special] * (2 * K), ism.V_SCALE, s0, V, Y, Bv, By)
    z = r.decoded()
    worst = max(float(np.abs(z.real - r.want).max()), float(np.abs(z.imag).max()))
    ymin = float(np.abs(r.want).min())
    print(f"{r.case.name}: min|Y_K| {ymin:.3f}, max error 2^{math.log2(max(worst, 1e-300)):.2f}, bound (K_r = 0) 2^{math.log2(bound):.2f}, "
          f"with key switches 2^{math.log2(full):.2f}")
    assert ymin >= 0.5 and full >= bound and full <= 2.0 ** -20 * ymin and worst <= bound


def test_two_steps_take_a_ten_percent_guess_to_two_in_a_thousand():
    r = ism.run(8, 2, 2, 982)
    rel = [float(np.abs(y * np.sqrt(r.v) - 1).max()) for y in r.iterates]
    assert 0.05 < rel[0] <= ism.GUESS_OFF + 1e-12 and rel[1] <= 1.6 * rel[0] ** 2 + rel[0] ** 3 and rel[2] <= 2e-3


def test_unbalanced_guess_scale_drifts_cubically():
    q = list(ism.run(8, 2, 2, 982).data.moduli)
    drop = [q[-1 - r] for r in range(4)]
    s0 = ism.balanced_guess_scale(ism.V_SCALE, q[-1], q[-2])
    s, _ = ism.step_scales(drop, ism.V_SCALE, 2.0 * s0)
    assert abs(s[1] / s0 / 8.0 - 1) < 2.0 ** -20 and abs(s[2] / s0 / 512.0 - 1) < 2.0 ** -18     # c = 2: c^3, c^9


def test_model_rejects_planted_errors():
    r = ism.run(8, 2, 2, 982)
    q = list(r.data.moduli)
    mu_v, mu_y = [r.m_v[t] for t in range(2)], [r.m_y[t] for t in range(2)]
    again, s, w = ism.model(q, 2, ism.V_SCALE, r.guess_scale, mu_v, mu_y)
    assert np.array_equal(again, r.words) and s == r.s and w == r.w
    # a guess scale one ulp up: other weights or other scales
    s2, steps2 = ism.step_scales([q[-1 - i] for i in range(4)], ism.V_SCALE, math.nextafter(r.guess_scale, math.inf))
    assert s2 != r.s
    # a scale rule that divides by 2^60 instead of the prime: another weight
    _, steps = ism.step_scales([1 << 60] * 4, ism.V_SCALE, r.guess_scale)
    assert [st[3] for st in steps] != r.w
    # a weight off by one moves every output coefficient by about mu / q_b: other words
    real = ism.step_scales

    def off_by_one(drop, v_scale, guess_scale):
        s, steps = real(drop, v_scale, guess_scale)
        return s, [(a, b, t, wn + 1) for a, b, t, wn in steps]
    ism.step_scales = off_by_one
    try:
        assert not np.array_equal(ism.model(q, 2, ism.V_SCALE, r.guess_scale, mu_v, mu_y)[0], r.words)
    finally:
        ism.step_scales = real
