"""The exact integer model of ApproxPackedLinear on a transparent input (tests/approx_layer_model.py), held on the CPU before the GPU test relies on it:
  - model A (big integers) and model B (the oracle, limb by limb) give equal words on every small-ring case - which licenses model B at N = 32768;
  - model A's output decodes to the float64 W x + b at every slot that holds a row, every token, both parts with two tokens per ciphertext, within the
    header's bound evaluated with K = 0 (a transparent input has no key-switch error) - derived, not measured; every case has a bound <= 2^-20 against
    max|y| >= 1;
  - the geometry gives the blocks, folds and output ciphertexts each case of the table is there for;
  - both models have the resolution claimed: one weight off by 2^-30 relative, or the bias encoded at Dx Dw / 2^60 instead of / q_last, changes words.
The agreement of the geometry with the library's row_of_slot(), output_ciphertexts(), dim() and input_period() is asserted in
tests/test_gpu_approx_layer_words.py: those live in the layer object, whose constructor allocates on the device.
"""
import functools
import math

import numpy as np
import pytest

import approx_layer_model as alm

IDS = [c.name for c in alm.SMALL]


@functools.lru_cache(maxsize=None)
def run_a(name):
    return alm.Run(next(c for c in alm.SMALL if c.name == name), "A")


@pytest.mark.parametrize("case", alm.SMALL, ids=IDS)
def test_big_integer_and_oracle_models_give_equal_words(case):
    a, b = run_a(case.name), alm.Run(case, "B")
    for k in range(len(case.layers)):
        assert a.words[k].shape == b.words[k].shape and np.array_equal(a.words[k], b.words[k]), (case.name, k)
        assert not a.words[k][:, 1].any() and a.words[k][:, 0].any()
        assert a.scales[k + 1] == b.scales[k + 1]


@pytest.mark.parametrize("case", alm.SMALL, ids=IDS)
def test_model_decodes_to_the_float64_layer_within_the_derived_bound(case):
    r = run_a(case.name)
    moduli = list(r.data.moduli)
    y = r.x                                   # [T * tpc][in_dim]: the float64 reference, layer after layer
    X, Bin = 1.0, alm.fresh_noise_bound(case.log2n, case.input_scale, 1.0, case.tpc)
    for k, (l, geo, W, b) in enumerate(zip(case.layers, r.geos, r.Ws, r.bs)):
        y = y @ W.T + (b if b is not None else 0.0)
        bound = alm.error_bound(case.log2n, geo, W, b, r.scales[k], l.weight_scale, moduli[-1 - k], case.tpc, X, Bin)
        z, rows = r.decoded(k), geo.rows()
        worst, checked = 0.0, 0
        for o in range(geo.passes):
            held = rows[o] >= 0
            for t in range(case.T):
                v = z[o * case.T + t][held]
                worst = max(worst, float(np.abs(v.real - y[t * case.tpc][rows[o][held]]).max()))
                if case.tpc == 2:
                    worst = max(worst, float(np.abs(v.imag - y[t * case.tpc + 1][rows[o][held]]).max()))
                else:
                    worst = max(worst, float(np.abs(v.imag).max()))       # one token: the imaginary parts decode to zero
                checked += int(held.sum()) * case.tpc
        ymax = float(np.abs(y).max())
        print(f"{case.name} layer {k}: n1 x n2 = {geo.n1} x {geo.n2}, passes {geo.passes}, max|y| {ymax:.3f}, "
              f"max error 2^{math.log2(max(worst, 1e-300)):.2f}, bound 2^{math.log2(bound):.2f} ({checked} slots)")
        assert set(rows[rows >= 0].tolist()) == set(range(l.out_dim))          # every row is held somewhere
        assert checked >= l.out_dim * case.T * case.tpc
        assert bound <= 2.0 ** -20
        assert ymax >= 1.0
        assert worst <= bound
        # the next layer's input: its slots are off y by at most `bound` in units of this layer's output.  The header's S = N Bin is its bound on
        # a baby step's SLOT error from a coefficient bound; here the slot error is known directly, so Bin = Do bound / N gives S = Do bound.
        X, Bin = ymax + bound, r.scales[k + 1] * bound / (1 << case.log2n)


def test_geometry_of_the_table():
    g = {c.name: alm.Geometry(c.log2n, c.layers[0].out_dim, c.layers[0].in_dim, c.layers[0].n1, c.layers[0].n2) for c in alm.CASES}
    facts = lambda q: (q.n, q.m, q.blocks, q.passes, len(q.folds), q.n2)
    assert facts(g["n10_2x2_bias"]) == (2, 2, 1, 1, 0, 1)                 # m = 2, no giant step: the copy path
    assert facts(g["n10_1x3_bias"]) == (4, 2, 1, 1, 1, 1)                 # n2 = 1 with one fold rotation
    assert facts(g["n10_16x16_bias"]) == (16, 16, 1, 1, 0, 2)             # one replicated block
    assert facts(g["n10_77x24_bias"]) == (32, 32, 3, 1, 0, 2)             # ragged rows, three blocks in one pass
    assert facts(g["n10_12x100_pair_bias"]) == (128, 16, 1, 1, 3, 2)      # wide input, three fold steps
    assert facts(g["n10_600x200_bias"]) == (256, 256, 3, 2, 0, 8)         # two output ciphertexts
    assert facts(g["n15_16x16_pair_bias"]) == (16, 16, 1, 1, 0, 2)
    q = g["n10_77x24_bias"]
    assert q.row_of_slot(0, 0) == 0 and q.row_of_slot(0, 32 + 5) == 37 and q.row_of_slot(0, 64 + 12) == 76 and q.row_of_slot(0, 64 + 13) == -1
    assert q.row_of_slot(0, 96) == -1                                      # a window past the last block
    q = g["n10_600x200_bias"]
    assert q.row_of_slot(0, 256 + 1) == 257 and q.row_of_slot(1, 87) == 599 and q.row_of_slot(1, 88) == -1 and q.row_of_slot(1, 256) == -1
    # the rescaling prime of the mixed chain sits near the weight scale, so the output scale stays near the input scale
    c = next(c for c in alm.CASES if c.chain == "mixed45")
    data, special, _ = c.params()
    assert 2 ** 44 < data.moduli[-1] < 2 ** 45 and all(q > 2 ** 59 for q in data.moduli[:-1] + (special,))
    assert 0.99 < alm.output_scale(c.input_scale, c.layers[0].weight_scale, data.moduli[-1]) / c.input_scale < 1.01


PLANTED = ["n10_16x16_bias", "n10_12x100_pair_bias"]


@pytest.mark.parametrize("name", PLANTED)
@pytest.mark.parametrize("model", ["A", "B"])
def test_models_reject_planted_errors_in_their_inputs(name, model):
    case = next(c for c in alm.SMALL if c.name == name)
    clean = run_a(name).words[0]
    l = case.layers[0]
    off = alm.Run(case, model, perturb=("weight", 0, l.out_dim - 1, l.in_dim // 2, 1.0 + 2.0 ** -30)).words[0]
    assert off.shape == clean.shape and not np.array_equal(off, clean)
    bias = alm.Run(case, model, perturb=("bias_scale_2_60", 0)).words[0]
    assert bias.shape == clean.shape and not np.array_equal(bias, clean)
    assert np.array_equal(alm.Run(case, model).words[0], clean)                # ... and the unperturbed run of the same model gives the words again
