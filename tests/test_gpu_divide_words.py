"""-m gpu: ApproxDivide on TRANSPARENT inputs gives the words of the exact integer model, every word of every numerator, limb and component.

Ciphertexts (c0, 0) make every relinearisation digit zero and every division by P exact, so the Goldschmidt steps are a deterministic integer function of the
input polynomials and the scales; tests/divide_model.py states that function and tests/test_divide_model_cpu.py holds the model to the float64 iteration.
Here tests/cpp/divide/divide_words.cpp runs the steps at N = 256 and N = 4096 (one process per case: K = 1, 2 and 4; G x T = 1 x 1, 2 x 3 and 3 x 5) and once
on a mixed-class context (f64 data limbs under a fold special prime, one step), and every case asserts: the output words equal the model's; the c1 words are
all zero; every sigma_n and nu_n equals the model's double bit for bit; every kappa_n is the model's.

This test sees what the encrypted one (tests/test_gpu_divide.py) cannot - a wrong constant, a numerator multiplied by another group's factor, the self product in
the wrong place or at the wrong level, a wrong scale rule, a rounding rule - because it has no noise to allow for; it cannot see the relinearisation, which is
zero here and which the encrypted test carries.

Without a GPU: the program links."""
import re
import subprocess

import numpy as np
import pytest

import class_edges
import divide_model as dm

CASES = [(8, 1, 1, 1), (8, 2, 2, 3), (8, 4, 3, 5), (12, 1, 2, 3), (12, 2, 3, 5), (12, 4, 1, 1)]


def check(run, tmp_path):
    c = run.case
    case_file, out_file = str(tmp_path / "case.bin"), str(tmp_path / "words.bin")
    run.write_case_file(case_file)
    out = subprocess.run([dm.build_words_program(), case_file, out_file], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("division words written"), out.stdout[-4000:] + out.stderr[-2000:]
    line = re.search(r"^iterations (\d+) depth (\d+) den_scales (.*) num_scales (.*) kappas (.*)$", out.stdout, re.M)
    assert line and int(line.group(1)) == c.K and int(line.group(2)) == c.K, out.stdout[-2000:]
    assert [float.fromhex(v) for v in line.group(3).split()] == run.sigma                        # bit for bit
    assert [float.fromhex(v) for v in line.group(4).split()] == run.nu
    assert [int(v) for v in line.group(5).split()] == run.kappa
    want = run.words
    got = np.fromfile(out_file, dtype="<u8")
    assert got.size == want.size, (got.size, want.size)
    got = got.reshape(want.shape)
    assert not got[:, 1].any(), "c1 words are not all zero"
    differ = np.argwhere(got[:, 0] != want[:, 0])
    assert differ.size == 0, f"{len(differ)} of {want[:, 0].size} c0 words differ; first (item, limb, coefficient) {differ[0].tolist()}"


def test_program_links_and_rejects_a_missing_case_file(tmp_path):
    out = subprocess.run([dm.build_words_program(), str(tmp_path / "none"), str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "cannot read" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("log2n,K,G,T", CASES, ids=[f"n{1 << ln}_K{K}_{G}x{T}" for ln, K, G, T in CASES])
def test_goldschmidt_words_equal_the_integer_model(log2n, K, G, T, tmp_path):
    check(dm.run(log2n, K, G, T, 600 + 10 * log2n + K), tmp_path)


@pytest.mark.gpu
def test_goldschmidt_words_on_the_mixed_class_context(tmp_path):
    """three f64 data limbs (47 bits) under a fold special prime: one step, the denominator at the dropped prime's size, the numerators at 2^30"""
    p = class_edges.edge_moduli("f64_under_fold", 10)
    assert p.n_limbs == 4
    check(dm.Run(dm.Case(10, 1, 2, 3, 640, params=p, num_scale=2.0 ** 30)), tmp_path)
