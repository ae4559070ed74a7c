"""-m gpu: ApproxPolynomial on a TRANSPARENT input gives the words of the exact integer model, every word of every token, limb and component.

A ciphertext (c0, 0) makes every relinearisation digit zero and every division by P exact, so the polynomial is a deterministic integer function of c0,
the coefficients and the scales; tests/approx_poly_model.py states that function and tests/test_approx_poly_model_cpu.py holds the model to the float64
p(x).  Here tests/cpp/approx_poly_words.cpp runs the polynomial at N = 4096 (one process per case: degrees 2, 3, 4, 7, one and three tokens) and every case
asserts: the output words equal the model's; the c1 words are all zero; every s_k equals the model's double bit for bit; every weight is the model's.

This test sees what the encrypted one (tests/test_gpu_approx_poly.py) cannot - a wrong scalar, a wrong scale rule, a rounding rule - because it has no
noise to allow for; it cannot see the relinearisation, which is zero here and which the encrypted test and tests/test_gpu_fused_rescale.py carry.

Without a GPU: the program links."""
import re
import subprocess

import numpy as np
import pytest

import approx_poly_model as apm

CASES = [(d, T) for d in (2, 3, 4, 7) for T in (1, 3)]


def test_program_links_and_rejects_a_missing_case_file(tmp_path):
    out = subprocess.run([apm.build_words_program(), str(tmp_path / "none"), str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "cannot read" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("d,T", CASES, ids=[f"d{d}_T{T}" for d, T in CASES])
def test_polynomial_words_equal_the_integer_model(d, T, tmp_path):
    run = apm.run(12, d, 3, 500 + d)            # one model per degree; the one-token case is its first token
    case_file, out_file = str(tmp_path / "case.bin"), str(tmp_path / "words.bin")
    run.write_case_file(case_file, tokens=T)
    out = subprocess.run([apm.build_words_program(), case_file, out_file], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("approximate polynomial words written"), out.stdout[-4000:] + out.stderr[-2000:]
    line = re.search(r"^degree (\d+) depth (\d+) scales (.*) weights (.*)$", out.stdout, re.M)
    assert line and int(line.group(1)) == d and int(line.group(2)) == apm.ceil_log2(d) + 1, out.stdout[-2000:]
    assert [float.fromhex(v) for v in line.group(3).split()] == run.s[1:]                       # bit for bit
    q_star = run.data.moduli[len(run.data.moduli) - 1 - apm.ceil_log2(d)]
    assert [int(v) for v in line.group(4).split()] == [run.c[0] // q_star] + run.c[1:] and run.c[0] % q_star == 0
    want = run.words[:T]
    got = np.fromfile(out_file, dtype="<u8")
    assert got.size == want.size, (got.size, want.size)
    got = got.reshape(want.shape)
    assert not got[:, 1].any(), "c1 words are not all zero"
    differ = np.argwhere(got[:, 0] != want[:, 0])
    assert differ.size == 0, f"{len(differ)} of {want[:, 0].size} c0 words differ; first (token, limb, coefficient) {differ[0].tolist()}"
