"""-m gpu: ApproxInvSqrt on TRANSPARENT inputs gives the words of the exact integer model, every word of every token, limb and component.

Ciphertexts (c0, 0) make every relinearisation digit zero and every division by P exact, so the Newton steps are a deterministic integer function of the two
input polynomials and the scales; tests/invsqrt_model.py states that function and tests/test_invsqrt_model_cpu.py holds the model to the float64 iteration.
Here tests/cpp/newton/invsqrt_words.cpp runs the steps at N = 1024 (one process per case: K = 1 and 2, one and three tokens) and every case asserts: the output words
equal the model's; the c1 words are all zero; every s_n equals the model's double bit for bit; every weight is the model's.

This test sees what the encrypted one (tests/test_gpu_invsqrt.py) cannot - a wrong weight, a term read at the wrong level or stride, a wrong scale rule, a
rounding rule - because it has no noise to allow for; it cannot see the relinearisation, which is zero here and which the encrypted test and
tests/test_gpu_relin_lincomb.py carry.

Without a GPU: the program links."""
import re
import subprocess

import numpy as np
import pytest

import invsqrt_model as ism

CASES = [(K, T) for K in (1, 2) for T in (1, 3)]


def test_program_links_and_rejects_a_missing_case_file(tmp_path):
    out = subprocess.run([ism.build_words_program(), str(tmp_path / "none"), str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "cannot read" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("K,T", CASES, ids=[f"K{K}_T{T}" for K, T in CASES])
def test_newton_words_equal_the_integer_model(K, T, tmp_path):
    run = ism.run(10, K, 3, 700 + K)            # one model per K; the one-token case is its first token
    case_file, out_file = str(tmp_path / "case.bin"), str(tmp_path / "words.bin")
    run.write_case_file(case_file, tokens=T)
    out = subprocess.run([ism.build_words_program(), case_file, out_file], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("inverse square root words written"), out.stdout[-4000:] + out.stderr[-2000:]
    line = re.search(r"^iterations (\d+) depth (\d+) scales (.*) weights (.*)$", out.stdout, re.M)
    assert line and int(line.group(1)) == K and int(line.group(2)) == 2 * K, out.stdout[-2000:]
    assert [float.fromhex(v) for v in line.group(3).split()] == run.s                            # bit for bit
    assert [int(v) for v in line.group(4).split()] == run.w
    want = run.words[:T]
    got = np.fromfile(out_file, dtype="<u8")
    assert got.size == want.size, (got.size, want.size)
    got = got.reshape(want.shape)
    assert not got[:, 1].any(), "c1 words are not all zero"
    differ = np.argwhere(got[:, 0] != want[:, 0])
    assert differ.size == 0, f"{len(differ)} of {want[:, 0].size} c0 words differ; first (token, limb, coefficient) {differ[0].tolist()}"
