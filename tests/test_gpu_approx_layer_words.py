"""-m gpu: ApproxPackedLinear on a TRANSPARENT input gives the words of the exact integer model, every word of every item, limb and component.

A ciphertext (c0, 0) makes every key-switch digit zero and every division by P exact, so the layer is a deterministic integer function of c0, W, b and
the scales; tests/approx_layer_model.py states that function and tests/test_approx_layer_model_cpu.py holds the model to the
float64 layer within 2^-20.  Here tests/cpp/approx_layer_words.cpp runs the layer (one process per case) and every case asserts: the output words equal
the model's; the c1 words are all zero; output_scale() equals the model's double bit for bit; and the geometry the layer reports - the split, dim(),
input_period(), output_ciphertexts(), row_of_slot() of every slot - is the model's (the program has no device-free mode: the geometry lives in the layer
object, whose constructor allocates on the device).

This test sees what the encrypted one (tests/test_gpu_approx_linear.py) cannot - a weight narrowed to float32, a bias at a slightly wrong scale, a
rounding rule - because it has no noise to allow for; it cannot see the key-switch terms or the c1 path, which are zero here and which the encrypted
test catches at the order of max|y|.  The two are complementary.

Without a GPU: the program links."""
import re
import subprocess
import time

import numpy as np
import pytest

import approx_layer_model as alm

IDS = [c.name for c in alm.CASES]


def test_program_links_and_rejects_a_missing_case_file(tmp_path):
    out = subprocess.run([alm.build_words_program(), str(tmp_path / "none"), str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "cannot read" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("case", alm.CASES, ids=IDS)
def test_layer_words_equal_the_integer_model(case, tmp_path):
    t0 = time.time()
    run = alm.Run(case)
    t_model = time.time() - t0
    case_file, out_file = str(tmp_path / "case.bin"), str(tmp_path / "words.bin")
    run.write_case_file(case_file)
    t0 = time.time()
    out = subprocess.run([alm.build_words_program(), case_file, out_file], capture_output=True, text=True, timeout=300 if case.log2n >= 15 else 120)
    t_device = time.time() - t0
    assert out.returncode == 0 and out.stdout.strip().endswith("approximate layer words written"), out.stdout[-4000:] + out.stderr[-2000:]
    lines = re.findall(r"^layer (\d+) passes (\d+) n1 (\d+) n2 (\d+) dim (\d+) input_period (\d+) output_scale (\S+) rows(.*)$", out.stdout, re.M)
    assert len(lines) == len(case.layers), out.stdout[-2000:]
    for k, (geo, line) in enumerate(zip(run.geos, lines)):
        assert [int(v) for v in line[:6]] == [k, geo.passes, geo.n1, geo.n2, geo.m, geo.n], (case.name, line[:6])
        assert float.fromhex(line[6]) == run.scales[k + 1], (case.name, line[6], run.scales[k + 1].hex())       # bit for bit
        assert np.array_equal(np.array(line[7].split(), dtype=np.int64).reshape(geo.passes, geo.row), geo.rows()), (case.name, "row_of_slot")
    want = run.words[-1]
    got = np.fromfile(out_file, dtype="<u8")
    assert got.size == want.size, (case.name, got.size, want.size)
    got = got.reshape(want.shape)
    geo = run.geos[-1]
    print(f"{case.name}: n1 x n2 = {geo.n1} x {geo.n2}, passes {geo.passes}, {want.size} words compared, model {run.case.model} {t_model:.2f} s, "
          f"program {t_device:.2f} s")
    assert not got[:, 1].any(), (case.name, "c1 words are not all zero")
    differ = np.argwhere(got[:, 0] != want[:, 0])
    assert differ.size == 0, (case.name, f"{len(differ)} of {want[:, 0].size} c0 words differ; first (item, limb, coefficient) {differ[0].tolist()}")
