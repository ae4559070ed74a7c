"""The Newton step and the inverse square root in the C++ facade (ScalarWeights, HybridKeySwitcher::multiply_lincomb_rescale_range, ApproxInvSqrt): builds
tests/cpp/newton/test_invsqrt_api.cpp and, -m gpu, runs it - on encrypted inputs at N = 4096, one and two Newton steps, three tokens: every decoded slot within the
stated error_bound of the float64 iteration from the values encrypted; one fused product + term + constant within the bound of its own recurrence, and equal
to multiply_rescale word for word without terms; both calls behind the stream gate; the rejections.  Without a GPU: the program links, and its `ref` mode (no
device) shows that every drawn case has min|Y_K| >= 1/2 and error_bound <= 2^-10 min|Y_K|, so the tolerance cannot hide an error of the order of the output."""
import math
import re
import subprocess

import pytest

import invsqrt_model as ism
import stream_gate as sg


def test_program_links_and_its_cases_have_outputs_of_order_one_and_a_tight_bound():
    out = subprocess.run([ism.build_api_test(), "ref"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = re.findall(r"^steps (\d+): min\|Y_K\| = ([0-9.]+) error_bound = 2\^(-?[0-9.]+)", out.stdout, re.M)
    assert [int(r[0]) for r in rows] == [1, 2], out.stdout
    for _, ymin, log2_bound in rows:
        assert float(ymin) >= 0.5 and float(log2_bound) <= -10.0 + math.log2(float(ymin)), out.stdout


@pytest.mark.gpu
def test_cpp_inverse_square_root_facade():
    out = subprocess.run([ism.build_api_test(), str(sg.GATE_SECONDS)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("inverse square root C++ facade OK"), out.stdout[-4000:] + out.stderr[-2000:]
    assert len(re.findall(r"error_bound 2\^-", out.stdout)) == 2 and len(re.findall(r"behind the gate", out.stdout)) == 2
