"""The approximate family's activations in the C++ facade (HybridKeySwitcher::multiply_rescale, ApproxPolynomial): builds tests/cpp/test_approx_poly_api.cpp
and, -m gpu, runs it - on encrypted inputs at N = 4096, degrees 2, 3, 4 and 7, three tokens: every decoded slot within the stated error_bound of the
float64 p(x); one product within the bound of its own recurrence; both calls behind the stream gate; the rejections.  Without a GPU: the program links,
and its `ref` mode (no device) shows that every drawn case has max|p(x)| >= 1 and error_bound <= 2^-10 max|p(x)|, so the tolerance cannot hide an error of
the order of the outputs."""
import math
import re
import subprocess

import pytest

import approx_poly_model as apm
import stream_gate as sg


def test_program_links_and_its_cases_have_outputs_of_order_one_and_a_tight_bound():
    out = subprocess.run([apm.build_api_test(), "ref"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = re.findall(r"^degree (\d+): max\|p\(x\)\| = ([0-9.]+) error_bound = 2\^(-?[0-9.]+)", out.stdout, re.M)
    assert [int(r[0]) for r in rows] == [2, 3, 4, 7], out.stdout
    for _, pmax, log2_bound in rows:
        assert float(pmax) >= 1.0 and float(log2_bound) <= -10.0 + math.log2(float(pmax)), out.stdout


@pytest.mark.gpu
def test_cpp_approx_polynomial_facade():
    out = subprocess.run([apm.build_api_test(), str(sg.GATE_SECONDS)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("approximate polynomial C++ facade OK"), out.stdout[-4000:] + out.stderr[-2000:]
    assert len(re.findall(r"error_bound 2\^-", out.stdout)) == 4 and len(re.findall(r"behind the gate", out.stdout)) == 2
