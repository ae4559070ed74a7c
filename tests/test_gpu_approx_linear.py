"""The approximate packed layer of the C++ facade (ApproxPackedLinear, Evaluator::add_plain / sub_plain): builds tests/cpp/test_approx_linear_api.cpp and,
-m gpu, runs it - every shape's unpacked outputs within the layer's stated error_bound of the float64 W x + b, with and without bias, one and two
tokens per ciphertext, one and two output ciphertexts; the stream contract of apply(); the constructor's rejections.  Without a GPU: the program links,
and the cases it draws have max|y| >= 1 (its `ref` mode touches no device), so the tolerance cannot hide an error of the order of the outputs."""
import re
import subprocess

import pytest

import cpp_build
import stream_gate as sg


def build_approx_linear_test():
    return cpp_build.build_program("test_approx_linear_api", gate=True)


def test_program_links_and_its_cases_have_outputs_of_order_one():
    out = subprocess.run([build_approx_linear_test(), "ref"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    ymax = [float(v) for v in re.findall(r"max\|y\| = ([0-9.]+)", out.stdout)]
    assert len(ymax) == 8 and min(ymax) >= 1.0, out.stdout      # four shapes, with and without bias


@pytest.mark.gpu
def test_cpp_approx_linear_facade():
    out = subprocess.run([build_approx_linear_test(), str(sg.GATE_SECONDS)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("approximate packed layer C++ facade OK"), out.stdout[-4000:] + out.stderr[-2000:]
    assert len(re.findall(r"error_bound 2\^-", out.stdout)) == 8
