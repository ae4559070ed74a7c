"""The Goldschmidt step and the division in the C++ facade (ComplementConstant, HybridKeySwitcher::multiply_complement_rescale_range, ApproxDivide): builds
tests/cpp/divide/test_divide_api.cpp and, -m gpu, runs it - on encrypted inputs at N = 4096 with K = 3 and N = 8192 with K = 4, on 60-bit fold primes with the
special prime, 2 groups of 3 numerators: every decoded slot within the stated error_bound of the float64 iteration from the values encrypted, the bound below the
largest quotient, every slot within error_bound + |n / D| (1 - D_0)^(2^K) of the true quotient; one step word for word against negate, add_plain and
multiply_rescale_range; the step and apply behind the stream gate (Gate::gated of tests/cpp/facade_test.h); the rejections.  Without a GPU: the program links
(tests/test_divide_model_cpu.py runs its `ref` mode)."""
import re
import subprocess

import pytest

import divide_model as dm
import stream_gate as sg


def test_program_links_and_prints_its_usage():
    out = subprocess.run([dm.build_api_test(), "run"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "usage" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("log2n,K", [(12, 3), (13, 4)])
def test_cpp_division_facade(log2n, K):
    out = subprocess.run([dm.build_api_test(), "run", str(log2n), str(K), str(sg.GATE_SECONDS)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("division C++ facade OK"), out.stdout[-4000:] + out.stderr[-2000:]
    m = re.search(r"max\|n/D\| ([0-9.]+), max error 2\^(-?[0-9.]+), error_bound 2\^(-?[0-9.]+)", out.stdout)
    assert m and float(m.group(1)) >= 1.0 and float(m.group(2)) <= float(m.group(3)) <= -10.0, out.stdout
    assert len(re.findall(r"behind the gate", out.stdout)) == 2
