"""The all-pairs product step in the C++ facade (HybridKeySwitcher::multiply_outer_rescale_range): builds tests/cpp/attention/test_outer_api.cpp and, -m gpu, runs
it - on encrypted inputs at N = 1024 and N = 4096 on 60-bit fold primes with the special prime, 5 queries against 6 keys and 5 x 5 causal: word for word
multiply_rescale_range on the pair lists copied out item by item, ranges that do not start at 0, one buffer for both operands, every pair decrypting to the
product of what was encrypted; the step behind the stream gate (Gate::gated of tests/cpp/facade_test.h); the rejections.  Without a GPU: the program links."""
import os
import re
import subprocess

import pytest

import cpp_build
import stream_gate as sg


def build_api_test():
    """tests/cpp/attention/test_outer_api.cpp -> tests/cpp/bin/attention/test_outer_api (tests/cpp_build.py makes tests/cpp/bin but no directory below it)"""
    os.makedirs(os.path.join(cpp_build.BIN_DIR, "attention"), exist_ok=True)
    return cpp_build.build_program("attention/test_outer_api", gate=True)


def test_program_links_and_prints_its_usage():
    out = subprocess.run([build_api_test(), "run"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "usage" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("log2n", (10, 12))
def test_cpp_outer_product_facade(log2n):
    out = subprocess.run([build_api_test(), "run", str(log2n), str(sg.GATE_SECONDS)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("outer product C++ facade OK"), out.stdout[-4000:] + out.stderr[-2000:]
    errs = re.findall(r"the words of multiply_rescale_range on (\d+) pairs; max slot error 2\^(-?[0-9.]+)", out.stdout)
    assert [int(n) for n, _ in errs] == [30, 15] and all(float(e) < -12.0 for _, e in errs), out.stdout
    assert len(re.findall(r"behind the gate", out.stdout)) == 1
