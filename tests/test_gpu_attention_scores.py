"""The attention scores in the C++ facade (ApproxAttentionScores): builds tests/cpp/attention/test_attention_api.cpp and, -m gpu, runs it - on encrypted queries
and keys at N = 1024 and N = 4096 on 60-bit fold primes with the special prime, both packings (one head: block 16, stride 1; heads interleaved: block 8,
stride 4, the small stand-in for 64 / 16), full and causal, T in {1, 3, 5}: every slot of every pair within the header's error_bound of the float64 score,
distinct pairs' scores at least four bounds apart, word for word the product step on pair lists followed by SlotSum, apply() behind the stream gate
(Gate::gated of tests/cpp/facade_test.h), the rejections.  The measured error and the bound are printed.  Without a GPU: the program links and its `ref` mode
holds the static error_bound to its monotonicity."""
import os
import re
import subprocess

import pytest

import cpp_build
import stream_gate as sg


def build_api_test():
    """tests/cpp/attention/test_attention_api.cpp -> tests/cpp/bin/attention/test_attention_api"""
    os.makedirs(os.path.join(cpp_build.BIN_DIR, "attention"), exist_ok=True)
    return cpp_build.build_program("attention/test_attention_api", gate=True)


def test_program_links_and_prints_its_usage():
    out = subprocess.run([build_api_test(), "run"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "usage" in out.stdout, out.stdout + out.stderr


def test_static_error_bound_needs_no_device():
    out = subprocess.run([build_api_test(), "ref"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("attention scores reference OK"), out.stdout + out.stderr
    bounds = [float(v) for v in re.findall(r"block 8: 2\^(-?[0-9.]+)", out.stdout)]
    assert len(bounds) == 2 and bounds[0] < bounds[1] < 0.0, out.stdout      # N = 1024 below N = 4096 (the key-switch term grows with N), both below 1


CASES = [(10, 1, "one", 0), (10, 3, "one", 1), (10, 5, "one", 0), (10, 1, "heads", 1), (10, 3, "heads", 0), (10, 5, "heads", 1), (12, 5, "heads", 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("log2n,T,packing,causal", CASES)
def test_cpp_attention_scores_facade(log2n, T, packing, causal):
    out = subprocess.run([build_api_test(), "run", str(log2n), str(T), packing, str(causal), str(sg.GATE_SECONDS)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("attention scores C++ facade OK"), out.stdout[-4000:] + out.stderr[-2000:]
    m = re.search(r"(\d+) pairs x \d+ slots, max error 2\^(-?[0-9.]+), error_bound 2\^(-?[0-9.]+)", out.stdout)
    assert m and int(m.group(1)) == (T * (T + 1) // 2 if causal else T * T) and float(m.group(2)) <= float(m.group(3)), out.stdout
    assert len(re.findall(r"behind the gate", out.stdout)) == 1
