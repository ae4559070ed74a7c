"""-m gpu: examples/encrypted_softmax_approx - a degree-7 polynomial of x / 4, two squarings, the row sums and ApproxDivide with five Goldschmidt steps at
N = 32768 - built with the examples' own Makefile and run at 2 tokens, 1 rep, JSON: `"correct": true` (every slot of every weight within
error_bound + |p| residual of float64's softmax, and that tolerance below the largest weight) is the pass condition."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_softmax_example_prints_ok_at_two_tokens():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "encrypted_softmax_approx"])
    out = subprocess.run([os.path.join(ROOT, "examples", "encrypted_softmax_approx"), "2", "1", "json"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-4000:] + out.stderr[-2000:]
    row = json.loads(out.stdout.strip().splitlines()[0])
    assert row["tokens"] == 2 and row["goldschmidt_steps"] >= 4 and row["correct"] is True, row
