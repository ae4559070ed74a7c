"""-m gpu: examples/encrypted_attention_scores_approx - the causal scores of GPT-2 small's 12 heads x 64, interleaved at stride 16, at N = 32768 on
FheParams::n32768(8): the client encrypts q and k, the server runs ApproxAttentionScores, the client decrypts and checks every slot of every pair against
float64 and the bound - prints OK at 2 and at 8 tokens.  Without a GPU: the example builds."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "encrypted_attention_scores_approx")


def build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "encrypted_attention_scores_approx"])
    return EXE


def test_example_builds_and_rejects_bad_arguments():
    out = subprocess.run([build(), "0"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and "tokens in [1, 32]" in out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("tokens", (2, 8))
def test_example_prints_ok(tokens):
    out = subprocess.run([build(), str(tokens), "1", "json"], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-4000:] + out.stderr[-2000:]
    assert f'"tokens": {tokens}' in out.stdout and f'"pairs": {tokens * (tokens + 1) // 2}' in out.stdout and '"correct": true' in out.stdout
