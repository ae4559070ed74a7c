"""Slot sums in the C++ facade (HybridKeySwitcher::rotate_add_range, SlotSum): builds tests/cpp/test_slot_sum_api.cpp and, -m gpu, runs it ONCE - on encrypted
inputs at N = 4096, Ld = 4, three tokens: blocks 2, 8 and 2048 at stride 1 and block 8 at stride 4 in the approximate family, every decoded slot within the
stated error_bound of the float64 sum; block 8 in the exact family, the decrypted slots equal to the sums mod t; apply() behind the stream gate; the
rejections - and then holds the Python mirror (Evaluator.rotate_add_hybrid) to the words the program dumped: the facade's own keys and ciphertexts.
Without a GPU: the program links, and its `ref` mode (no device) shows that every drawn case has max|sum| >= 1 and error_bound <= 2^-10 max|sum|, so the
tolerance cannot hide an error of the order of the outputs."""
import math
import re
import subprocess

import numpy as np
import pytest

import cpp_build
import stream_gate as sg

CASES = [(2, 1), (8, 1), (2048, 1), (8, 4)]
MAGIC = 0x534C4F5453554D31


def build_api_test():
    return cpp_build.build_program("test_slot_sum_api", gate=True)


def test_program_links_and_its_cases_have_sums_of_order_one_and_a_tight_bound():
    out = subprocess.run([build_api_test(), "ref"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = re.findall(r"^block (\d+) stride (\d+): max\|sum\| = ([0-9.]+) error_bound = 2\^(-?[0-9.]+)", out.stdout, re.M)
    assert [(int(r[0]), int(r[1])) for r in rows] == CASES, out.stdout
    for block, _, smax, log2_bound in rows:
        assert float(smax) >= 1.0 and float(log2_bound) <= -10.0 + math.log2(float(smax)), out.stdout
        assert 0.5 * int(block) <= float(smax) <= int(block)          # inputs in [0.5, 1]


@pytest.fixture(scope="module")
def program_run(tmp_path_factory):
    dump = tmp_path_factory.mktemp("slot_sum") / "words.bin"
    out = subprocess.run([build_api_test(), str(sg.GATE_SECONDS), str(dump)], capture_output=True, text=True, timeout=600)
    return out, dump


@pytest.mark.gpu
def test_cpp_slot_sum_facade(program_run):
    out, _ = program_run
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("slot sum C++ facade OK"), out.stdout[-4000:] + out.stderr[-2000:]
    assert len(re.findall(r"error_bound 2\^-", out.stdout)) == 4 and len(re.findall(r"behind the gate", out.stdout)) == 1
    assert "exact family, block 8, 2 items: 0 wrong slots of 8192" in out.stdout


@pytest.mark.gpu
def test_python_mirror_gives_the_facade_words(program_run):
    """last: the ladder of SlotSum(2048) on two of the program's ciphertexts under the facade's keys, through Evaluator.rotate_add_hybrid"""
    import torch
    from deeppowers_amd.evaluator import Ciphertext, Context, Evaluator, to_device, to_host
    from deeppowers_amd.params import FheParams
    out, dump = program_run
    assert out.returncode == 0, out.stdout[-2000:]
    raw = np.fromfile(dump, dtype="<u8")
    magic, log2n, L, steps, T = (int(v) for v in raw[:5])
    assert magic == MAGIC and (log2n, L, steps, T) == (12, 5, 11, 2)
    n, Ld, at = 1 << log2n, L - 1, 5
    moduli, psi = [int(v) for v in raw[at:at + L]], [int(v) for v in raw[at + L:at + 2 * L]]
    elts = [int(v) for v in raw[at + 2 * L:at + 2 * L + steps]]
    assert elts == [pow(3, 1 << e, 2 * n) for e in range(steps)]
    at += 2 * L + steps
    keys = raw[at:at + steps * Ld * 2 * L * n].reshape(steps, Ld, 2, L, n)
    at += keys.size
    cin = raw[at:at + T * 2 * Ld * n].reshape(T, 2, Ld, n)
    want = raw[at + cin.size:].reshape(T, 2, Ld, n)
    ctx = Context(FheParams(log2n, tuple(moduli), tuple(psi)), 0)
    try:
        got = Evaluator(ctx).rotate_add_hybrid(Ciphertext(to_device(np.ascontiguousarray(cin), ctx.device)), elts, to_device(np.ascontiguousarray(keys), ctx.device))
        torch.cuda.synchronize()
        assert np.array_equal(to_host(got.data), want)
        assert not np.array_equal(cin, want)
    finally:
        ctx.close()
