"""-m gpu: hoisted slot sums in the C++ facade (HybridKeySwitcher::rotate_sum_range, SlotSum's radix argument): builds tests/cpp/slot_sum/test_slot_sum_radix_api.cpp
and runs it ONCE - at N = 4096, five data limbs + P, (block, stride, radix) = (64, 1, 8), (64, 16, 4), (32, 1, 8): the exact family's sums mod t, the
approximate family within the header's error_bound, radix 2 word for word today's ladder, the stream gate, the rejections."""
import os
import re
import subprocess

import pytest

import cpp_build
import stream_gate as sg


@pytest.mark.gpu
def test_cpp_slot_sum_radix_facade():
    os.makedirs(os.path.join(cpp_build.BIN_DIR, "slot_sum"), exist_ok=True)
    out = subprocess.run([cpp_build.build_program("slot_sum/test_slot_sum_radix_api", gate=True), str(sg.GATE_SECONDS)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("slot sum radix C++ facade OK"), out.stdout[-4000:] + out.stderr[-2000:]
    assert len(re.findall(r"error_bound 2\^-", out.stdout)) == 3 and len(re.findall(r": 0 wrong slots of 8192", out.stdout)) == 3
