"""-m gpu: grouped key switching in the C++ facade (GroupedKeySwitcher, KeyGenerator::make_grouped_key): builds
tests/cpp/switch_key_grouped/test_grouped_keyswitch_api.cpp and runs it ONCE - at N = 4096, four data limbs and two special primes: a relinearised product and a
switched automorphism decrypt within the header's noise_bound(); the rejections."""
import os
import subprocess

import pytest

import cpp_build


@pytest.mark.gpu
def test_cpp_grouped_key_switch_facade():
    os.makedirs(os.path.join(cpp_build.BIN_DIR, "switch_key_grouped"), exist_ok=True)
    out = subprocess.run([cpp_build.build_program("switch_key_grouped/test_grouped_keyswitch_api")], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("grouped key switch C++ facade OK"), out.stdout[-4000:] + out.stderr[-2000:]
