"""The approximate packed layer of the C++ facade (ApproxPackedLinear, Evaluator::add_plain / sub_plain): builds tests/cpp/test_approx_linear_api.cpp and,
-m gpu, runs it - every shape's unpacked outputs within the layer's stated error_bound of the float64 W x + b, with and without bias, one and two
tokens per ciphertext, one and two output ciphertexts; the stream contract of apply(); the constructor's rejections.  Without a GPU: the program links,
and the cases it draws have max|y| >= 1 (its `ref` mode touches no device), so the tolerance cannot hide an error of the order of the outputs."""
import os
import re
import subprocess

import pytest

import stream_gate as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_approx_linear_test():
    """rebuilt only when the source, the header or a library changed"""
    exe = os.path.join(ROOT, "tests", "cpp", "test_approx_linear_api")
    src = os.path.join(ROOT, "tests", "cpp", "test_approx_linear_api.cpp")
    lib, gate_dir = os.path.join(ROOT, "deeppowers_amd"), os.path.dirname(sg.build_library())
    deps = [src, sg.LIB, os.path.join(ROOT, "include", "deeppowers", "fhe.hpp"), os.path.join(lib, "libdpfhe_api.so")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", src, "-o", exe,
                               "-L" + lib, "-ldpfhe_api", "-ldpfhe_hip", "-L" + gate_dir, "-lstream_gate", "-L/opt/rocm/lib", "-lamdhip64",
                               f"-Wl,-rpath,{lib}", f"-Wl,-rpath,{gate_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


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
