"""CPU: every C++ facade test program under tests/cpp/ still builds and links through tests/cpp_build.py (no GPU call), and the programs with a no-device
mode run it.  tests/cpp/sampler_stream.cpp is not here: it is a stand-alone program without the library, which tests/test_facade_sampler_cpu.py builds
with its own flags."""
import os
import subprocess

import pytest

import cpp_build

# name -> (what build_program needs, the arguments of the program's no-device mode or None)
PROGRAMS = {
    "test_fhe_api": (dict(oracle=True), None),
    "test_affine_api": ({}, None),
    "test_compact_api": ({}, None),
    "test_seeded_api": ({}, None),
    "test_rerandomize_api": ({}, None),
    "test_encode_api": ({}, None),
    "test_complex_encode_api": ({}, None),
    "facade_digests": ({}, None),
    "test_stream_api": (dict(gate=True), None),
    "test_slot_sum_api": (dict(gate=True), ["ref"]),
    "test_approx_poly_api": (dict(gate=True), ["ref"]),
    "test_approx_linear_api": (dict(gate=True), ["ref"]),
    "approx_layer_words": ({}, None),
    "approx_poly_words": ({}, None),
}


def test_every_program_is_listed():
    sources = {f[:-len(".cpp")] for f in os.listdir(cpp_build.CPP_DIR) if f.endswith(".cpp")}
    assert sources - {"sampler_stream"} == set(PROGRAMS)


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_program_builds_and_links(name):
    needs, no_device = PROGRAMS[name]
    exe = cpp_build.build_program(name, **needs)
    if no_device is not None:
        out = subprocess.run([exe] + no_device, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.strip(), out.stdout + out.stderr
