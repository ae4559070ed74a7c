"""CPU: the generator behind every secret key, error and seed of the C++ facade (deeppowers_amd/csrc/fhe_sampler.h) against its definition.

tests/cpp/sampler_stream.cpp includes that header alone and prints what it draws; everything is restated here independently and must be equal:
the secure path's key stream from chacha20_block of tests/test_seeded_cpu.py (held there to RFC 8439's vector and to openssl) with a 64-bit block
counter in words 12, 13 that starts at 0xFFFFFFFE, so the carry into word 13 happens inside the window; below() as mask-and-reject on that stream;
error() as the difference of two 21-bit popcounts; the TestSeed path as SplitMix64.  The program is built a second time with the address and
undefined-behaviour sanitizers (a stand-alone host program) and must print the same."""
import os
import struct
import subprocess

import pytest

from deeppowers_amd.params import FheParams
from test_seeded_cpu import chacha20_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
KEY_BUFFER = bytes((7 * i + 3) & 0xFF for i in range(40)) + struct.pack("<Q", 0xFFFFFFFE)   # key | nonce | counter start
BOUNDS = (1, 2, 3, 1 << 20, (1 << 20) + 1, FheParams.n4096_l4().moduli[0])
COUNT = 48


def chacha20_stream(buf):
    """64-bit values: the block function's (counter, n0, n1, n2) = (counter low, counter high, nonce), two output words per value"""
    key, nonce, counter = buf[:32], buf[32:40], struct.unpack("<Q", buf[40:48])[0]
    while True:
        block = chacha20_block(key, counter & 0xFFFFFFFF, struct.pack("<I", counter >> 32) + nonce)
        yield from struct.unpack("<8Q", block)
        counter = (counter + 1) & M64


def splitmix64_stream(state):
    while True:
        state = (state + 0x9E3779B97F4A7C15) & M64
        z = ((state ^ (state >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        yield z ^ (z >> 31)


def below(stream, bound):
    if bound <= 1:
        return 0
    mask = (1 << (bound - 1).bit_length()) - 1
    while True:
        v = next(stream) & mask
        if v < bound:
            return v


def error(stream):
    v = next(stream)
    return bin(v & 0x1FFFFF).count("1") - bin((v >> 21) & 0x1FFFFF).count("1")


def restatement():
    lines = []
    for name, fresh in (("chacha20", lambda: chacha20_stream(KEY_BUFFER)), ("testseed", lambda: splitmix64_stream(7))):
        s = fresh()
        lines.append(f"{name} next : " + " ".join(str(next(s)) for _ in range(40)))
        for b in BOUNDS:
            s = fresh()
            lines.append(f"{name} below {b} : " + " ".join(str(below(s, b)) for _ in range(COUNT)))
        s = fresh()
        lines.append(f"{name} ternary : " + " ".join(str(below(s, 3) - 1) for _ in range(COUNT)))
        s = fresh()
        lines.append(f"{name} error : " + " ".join(str(error(s)) for _ in range(COUNT)))
    return lines


def _sanitizers_link(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    return subprocess.call(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], stderr=subprocess.DEVNULL) == 0


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "sanitized"])
def test_sampler_draws_what_its_definition_says(tmp_path, flags):
    if flags and not _sanitizers_link(tmp_path):
        pytest.skip("the host compiler's sanitizer runtimes are not installed")
    exe = str(tmp_path / "sampler_stream")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "deeppowers_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "sampler_stream.cpp"), "-o", exe])
    out = subprocess.run([exe] + [str(b) for b in BOUNDS], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    got, want = out.stdout.splitlines(), restatement()
    assert [l.split(" :")[0] for l in got] == [l.split(" :")[0] for l in want]
    for g, w in zip(got, want):
        assert g == w
    # the window holds what it is meant to hold: the counter's carry, a rejection, both signs
    stream = chacha20_stream(KEY_BUFFER)
    first = [next(stream) for _ in range(40)]
    assert first[16:24] == list(struct.unpack("<8Q", chacha20_block(KEY_BUFFER[:32], 0, struct.pack("<I", 1) + KEY_BUFFER[32:40])))
    assert any((v & 3) == 3 for v in first)                       # below(3) rejects at least once
    assert {-1, 0, 1} <= set(int(v) for v in want[7].split(" : ")[1].split())
