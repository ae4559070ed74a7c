"""CPU: the per-thread loop of reduce_thin_kernel (csrc/reduce_thin.h thin_sum, the lazy 64-bit sums of the shard-local reduce) emulated thread by
thread (tools/emulate_reduce.cpp) with the split bounds the launcher passes.  All-(q - 1) inputs put every lazy sum at its bound: the wrap-around
counter must stay at zero, every partial must come out canonical, and the total must be the exact modular sum."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from deeppowers_amd.params import PRIMES_60

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = C.POINTER(C.c_uint64)
THREADS = 4   # emulated threads = 8 words per item: every thread runs the same loop


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu") / "libemu_reduce.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "emulate_reduce.cpp")])
    lib = C.CDLL(so)
    lib.emu_reduce_thin.argtypes = [C.c_uint64, U, C.c_size_t, C.c_uint, C.c_uint, U]
    lib.emu_reduce_thin.restype = C.c_int
    lib.emu_reduce_overflows.restype = C.c_long
    return lib


def _run(emu, q, data, nsplit=15):
    data = np.ascontiguousarray(data, dtype=np.uint64)
    out = np.zeros(2 * THREADS, dtype=np.uint64)
    rc = emu.emu_reduce_thin(q, data.ctypes.data_as(U), data.shape[0], nsplit, THREADS, out.ctypes.data_as(U))
    return rc, out


# 513: the first count the thin kernel serves; 8192: the benchmark's shard; 1000 and 8191: not multiples of 15 splits x 10 terms per pass (ragged
# splits, ragged rings, ragged ends); 16381: a large odd count
@pytest.mark.parametrize("count", [513, 8192, 1000, 8191, 16381])
def test_lazy_sums_at_their_bound(emu, count):
    before = emu.emu_reduce_overflows()
    for q in (PRIMES_60[0][0], PRIMES_60[3][0], max(p[0] for p in PRIMES_60), min(p[0] for p in PRIMES_60)):
        rc, out = _run(emu, q, np.full((count, 2 * THREADS), q - 1, dtype=np.uint64))
        assert rc == 0
        assert all(int(x) < 15 * q for x in out)
        want = (count * (q - 1)) % q
        assert [int(x) % q for x in out] == [want] * (2 * THREADS), (count, q)
    assert emu.emu_reduce_overflows() == before, "a lazy sum wrapped around 2^64"


@pytest.mark.parametrize("count,nsplit", [(513, 15), (1000, 15), (77, 9), (4, 1), (3, 1), (23, 15)])
def test_random_inputs_match_python_integers(emu, count, nsplit):
    """(the short counts never reach the thin kernel in the library; its loop must still be right for splits shorter than one ring)"""
    rng = np.random.default_rng(count)
    before = emu.emu_reduce_overflows()
    q = PRIMES_60[1][0]
    data = rng.integers(0, q, size=(count, 2 * THREADS), dtype=np.uint64)
    rc, out = _run(emu, q, data, nsplit)
    assert rc == 0
    want = [sum(int(x) for x in data[:, w]) % q for w in range(2 * THREADS)]
    assert [int(x) % q for x in out] == want
    assert emu.emu_reduce_overflows() == before
