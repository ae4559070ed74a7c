"""CPU: the slot-encoding kernels' per-lane code (csrc/encode.h enc_lane_*, what k_encode.hip runs between its barriers) emulated lane by lane
(tools/emulate_encode.cpp) must give the host twin's words: the one-kernel form at N = 256 and N = 4096 with the lane counts the launcher uses, and
the two-kernel form of N = 32768 / 65536 at chunk sizes small enough to run here (2 and 3 levels left for the second kernel)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from encode_ref import slot_vectors, smallest_t, twin
from test_plain_add_cpu import big_prime_t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULI = (1152921504606830593, 12289, 2013265921)   # a 60-bit limb, one below every t used here, a 31-bit one


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu") / "libemu_encode.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "emulate_encode.cpp")])
    lib = C.CDLL(so)
    lib.emu_encode_slots.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    lib.emu_encode_slots.restype = C.c_int
    return lib


def _aligned(shape):
    raw = np.zeros(int(np.prod(shape)) + 2, dtype=np.uint64)
    off = (-raw.ctypes.data % 16) // 8
    return raw[off:off + int(np.prod(shape))].reshape(shape)


@pytest.mark.parametrize("log2n,log2c,threads", [(8, 8, 32), (12, 12, 512), (12, 12, 256), (10, 8, 32), (11, 8, 32), (12, 10, 128)])
def test_emulated_lanes_match_host_twin(emu, log2n, log2c, threads):
    n = 1 << log2n
    for t in (smallest_t(log2n), big_prime_t()):
        slots = slot_vectors(np.random.default_rng(log2n * 100 + log2c), n, t)[[0, 3, 4, 5]]
        sl = _aligned((4, n // 2)).view(np.uint32).reshape(4, n)
        sl[:] = slots
        m = (C.c_uint64 * len(MODULI))(*MODULI)
        for plain in (False, True):
            out = _aligned((4, n) if plain else (4, len(MODULI), n))
            assert emu.emu_encode_slots(log2n, log2c, threads, t, m, len(MODULI), out.ctypes.data, sl.ctypes.data, 4, int(plain)) == 0
            assert np.array_equal(out, twin(MODULI, log2n, t, slots, plain=plain)), (log2n, log2c, threads, t, plain)
