"""CPU: the complex slot-encoding kernels' per-lane code (csrc/cencode.h cenc_lane_*, what k_cencode.hip runs between its barriers) emulated lane by
lane (tools/emulate_cencode.cpp) must give the host twin's words bit for bit: the one-kernel form at N = 256 and N = 4096 with the lane counts the
launcher uses, the two-kernel form at the smallest ring that takes it (N = 32768: 4096-word chunks, 2 levels left for the second kernel), and the
same split at chunk sizes small enough to be cheap (1, 2 and 3 levels left)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from deeppowers_amd import ckks
from complex_encode_ref import special_vectors, twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULI = (1152921504606830593, 12289, 2013265921)   # a 60-bit limb, a 14-bit one, a 31-bit one


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu") / "libemu_cencode.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "emulate_cencode.cpp")])
    lib = C.CDLL(so)
    lib.emu_encode_complex.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double,
                                       C.c_int, C.c_int]
    lib.emu_encode_complex.restype = C.c_int
    return lib


@pytest.mark.parametrize("log2n,log2c,threads", [(8, 7, 16), (12, 11, 256), (15, 12, 512), (9, 7, 16), (10, 7, 16), (11, 7, 16), (12, 9, 64)])
def test_emulated_lanes_match_host_twin(emu, log2n, log2c, threads):
    h = 1 << (log2n - 1)
    z = special_vectors(np.random.default_rng(log2n * 100 + log2c), log2n)
    items = z.shape[0] if log2n < 15 else 2
    z = z[[0, 2][:items]] if items == 2 else z
    m = (C.c_uint64 * len(MODULI))(*MODULI)
    for real in (False, True):
        src = ckks.aligned((items, h), np.float64 if real else np.complex128)
        src[...] = z.real + z.imag if real else z
        for scale in (2.0 ** 40, 2.0 ** 60):
            for plain in (False, True):
                out = ckks.aligned((items, 1 << log2n) if plain else (items, len(MODULI), 1 << log2n), np.uint64)
                out[...] = 0xDEADBEEFCAFEF00D
                assert emu.emu_encode_complex(log2n, log2c, threads, m, len(MODULI), out.ctypes.data, src.ctypes.data, items, scale, int(real), int(plain)) == 0
                want = twin(MODULI, log2n, src, scale, plain=plain)
                assert np.array_equal(out, want.view(np.uint64)), (log2n, log2c, threads, real, scale, plain)
