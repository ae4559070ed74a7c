"""CPU: where a workgroup of the sum of tensor products works (csrc/workmap.h mul_sum_grid and chunk_work, through tools/emulate_workmap.cpp like
tests/test_relin_lincomb_work_map_cpu.py): every id of the launcher's grid is enumerated.

* the grid is groups * L * chunks - one workgroup per (group, limb, 512-word chunk), none dead; it does not depend on the number of terms (a workgroup loops
  over its group's terms) nor on whether the second operand is shared;
* coverage - the ids are every (chunk, limb, group) exactly once;
* order - id = (group * L + limb) * chunks + chunk: the chunks of one output row are consecutive;
* bounds - the last lane's pair of the last chunk ends inside the polynomial, or past N only in the one partial chunk of N = 256, whose upper lanes idle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64 = C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def wm(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu") / "libemu_workmap.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "emulate_workmap.cpp")])
    lib = C.CDLL(so)
    for name, res, args in (("wm_mul_sum_grid", C.c_uint64, [C.c_size_t, C.c_size_t, C.c_size_t]), ("wm_chunk_decode", None, [C.c_uint, C.c_int, C.c_int, I64]),
                            ("wm_chunks_of", C.c_int, [C.c_size_t])):
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    return lib


@pytest.mark.parametrize("log2n,groups,limbs", [(8, 1, 1), (8, 3, 4), (9, 3, 2), (9, 1, 5), (15, 1, 8), (15, 2, 3)])
def test_every_chunk_of_every_limb_of_every_group_once(wm, log2n, groups, limbs):
    n = 1 << log2n
    chunks = wm.wm_chunks_of(n)
    assert chunks == max(1, n // 512)
    grid = wm.wm_mul_sum_grid(groups, limbs, n)
    assert grid == groups * limbs * chunks < 10 ** 5
    rows = np.zeros((grid, 3), dtype=np.int64)
    wm.wm_chunk_decode(grid, chunks, limbs, rows.ctypes.data_as(I64))
    got = [tuple(int(v) for v in r) for r in rows]
    want = {(ch, l, g) for g in range(groups) for l in range(limbs) for ch in range(chunks)}
    assert len(got) == len(want) == len(set(got)) and set(got) == want
    for idx, (ch, l, g) in enumerate(got):
        assert idx == (g * limbs + l) * chunks + ch
        assert ch * 512 + 2 * 255 + 1 < max(n, 512)      # the last lane's pair stays inside the chunk row (lanes with a first word past N return)
