"""CPU: where a workgroup of the products with a shared complement factor works (csrc/workmap.h mul_complement_grid and chunk_work, through
tools/emulate_workmap.cpp like tests/test_mul_sum_work_map_cpu.py): every id of the launcher's grid is enumerated.

* the grid is groups * L * chunks - one workgroup per (group, limb, 512-word chunk); it depends neither on the number of items of a group (a workgroup walks
  them) nor on the self product;
* coverage - the live ids are every (chunk, limb, group) exactly once, and the dead ids number grid minus work: none;
* order - id = (group * L + limb) * chunks + chunk;
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
    for name, res, args in (("wm_mul_complement_grid", C.c_uint64, [C.c_size_t, C.c_size_t, C.c_size_t]), ("wm_chunk_decode", None, [C.c_uint, C.c_int, C.c_int, I64]),
                            ("wm_chunks_of", C.c_int, [C.c_size_t])):
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    return lib


@pytest.mark.parametrize("log2n,groups,limbs", [(8, 1, 1), (8, 3, 4), (9, 3, 2), (10, 1, 5), (12, 2, 3), (15, 1, 8)])
def test_every_chunk_of_every_limb_of_every_group_once(wm, log2n, groups, limbs):
    n = 1 << log2n
    chunks = wm.wm_chunks_of(n)
    assert chunks == max(1, n // 512)
    grid = wm.wm_mul_complement_grid(groups, limbs, n)
    work = groups * limbs * chunks
    assert work <= grid < 10 ** 5
    rows = np.zeros((grid, 3), dtype=np.int64)
    wm.wm_chunk_decode(grid, chunks, limbs, rows.ctypes.data_as(I64))
    got = [tuple(int(v) for v in r) for r in rows]
    live = [(ch, l, g) for ch, l, g in got if g < groups]
    want = {(ch, l, g) for g in range(groups) for l in range(limbs) for ch in range(chunks)}
    assert len(live) == len(want) == len(set(live)) and set(live) == want
    assert len(got) - len(live) == grid - work == 0
    for idx, (ch, l, g) in enumerate(got):
        assert idx == (g * limbs + l) * chunks + ch
        working = min(256, max(0, (n - ch * 512 + 1) // 2))          # lanes whose first word is past N return before they touch memory
        assert working == (128 if n == 256 else 256)
        assert ch * 512 + 2 * (working - 1) + 1 < n                  # the last working lane's pair ends inside the polynomial
