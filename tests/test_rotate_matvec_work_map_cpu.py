"""CPU: the work map of the fused baby steps x diagonals (csrc/workmap.h RotMatvecMap, csrc/rotate_matvec.h), enumerated id by id through
tools/emulate_workmap.cpp with the very functions the kernel and its launcher call.  (Its source side is QpSumMap::source: tests/test_rotate_sum_work_map_cpu.py.)"""
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
    lib.wm_rot_matvec_grid.restype, lib.wm_rot_matvec_grid.argtypes = C.c_uint64, [C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint)]
    lib.wm_rot_matvec_decode.restype, lib.wm_rot_matvec_decode.argtypes = None, [C.c_uint, C.c_int, C.c_uint, C.c_uint, C.c_uint, I64]
    return lib


@pytest.mark.parametrize("log2n,L,rows,items", [(8, 3, 1, 1), (8, 9, 7, 3), (10, 2, 6, 4), (13, 8, 32, 8), (15, 3, 13, 2), (16, 3, 1, 2)])
def test_layout(wm, log2n, L, rows, items):
    """live ids cover every (row, item, limb, output segment) exactly once, dead ids number grid - work, a (limb, segment)'s workgroups sit on one XCD at
    consecutive id >> 3, the items of a row tile next to each other"""
    tile, nseg, rt = wm.wm_rot_matvec_rows(), max(1, (1 << (log2n - 1)) // 256), C.c_uint()
    grid = int(wm.wm_rot_matvec_grid(log2n, L, items, rows, C.byref(rt)))
    per = rt.value * items
    assert rt.value == (rows + tile - 1) // tile and grid == (L * nseg + 7) // 8 * 8 * per
    out = np.zeros((grid, 5), np.int64)
    wm.wm_rot_matvec_decode(grid, log2n, L, items, rt.value, out.ctypes.data_as(I64))
    live = [tuple(r[:4]) for r in out.tolist() if r[4]]
    covered = sorted((row, t, l, s) for l, s, t, tl in live for row in range(tl * tile, min(rows, (tl + 1) * tile)))
    assert covered == sorted((row, t, l, s) for row in range(rows) for t in range(items) for l in range(L) for s in range(nseg))
    assert len(live) == L * nseg * per and grid - len(live) == ((L * nseg + 7) // 8 * 8 - L * nseg) * per
    for key in set(r[:2] for r in live):
        ids = [(i & 7, i >> 3, tl * items + t) for i, (l, s, t, tl, ok) in enumerate(out.tolist()) if ok and (l, s) == key]
        assert len({x for x, _, _ in ids}) == 1 and [q - ids[0][1] for _, q, _ in ids] == [k for _, _, k in ids] == list(range(per))
