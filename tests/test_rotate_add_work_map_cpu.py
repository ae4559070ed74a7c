"""CPU: where a workgroup of the rotate-and-add ladder's last pass works (csrc/workmap.h RotateAddMap, through tools/emulate_workmap.cpp like
tests/test_work_maps_cpu.py): every id of the launcher's grid is enumerated.

* coverage - the live ids are every (item, data limb, slice) exactly once, the rest of the grid is dead, and the grid is whole rounds of 8 polynomials;
* the slices tile the polynomial: `slices` divides the 512-word chunks, at most 8 where the polynomial is staged in LDS (N <= 8192, 64 KiB), one per chunk
  above, and one for a ring below a chunk;
* locality - the slices of one polynomial share an XCD (id & 7) and are consecutive there (id >> 3): whatever they read of c0 - all of it when staged,
  the gathered words otherwise - comes from HBM once."""
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
    for name, res, args in (("wm_rotate_add_slices", C.c_uint, [C.c_size_t]), ("wm_rotate_add_staged", C.c_int, [C.c_size_t]),
                            ("wm_rotate_add_grid", C.c_uint64, [C.c_size_t, C.c_uint]),
                            ("wm_rotate_add_decode", None, [C.c_uint, C.c_uint, C.c_size_t, C.c_uint, I64]), ("wm_chunks_of", C.c_int, [C.c_size_t])):
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    return lib


@pytest.mark.parametrize("log2n", range(8, 17))
def test_slices_tile_the_polynomial(wm, log2n):
    n = 1 << log2n
    chunks, slices, staged = wm.wm_chunks_of(n), wm.wm_rotate_add_slices(n), bool(wm.wm_rotate_add_staged(n))
    assert staged == (n * 8 <= 64 * 1024)                       # the polynomial fits the LDS a launch gets without raising the limit
    assert slices == (min(chunks, 8) if staged else chunks) and slices >= 1 and chunks % slices == 0


@pytest.mark.parametrize("log2n,batch,data_limbs", [(8, 1, 1), (8, 3, 2), (12, 3, 4), (13, 8, 4), (13, 5, 7), (14, 3, 2), (16, 1, 3)])
def test_every_slice_of_every_polynomial_once_and_on_one_xcd(wm, log2n, batch, data_limbs):
    n = 1 << log2n
    slices, polys = wm.wm_rotate_add_slices(n), batch * data_limbs
    grid = wm.wm_rotate_add_grid(polys, slices)
    assert grid == (polys + 7) // 8 * 8 * slices < 10 ** 5
    rows = np.zeros((grid, 4), dtype=np.int64)
    wm.wm_rotate_add_decode(grid, slices, polys, data_limbs, rows.ctypes.data_as(I64))
    live = [tuple(int(v) for v in r[:3]) for r in rows if r[3]]
    want = {(t, l, s) for t in range(batch) for l in range(data_limbs) for s in range(slices)}
    assert len(live) == len(want) == len(set(live)) and set(live) == want
    assert int((rows[:, 3] == 0).sum()) == grid - len(want)
    by_poly = {}
    for idx, r in enumerate(rows):
        if r[3]:
            by_poly.setdefault((int(r[0]), int(r[1])), []).append(idx)
    for key, ids in by_poly.items():
        assert len({i & 7 for i in ids}) == 1, key
        slots = sorted(i >> 3 for i in ids)
        assert slots == list(range(slots[0], slots[0] + slices)), key
