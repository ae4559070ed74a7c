"""CPU: where a workgroup of the fused relinearise + linear combination + rescale pass works (csrc/workmap.h relin_rescale_grid and chunk_work, through
tools/emulate_workmap.cpp like tests/test_rotate_add_work_map_cpu.py): every id of the launcher's grid is enumerated.

* the grid is batch * 2 * (Ld - 1) * chunks - one workgroup per (polynomial, KEPT limb, 512-word chunk), none dead;
* coverage - the ids are every (chunk, kept limb, polynomial) exactly once; no id names the dropped limb Ld - 1 or the special limb, which every workgroup reads
  beside its own; polynomial = item * 2 + component runs over both components of every item;
* order - id = (polynomial * (Ld - 1) + limb) * chunks + chunk: the chunks of one output row are consecutive, the Ld - 1 workgroups that share a polynomial's
  rows Ld - 1 and P follow each other chunk-row by chunk-row."""
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
    for name, res, args in (("wm_relin_rescale_grid", C.c_uint64, [C.c_size_t, C.c_size_t, C.c_size_t]), ("wm_chunk_decode", None, [C.c_uint, C.c_int, C.c_int, I64]),
                            ("wm_chunks_of", C.c_int, [C.c_size_t])):
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    return lib


@pytest.mark.parametrize("log2n", range(8, 17))
def test_chunks_tile_the_polynomial(wm, log2n):
    n = 1 << log2n
    chunks = wm.wm_chunks_of(n)
    assert chunks == max(1, n // 512) and chunks * 512 >= n > (chunks - 1) * 512      # one partial chunk below N = 512, whole chunks above


@pytest.mark.parametrize("log2n,batch,data_limbs", [(8, 1, 2), (8, 3, 4), (12, 3, 2), (12, 3, 4), (13, 8, 5), (14, 1, 2), (15, 2, 7), (16, 1, 3)])
def test_every_kept_row_of_every_polynomial_once(wm, log2n, batch, data_limbs):
    n = 1 << log2n
    chunks, kept = wm.wm_chunks_of(n), data_limbs - 1
    grid = wm.wm_relin_rescale_grid(batch, data_limbs, n)
    assert grid == batch * 2 * kept * chunks < 10 ** 5
    rows = np.zeros((grid, 3), dtype=np.int64)
    wm.wm_chunk_decode(grid, chunks, kept, rows.ctypes.data_as(I64))
    got = [tuple(int(v) for v in r) for r in rows]
    want = {(ch, l, p) for p in range(2 * batch) for l in range(kept) for ch in range(chunks)}
    assert len(got) == len(want) == len(set(got)) and set(got) == want
    assert int(rows[:, 1].max()) == kept - 1 and int(rows[:, 2].max()) == 2 * batch - 1
    for idx, (ch, l, p) in enumerate(got):
        assert idx == (p * kept + l) * chunks + ch
        assert ch * 512 + 2 * 255 + 1 < max(n, 512)                                  # the last lane's pair stays inside the chunk row (lanes past N idle)
