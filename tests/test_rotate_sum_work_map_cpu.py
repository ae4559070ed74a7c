"""CPU: the work map of the hoisted slot sums (csrc/workmap.h QpSumMap, csrc/kernels_rotate_sum.h), enumerated id by id through tools/emulate_workmap.cpp
with the very functions the kernel and its launcher call, and its out-to-source pair map against galois_elements.src_pos in Python integers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from galois_elements import all_elements, edge_elements, src_pos

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64 = C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def wm(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu") / "libemu_workmap.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "emulate_workmap.cpp")])
    lib = C.CDLL(so)
    lib.wm_qp_sum_grid.restype, lib.wm_qp_sum_grid.argtypes = C.c_uint64, [C.c_int, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint)]
    lib.wm_qp_sum_decode.restype, lib.wm_qp_sum_decode.argtypes = None, [C.c_uint, C.c_int, C.c_uint, C.c_uint, I64]
    lib.wm_qp_sum_source.restype, lib.wm_qp_sum_source.argtypes = None, [C.c_int, C.c_uint, C.c_uint, I64]
    return lib


@pytest.mark.parametrize("log2n,L,items", [(8, 4, 1), (8, 3, 5), (10, 2, 4), (12, 5, 9), (13, 8, 36), (16, 3, 2)])
def test_layout(wm, log2n, L, items):
    """live ids cover (limb, output segment, tile) exactly once, dead ids number grid - work, a (limb, segment)'s tiles sit on one XCD at consecutive id >> 3"""
    tile, nseg, tiles = wm.wm_qp_sum_tile(), max(1, (1 << (log2n - 1)) // 256), C.c_uint()
    grid = int(wm.wm_qp_sum_grid(log2n, L, items, C.byref(tiles)))
    assert tiles.value == (items + tile - 1) // tile and grid == (L * nseg + 7) // 8 * 8 * tiles.value
    rows = np.zeros((grid, 4), np.int64)
    wm.wm_qp_sum_decode(grid, log2n, L, tiles.value, rows.ctypes.data_as(I64))
    live = [tuple(r[:3]) for r in rows.tolist() if r[3]]
    assert sorted(live) == [(l, s, t) for l in range(L) for s in range(nseg) for t in range(tiles.value)]
    assert grid - len(live) == ((L * nseg + 7) // 8 * 8 - L * nseg) * tiles.value
    for key in set(r[:2] for r in live):
        ids = [(i & 7, i >> 3, t) for i, (l, s, t, ok) in enumerate(rows.tolist()) if ok and (l, s) == key]
        assert len({x for x, _, _ in ids}) == 1 and [q - ids[0][1] for _, q, _ in ids] == [t for _, _, t in ids] == list(range(tiles.value))


@pytest.mark.parametrize("log2n", [8, 10, 13, 16])
def test_source_of_an_output_pair(wm, log2n):
    """output pair m gathers source pair src, swapped iff word 2 m comes from an odd position: every pair under EVERY element of the group at N = 256, 1024;
    the edge elements on three output segments above"""
    half, nseg = 1 << (log2n - 1), max(1, (1 << (log2n - 1)) // 256)
    rows = np.zeros((256, 4), np.int64)
    elts = all_elements(log2n) if log2n <= 10 else edge_elements(log2n)
    assert set(edge_elements(log2n)) <= set(elts)
    for g in elts:
        for oseg in (range(nseg) if log2n <= 10 else (0, nseg // 3, nseg - 1)):
            wm.wm_qp_sum_source(log2n, g, oseg, rows.ctypes.data_as(I64))
            for lane, (out, src, swap, ok) in enumerate(rows.tolist()):
                assert out == oseg * 256 + lane and ok == (out < half)
                if ok:
                    assert (src_pos(g, 2 * out, log2n), src_pos(g, 2 * out + 1, log2n)) == ((2 * src + 1, 2 * src) if swap else (2 * src, 2 * src + 1))
