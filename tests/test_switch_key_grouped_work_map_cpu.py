"""CPU: where the workgroups of dpfhe_switch_key_grouped's two kernels work (csrc/workmap.h GroupedKsMap, through tools/emulate_workmap.cpp as in
tests/test_work_maps_cpu.py): every id of both grids is decoded; every (item, group, chunk) of the lift and every (item, component, chunk) of the last pass appears
exactly once, the dead ids number grid - work (none: both maps are exact), and the plan refuses a shape without work, without a data limb, or above 2^31 - 1 ids."""
import ctypes as C
import itertools
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
    u, z, i = C.c_uint, C.c_size_t, C.c_int
    lib.wm_grouped_ks_plan.restype, lib.wm_grouped_ks_plan.argtypes = C.c_uint64, [z, u, u, z, C.POINTER(u), C.POINTER(C.c_uint64), C.POINTER(i)]
    lib.wm_grouped_lift_decode.restype, lib.wm_grouped_lift_decode.argtypes = None, [u, u, i, I64]
    lib.wm_grouped_moddown_decode.restype, lib.wm_grouped_moddown_decode.argtypes = None, [u, i, I64]
    return lib


def plan(wm, batch, L, alpha, n):
    groups, moddown, ok = C.c_uint(), C.c_uint64(), C.c_int()
    lift = wm.wm_grouped_ks_plan(batch, L, alpha, n, C.byref(groups), C.byref(moddown), C.byref(ok))
    return int(lift), int(moddown.value), groups.value, bool(ok.value)


@pytest.mark.parametrize("batch,L,alpha,n", [(1, 6, 2, 256), (3, 7, 2, 8192), (3, 8, 3, 16384), (2, 6, 3, 65536), (5, 5, 1, 4096), (1, 10, 4, 512), (2, 20, 10, 1024)])
def test_every_column_has_exactly_one_workgroup(wm, batch, L, alpha, n):
    lift, moddown, groups, ok = plan(wm, batch, L, alpha, n)
    chunks = (n + 511) // 512
    assert ok and groups == -(-(L - alpha) // alpha)
    for grid, outer, decode in ((lift, groups, lambda out: wm.wm_grouped_lift_decode(lift, groups, chunks, out)), (moddown, 2, lambda out: wm.wm_grouped_moddown_decode(moddown, chunks, out))):
        rows = np.zeros((grid, 3), np.int64)
        decode(rows.ctypes.data_as(I64))
        work = set(itertools.product(range(batch), range(outer), range(chunks)))
        seen = [tuple(r) for r in rows.tolist()]
        live = [w for w in seen if w in work]
        assert len(live) == len(set(live)) == len(work) and len(seen) - len(live) == grid - len(work)


@pytest.mark.parametrize("batch,L,alpha,n", [(0, 6, 2, 256), (1, 6, 0, 256), (1, 6, 6, 256), (1, 6, 7, 256), (1, 6, 2, 0), (1 << 40, 6, 2, 256), ((1 << 31) // 2, 6, 2, 512)])
def test_degenerate_shapes_are_refused(wm, batch, L, alpha, n):
    assert plan(wm, batch, L, alpha, n) == (0, 0, plan(wm, batch, L, alpha, n)[2], False)
    assert plan(wm, (1 << 30) - 1, 3, 1, 512)[3] and plan(wm, (1 << 30) - 1, 3, 1, 512)[1] == (1 << 31) - 2      # the largest last pass that fits
