"""CPU: where a workgroup of the all-pairs tensor product works and what it writes (csrc/workmap.h MulOuterMap, through tools/emulate_workmap.cpp): every id
of the launcher's grid is enumerated, and for every live id the pairs its loops write, by the very predicates the kernel calls (keys, writes, item).

* coverage - every (pair, limb, chunk) of the output is written exactly once: A * B items in the full form, T (T + 1) / 2 in the causal one, also when the
  call is cut into launches over ranges of queries and keys with their offsets (the blocks above the diagonal skipped, as the entry skips them);
* locality - the tiles of one (limb, chunk) have ids equal modulo 8 (one XCD) and consecutive above that;
* dead ids - grid minus work of them, all past the last slab, and they write nothing;
* bounds - every row and key a live id touches is inside its launch's ranges, a ragged last tile has A mod 4 rows, and a lane's pair ends inside the polynomial
  (or past N only in the one partial chunk of N = 256, whose upper lanes idle)."""
import ctypes as C
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64 = C.POINTER(C.c_int64)
LIMBS = 3


@pytest.fixture(scope="module")
def wm(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu") / "libemu_workmap.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "emulate_workmap.cpp")])
    lib = C.CDLL(so)
    S = C.c_size_t
    for name, res, args in (("wm_mul_outer_grid", C.c_uint64, [S, S, S]), ("wm_mul_outer_tile", C.c_int, []), ("wm_chunks_of", C.c_int, [S]),
                            ("wm_mul_outer_decode", None, [C.c_uint, C.c_uint, C.c_uint, S, S, S, S, C.c_int, I64]),
                            ("wm_mul_outer_pairs", S, [S, S, S, S, S, S, C.c_int, I64])):
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    return lib


def launch(wm, n, a_count, b_count, a_off, b_off, b_total, causal, written):
    """enumerate one launch: checks its ids, adds (item, limb, chunk) of everything it writes to `written`"""
    tile, chunks = wm.wm_mul_outer_tile(), wm.wm_chunks_of(n)
    assert tile == 4 and chunks == max(1, n // 512)
    tiles = -(-a_count // tile)
    grid = wm.wm_mul_outer_grid(a_count, LIMBS, n)
    work = LIMBS * chunks * tiles
    assert work <= grid == -(-LIMBS * chunks // 8) * 8 * tiles < 10 ** 5
    rows = np.zeros((grid, 6), dtype=np.int64)
    wm.wm_mul_outer_decode(grid, LIMBS, chunks, a_count, b_count, a_off, b_off, int(causal), rows.ctypes.data_as(I64))
    live = [(idx,) + tuple(int(v) for v in r) for idx, r in enumerate(rows) if r[3]]
    assert len(live) == work and {(l, ch, t) for _, l, ch, t, *_ in live} == {(l, ch, t) for l in range(LIMBS) for ch in range(chunks) for t in range(tiles)}
    dead = [idx for idx, r in enumerate(rows) if not r[3]]
    assert len(dead) == grid - work and all((idx >> 3) // tiles * 8 + (idx & 7) >= LIMBS * chunks for idx in dead)      # past the last slab: they return at once
    slab_ids = {}
    buf = np.zeros((tile * max(b_count, 1), 3), dtype=np.int64)
    for idx, l, ch, t, _, keys, nrows in live:
        slab_ids.setdefault((l, ch), []).append(idx)
        assert nrows == min(tile, a_count - t * tile) and 0 <= keys <= b_count
        if not causal:
            assert keys == b_count
        m = wm.wm_mul_outer_pairs(t, a_count, b_count, a_off, b_off, b_total, int(causal), buf.ctypes.data_as(I64))
        for item, i, j in buf[:m]:
            assert t * tile <= i < t * tile + nrows and 0 <= j < keys                 # inside the launch's ranges: what the kernel loads
            gi, gj = a_off + int(i), b_off + int(j)
            assert int(item) == (gi * (gi + 1) // 2 + gj if causal else gi * b_total + gj) and (not causal or gj <= gi)
            written[(int(item), l, ch)] += 1
        working = min(256, max(0, (n - ch * 512 + 1) // 2))
        assert working == (128 if n == 256 else 256) and ch * 512 + 2 * (working - 1) + 1 < n
    for ids in slab_ids.values():                                                     # one XCD, consecutive in its order
        assert len({i & 7 for i in ids}) == 1 and sorted(i >> 3 for i in ids) == list(range(min(ids) >> 3, (min(ids) >> 3) + tiles))


def check_once(wm, n, written, items):
    chunks = wm.wm_chunks_of(n)
    assert set(written) == {(it, l, ch) for it in range(items) for l in range(LIMBS) for ch in range(chunks)}
    assert set(written.values()) == {1}


@pytest.mark.parametrize("log2n", (8, 9, 12))
@pytest.mark.parametrize("B", (1, 4, 9))
@pytest.mark.parametrize("A", (1, 3, 4, 5, 9))
def test_full_form_writes_every_pair_limb_and_chunk_once(wm, log2n, A, B):
    written = Counter()
    launch(wm, 1 << log2n, A, B, 0, 0, B, False, written)
    check_once(wm, 1 << log2n, written, A * B)


@pytest.mark.parametrize("log2n", (8, 9, 12))
@pytest.mark.parametrize("T", (1, 2, 4, 5, 9))
def test_causal_form_writes_the_lower_triangle_once(wm, log2n, T):
    written = Counter()
    launch(wm, 1 << log2n, T, T, 0, 0, T, True, written)
    check_once(wm, 1 << log2n, written, T * (T + 1) // 2)


@pytest.mark.parametrize("causal", (False, True))
@pytest.mark.parametrize("T,a_per,b_per", [(9, 4, 2), (9, 8, 3), (5, 4, 2), (5, 5, 3)])
def test_ranges_with_offsets_tile_the_whole_call(wm, T, a_per, b_per, causal):
    """the entry's loop over ranges (whole tiles of queries, keys as they come; under the causal flag the keys past a range's last query are never launched):
    the union of the launches writes everything once"""
    n, written, launches = 512, Counter(), 0
    for a0 in range(0, T, a_per):
        am = min(a_per, T - a0)
        b_end = min(a0 + am, T) if causal else T
        for b0 in range(0, b_end, b_per):
            launch(wm, n, am, min(b_per, b_end - b0), a0, b0, T, causal, written)
            launches += 1
    assert launches > 1 or (a_per >= T and b_per >= T)
    check_once(wm, n, written, T * (T + 1) // 2 if causal else T * T)
