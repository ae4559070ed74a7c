"""CPU: where a workgroup works.  Every kernel family decodes its workgroup id through one map in csrc/workmap.h, and its launcher takes the grid from
the same header; tools/emulate_workmap.cpp exports both, so every id of every grid below is enumerated here:

* coverage - the live ids decode onto the full work set, each element exactly once; the dead ids number grid - work; the host's grid is the smallest
  that covers the work under the layout's rounding (whole rounds of 8 outer items, one per XCD);
* locality - what each layout exists for: all workgroups that share a key tile (key switching, hoisted rotations), a W tile (matrix-vector products)
  or a (limb, source segment, rotation group) block (baby steps) have the same id & 7 (the same XCD) and occupy consecutive id >> 3 (adjacent in time
  there).  The workgroups that share an x tile of a matrix-vector product (one slab, one group of right-hand sides, every row tile) are `groups`
  apart by construction (the group is the fastest index): the same id & 7, and their sorted id >> 3 are an arithmetic progression of step `groups`
  inside their slab's block of consecutive id >> 3 - consecutive themselves with one group;
* items in chunks (expand, noise, plain add, compact, the two encoders): every THREAD of every id is a lane of an item, the lanes cover items x lanes
  exactly once, and the plan refuses an empty launch, a shift that wraps and a grid above 2^31 - 1;
* the Galois position maps are the permutations the kernels' comments say they are, in Python integers.

A layout change starts here."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from galois_elements import edge_elements

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64 = C.POINTER(C.c_int64)
ROT_MAJOR = 0x80000000


@pytest.fixture(scope="module")
def wm(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu") / "libemu_workmap.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "emulate_workmap.cpp")])
    lib = C.CDLL(so)
    u, z, i, ull = C.c_uint, C.c_size_t, C.c_int, C.c_ulonglong
    for name, res, args in (
        ("wm_relin_plan", C.c_uint64, [z, u, z, u, C.POINTER(u)]),
        ("wm_relin_decode", None, [u, u, u, u, i, i, ull, I64]),
        ("wm_hoisted_plan", None, [z, u, z, i, C.POINTER(u), C.POINTER(u)]),
        ("wm_hoisted_decode", None, [u, u, u, u, i, I64]),
        ("wm_matvec_grid", C.c_uint64, [z, z, z, z]),
        ("wm_matvec_decode", None, [u, u, u, u, u, I64]),
        ("wm_qp_grid", C.c_uint64, [i, z, z, z, u]),
        ("wm_qp_segments", u, [i, u]),
        ("wm_qp_decode", None, [u, i, u, u, u, u, I64]),
        ("wm_qp_pair_map", None, [i, u, u, u, I64]),
        ("wm_chunks_of", i, [z]),
        ("wm_chunk_decode", None, [u, i, i, I64]),
        ("wm_item_chunk_plan", C.c_uint64, [z, u, u, C.POINTER(u), C.POINTER(u), C.POINTER(i)]),
        ("wm_item_chunk_fixed", C.c_uint64, [z, u, u, C.POINTER(i)]),
        ("wm_item_chunk_lanes", None, [u, u, u, I64]),
        ("wm_transform_decode", None, [u, i, i, i, ull, I64]),
        ("wm_galois_src_pos", i, [i, u, I64]),
    ):
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    return lib


def _rows(fn, n_ids, cols, *args):
    out = np.zeros((n_ids, cols), dtype=np.int64)
    fn(n_ids, *args, out.ctypes.data_as(I64))
    return out


def _round8(x):
    return (x + 7) // 8 * 8


def _check_cover(rows, work, grid):
    """rows: decoded ids, last column = live.  The live rows are `work` (an iterable of tuples), each exactly once; the rest of the grid is dead."""
    assert len(rows) == grid < 10 ** 5
    live = [tuple(int(v) for v in r[:-1]) for r in rows if r[-1]]
    work = list(work)
    assert len(live) == len(work) and set(live) == set(work) and len(set(live)) == len(live)
    assert int((rows[:, -1] == 0).sum()) == grid - len(work)


def _check_local(rows, key, what, step=1):
    """all live ids with the same key(row): one XCD (id & 7) and consecutive id >> 3 (an arithmetic progression of `step`)"""
    groups = {}
    for idx, r in enumerate(rows):
        if r[-1]:
            groups.setdefault(key(r), []).append(idx)
    for k, ids in groups.items():
        assert len({x & 7 for x in ids}) == 1, (what, k)
        q = sorted(x >> 3 for x in ids)
        assert q == list(range(q[0], q[0] + step * len(q), step)), (what, k)


def _check_smallest(rows, grid, group):
    """the grid is whole rounds of 8 outer items x `group`, and its last round is in use"""
    assert grid % (8 * group) == 0
    assert rows[grid - 8 * group:, -1].any()


# ---- key switching -------------------------------------------------------------------------------------------------------------------------------------
def _relin(wm, items, La, kg, key_stride, n_limbs=None, n_active=0, active_map=0):
    blocks = items * La
    n_outer = C.c_uint(0)
    grid = int(wm.wm_relin_plan(blocks, La, key_stride, kg, C.byref(n_outer)))
    rows = _rows(wm.wm_relin_decode, grid, 3, n_outer.value, kg, La, n_limbs or La, n_active, active_map)
    return n_outer.value, grid, rows


@pytest.mark.parametrize("La,kg,n_keys,key_stride", list(itertools.product((1, 3, 5), (1, 2, 3), (1, 7, 8, 9, 17), (0, 4096))))
def test_relin_layouts(wm, La, kg, n_keys, key_stride):
    items = n_keys * kg
    n_outer, grid, rows = _relin(wm, items, La, kg, key_stride)
    _check_cover(rows, itertools.product(range(items), range(La)), grid)
    if kg == 1 and key_stride == 0:        # one key for every item: plain ids, an XCD only touches the key tiles of its own limbs
        assert n_outer == 0 and grid == items * La
        assert [tuple(r) for r in rows] == [(idx // La, idx % La, 1) for idx in range(grid)]
        return
    if n_keys >= 8:                        # key-major: a key's workgroups (all limbs, all items of the group) on one XCD, its key tiles adjacent inside
        assert n_outer == (n_keys * La) | ROT_MAJOR and grid == _round8(n_keys) * La * kg
        _check_smallest(rows, grid, La * kg)
        _check_local(rows, lambda r: r[0] // kg, "key")
    else:                                  # grouped: the items of a group, limb by limb
        assert n_outer == n_keys * La and grid == _round8(n_keys * La) * kg
        _check_smallest(rows, grid, kg)
    _check_local(rows, lambda r: (r[0] // kg, r[1]), "key tile")


@pytest.mark.parametrize("items,La,kg", [(7, 3, 2), (10, 5, 3), (1, 3, 2)])
def test_relin_partial_group_takes_the_plain_layout(wm, items, La, kg):
    n_outer, grid, rows = _relin(wm, items, La, kg, 4096)
    assert n_outer == 0 and grid == items * La
    assert [tuple(r) for r in rows] == [(idx // La, idx % La, 1) for idx in range(grid)]


@pytest.mark.parametrize("kg,n_keys", [(1, 1), (2, 7), (1, 9), (3, 17)])
def test_relin_class_mixture(wm, kg, n_keys):
    """a launch over one arithmetic class: limbs {1, 3, 4} of a 5-limb context through the launch's active_map"""
    limbs, items = (1, 3, 4), n_keys * kg
    amap = sum(l << (4 * i) for i, l in enumerate(limbs))
    for key_stride in (0, 4096):
        n_outer, grid, rows = _relin(wm, items, 3, kg, key_stride, n_limbs=5, n_active=3, active_map=amap)
        _check_cover(rows, itertools.product(range(items), limbs), grid)
        if n_outer:
            _check_local(rows, lambda r: (r[0] // kg, r[1]), "key tile")


# ---- hoisted rotations ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rots,La,tokens,merged", list(itertools.product((1, 5, 64), (2, 4), (1, 3), (0, 1))))
def test_hoisted_layout(wm, rots, La, tokens, merged):
    tiles, blocks = C.c_uint(0), C.c_uint(0)
    wm.wm_hoisted_plan(rots, La, tokens, merged, C.byref(tiles), C.byref(blocks))
    comps = 1 if merged else 2
    assert tiles.value == rots * La * comps and blocks.value == _round8(tiles.value) * tokens
    rows = _rows(wm.wm_hoisted_decode, blocks.value, 5, tokens, tiles.value, La, merged)
    _check_cover(rows, itertools.product(range(rots), range(La), range(comps), range(tokens)), blocks.value)
    _check_smallest(rows, blocks.value, tokens)
    _check_local(rows, lambda r: (r[0], r[1], r[2]), "key tile")


# ---- matrix-vector products ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,chunks,rtiles,groups", list(itertools.product((1, 3), (1, 2), (1, 3), (1, 2))))
def test_matvec_layout(wm, L, chunks, rtiles, groups):
    grid = int(wm.wm_matvec_grid(L, chunks, rtiles, groups))
    assert grid == _round8(L * chunks) * rtiles * groups
    rows = _rows(wm.wm_matvec_decode, grid, 5, L, chunks, rtiles, groups)
    _check_cover(rows, itertools.product(range(L), range(chunks), range(rtiles), range(groups)), grid)
    _check_smallest(rows, grid, rtiles * groups)
    _check_local(rows, lambda r: (r[0], r[1], r[2]), "W tile")
    _check_local(rows, lambda r: (r[0], r[1]), "slab")   # ... which holds every sharer of an x tile
    _check_local(rows, lambda r: (r[0], r[1], r[3]), "x tile", step=groups)   # group is the fastest index: sharers of an x tile are `groups` apart


# ---- baby steps of the double-hoisted products ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2n,L,rots,tokens,pairs", list(itertools.product((8, 10, 13), (2, 4), (1, 16, 17), (1, 3), (1, 2))))
def test_qp_layout(wm, log2n, L, rots, tokens, pairs):
    nseg = wm.wm_qp_segments(log2n, pairs)
    assert nseg == max(1, (1 << (log2n - 1)) // (256 * pairs))
    grid = int(wm.wm_qp_grid(log2n, L, rots, tokens, pairs))
    n_rg = (rots + 15) // 16
    assert grid == _round8(L * nseg) * n_rg * 16 * tokens
    rows = _rows(wm.wm_qp_decode, grid, 5, log2n, pairs, L, rots, tokens)
    _check_cover(rows, itertools.product(range(L), range(nseg), range(rots), range(tokens)), grid)
    _check_smallest(rows, grid, n_rg * 16 * tokens)
    _check_local(rows, lambda r: (r[0], r[1], r[2] // 16), "(limb, source segment, rotation group) block")


def _brv(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def _src_pos(g, p, log2n):
    """2 brv(p') + 1 = g (2 brv(p) + 1) mod 2N"""
    e2 = (g * (2 * _brv(p, log2n) + 1)) % (2 << log2n)
    return _brv((e2 - 1) // 2, log2n)


def _galois_elts(log2n):
    """3, 5, 2N - 1, 3^7, then the rest of galois_elements.edge_elements (the whole group and the other maps: tests/test_galois_elements_cpu.py)"""
    two_n = 2 << log2n
    first = (3, 5, two_n - 1, pow(3, 7, two_n))
    return first + tuple(g for g in edge_elements(log2n) if g not in first)


@pytest.mark.parametrize("log2n,pairs", list(itertools.product((8, 10, 13), (1, 2))))
def test_qp_pair_map(wm, log2n, pairs):
    """aligned pairs go onto aligned pairs of ONE source segment, swapped iff cf = g (2 brv(m) + 1) mod 2N >= N; over the source segments the output
    pairs cover the polynomial exactly once"""
    n, half, seg = 1 << log2n, 1 << (log2n - 1), 256 * pairs
    nseg = wm.wm_qp_segments(log2n, pairs)
    for g in _galois_elts(log2n):
        written = []
        for sseg in range(nseg):
            rows = _rows(lambda n_ids, *a: wm.wm_qp_pair_map(*a), seg, 4, log2n, pairs, g, sseg)
            for out, src, swap, ok in rows.tolist():
                assert ok == (out < half)
                if not ok:
                    continue
                written.append(out)
                assert src // seg == sseg if nseg > 1 else src < half
                cf = (g * (2 * _brv(out, log2n - 1) + 1)) % (2 * n)
                assert swap == (cf >= n)
                s0, s1 = _src_pos(g, 2 * out, log2n), _src_pos(g, 2 * out + 1, log2n)
                assert (s0, s1) == ((2 * src + 1, 2 * src) if swap else (2 * src, 2 * src + 1))
            assert len({o // seg for o, _, _, ok in rows.tolist() if ok}) == 1   # one output segment per source segment
        assert sorted(written) == list(range(half))


# ---- Galois source positions ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2n", [8, 10])
def test_galois_src_pos(wm, log2n):
    n = 1 << log2n
    for g in _galois_elts(log2n):
        out = np.zeros(n, dtype=np.int64)
        assert wm.wm_galois_src_pos(log2n, g, out.ctypes.data_as(I64)) == 0
        assert sorted(out.tolist()) == list(range(n))
        for p, sp in enumerate(out.tolist()):
            assert 2 * _brv(sp, log2n) + 1 == (g * (2 * _brv(p, log2n) + 1)) % (2 * n)


# ---- streaming kernels and batched transforms ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,chunks", list(itertools.product((1, 3), (1, 2, 16))))
def test_chunk_work(wm, L, chunks):
    polys = 3
    rows = _rows(wm.wm_chunk_decode, polys * L * chunks, 3, chunks, L)
    assert [tuple(r) for r in rows.tolist()] == [(c, l, p) for p in range(polys) for l in range(L) for c in range(chunks)]


def test_chunks_of(wm):
    assert [wm.wm_chunks_of(n) for n in (256, 512, 1024, 4096, 8192, 65536)] == [1, 1, 2, 8, 16, 128]


# ---- items in chunks: the byte-stream and encoding families ----------------------------------------------------------------------------------------------
def _item_chunk_plan(wm, outer, lanes, max_threads=256):
    threads, log2_chunks, ok = C.c_uint(0), C.c_uint(0), C.c_int(0)
    grid = int(wm.wm_item_chunk_plan(outer, lanes, max_threads, C.byref(threads), C.byref(log2_chunks), C.byref(ok)))
    return threads.value, log2_chunks.value, grid, bool(ok.value)


def _item_chunk_fixed(wm, outer, threads, log2_chunks):
    ok = C.c_int(0)
    return int(wm.wm_item_chunk_fixed(outer, threads, log2_chunks, C.byref(ok))), bool(ok.value)


def _item_chunk_lanes(wm, grid, log2_chunks, threads):
    """(outer, lane) of every thread of every id of the grid"""
    out = np.zeros((grid * threads, 2), dtype=np.int64)
    wm.wm_item_chunk_lanes(grid, log2_chunks, threads, out.ctypes.data_as(I64))
    return out


def _covers_once(rows, outer, lanes):
    """the rows (outer, lane) are outer x lanes, each pair exactly once (so no id and no thread is dead)"""
    assert len(rows) == outer * lanes
    assert (rows >= 0).all() and (rows[:, 0] < outer).all() and (rows[:, 1] < lanes).all()
    assert np.array_equal(np.sort(rows[:, 0] * lanes + rows[:, 1]), np.arange(outer * lanes))


@pytest.mark.parametrize("log2n,outer", list(itertools.product(range(8, 17), (1, 3, 8, 9))))
def test_item_chunk_layout(wm, log2n, outer):
    """N / 2 lanes per item (noise, plain add, compact) and N / 4 per (item, limb) (expand), at most 256 per workgroup"""
    for lanes in ((1 << log2n) // 2, (1 << log2n) // 4):
        threads, log2_chunks, grid, ok = _item_chunk_plan(wm, outer, lanes)
        assert ok and threads << log2_chunks == lanes and grid == outer << log2_chunks
        assert threads == (256 if log2n >= 10 else lanes) and threads in (64, 128, 256)
        _covers_once(_item_chunk_lanes(wm, grid, log2_chunks, threads), outer, lanes)


# (log2 of the transform's length, log2c): the slot encoder's N words with 64 KiB of LDS, the complex encoder's N / 2 complex words with 128 KiB
ENCODE_WHOLE = [(v, v) for v in range(8, 15)] + [(v, v) for v in range(7, 14)]
ENCODE_CHUNKED = [(15, 13), (16, 13), (14, 12), (15, 12)]


@pytest.mark.parametrize("log2v,log2c", sorted(set(ENCODE_WHOLE)) + ENCODE_CHUNKED)
def test_encode_chunk_layout(wm, log2v, log2c):
    """first kernel: a workgroup per chunk of 2^log2c words, its lanes walking the chunk in groups of 8; second kernel (chunked form): a lane per pair of
    columns of the chunks, 256 per workgroup"""
    items, C_, R = 3, 1 << log2c, log2v - log2c
    threads = min(C_ >> 3, 512)
    grid, ok = _item_chunk_fixed(wm, items, threads, R)
    assert ok and grid == items << R
    first = _item_chunk_lanes(wm, grid, R, 1)                       # (item, chunk): thread 0's lane with one thread per chunk is the chunk itself
    _covers_once(first, items, 1 << R)
    words = (first[:, :1] << log2v) + (first[:, 1:] << log2c) + np.arange(C_)   # the chunk's words start at base = chunk << log2c
    assert np.array_equal(np.sort(words.ravel()), np.arange(items << log2v))
    if R == 0:
        return
    t_threads, t_log2_chunks, t_grid, ok = _item_chunk_plan(wm, items, C_ // 2, 256)
    assert ok and t_threads == 256 and t_grid == items * (C_ // 2 // 256)
    tail = _item_chunk_lanes(wm, t_grid, t_log2_chunks, t_threads)
    _covers_once(tail, items, C_ // 2)
    # lane j reads and writes positions 2 j, 2 j + 1 of each of the 2^R chunks: over the lanes, every position of the vector exactly once
    pos = np.concatenate([tail[:, :1] * (1 << log2v) + (c << log2c) + 2 * tail[:, 1:] + h for c in range(1 << R) for h in (0, 1)])
    assert np.array_equal(np.sort(pos.ravel()), np.arange(items << log2v))


def test_item_chunk_bounds(wm):
    """ok = at least one item, no overflow of the shift, at most 2^31 - 1 workgroups"""
    assert _item_chunk_plan(wm, 2 ** 31 - 1, 256) == (256, 0, 2 ** 31 - 1, True)
    assert not _item_chunk_plan(wm, 2 ** 31, 256)[3]                # one chunk: the first grid of 2^31
    assert _item_chunk_plan(wm, 2 ** 29 - 1, 1024) == (256, 2, 2 ** 31 - 4, True)
    assert not _item_chunk_plan(wm, 2 ** 29, 1024)[3]               # four chunks: the first grid of 2^31
    threads, log2_chunks, grid, ok = _item_chunk_plan(wm, 2 ** 62 + 1, 1024)
    assert (log2_chunks, grid, ok) == (2, 4, False)                 # the shift wraps to a grid of 4: refused
    assert not _item_chunk_plan(wm, 0, 1024)[3]
    assert _item_chunk_fixed(wm, 2 ** 28 - 1, 512, 3) == (2 ** 31 - 8, True)
    assert not _item_chunk_fixed(wm, 2 ** 28, 512, 3)[1] and not _item_chunk_fixed(wm, 2 ** 61 + 1, 512, 3)[1] and not _item_chunk_fixed(wm, 0, 512, 3)[1]


def test_transform_block(wm):
    """block p transforms words [p N, (p + 1) N): (item, limb, sub-block) in that order - or, in a launch over one class, the class's limbs of every item"""
    rows = _rows(wm.wm_transform_decode, 2 * 3 * 8, 3, 8, 3, 0, 0)
    assert [tuple(r) for r in rows.tolist()] == [(p, (p // 8) % 3, p % 8) for p in range(48)]
    limbs = (1, 3, 4)
    amap = sum(l << (4 * i) for i, l in enumerate(limbs))
    rows = _rows(wm.wm_transform_decode, 4 * 3, 3, 1, 5, 3, amap)
    assert [tuple(r) for r in rows.tolist()] == [(item * 5 + l, l, 0) for item in range(4) for l in limbs]
