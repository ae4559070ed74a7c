"""CPU: tests/footprint.py is not vacuous.  A small Python stand-in "kernel" (out[i] = 3 a[i] + 1 mod 2^59 through a scratch buffer, a strided second
output) runs through the arena cleanly under both fill patterns; then one fault at a time is planted in it and every one must be reported with the right
buffer name.  Nothing here touches a device.  The five host twins of the library (expand, plain add, compact, encode, noise) run through the same arena at
ragged item counts and must stay inside their outputs."""
import ctypes as C

import numpy as np
import pytest

from deeppowers_amd import _cabi
from deeppowers_amd.params import ntt_primes
from footprint import MIN_GUARD, PATTERNS, SENTINEL, Arena, FootprintError, run_both_patterns
from test_seeded_cpu import SEED, ref_full

ITEM, ITEMS = 96, 5                 # a ragged little "batch": 5 items of 96 words
STRIDE, KEPT = 7, 4                 # the strided output: 4 of every 7 "limbs" of 16 words are written
MASK = np.uint64((1 << 59) - 1)


def stand_in(fault=None):
    """the arena of the stand-in kernel and the kernel itself; `fault` plants one defect"""
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1 << 59, ITEM * ITEMS, dtype=np.uint64)
    ar = Arena()
    ar.carve("a", a.size, "input", ITEM, data=a)
    ar.carve("work", a.size, "scratch", ITEM)
    ar.carve("out", a.size, "output", ITEM)
    seg = [(p * STRIDE * 16, KEPT * 16) for p in range(ITEMS)]
    ar.carve("strided", (ITEMS - 1) * STRIDE * 16 + KEPT * 16, "output", STRIDE * 16, segments=seg)
    want = (a * np.uint64(3) + np.uint64(1)) & MASK
    want_strided = np.concatenate([want[p * KEPT * 16:(p + 1) * KEPT * 16] for p in range(ITEMS)])

    def kernel(buf):
        o = {n: ar.offset(n) for n in ("a", "work", "out", "strided")}
        x = buf[o["a"]: o["a"] + a.size]
        work = buf[o["work"]: o["work"] + a.size]
        if fault == "reads_scratch":
            carry = work[17]                                  # read before it is written
        work[:] = x * np.uint64(3)
        res = (work + np.uint64(1)) & MASK
        if fault == "reads_scratch":
            res[40] = (res[40] + carry) & MASK
        if fault == "unwritten":
            buf[o["out"]: o["out"] + 200] = res[:200]
            buf[o["out"] + 201: o["out"] + a.size] = res[201:]
        else:
            buf[o["out"]: o["out"] + a.size] = res
        for p in range(ITEMS):
            at = o["strided"] + p * STRIDE * 16
            buf[at: at + KEPT * 16] = res[p * KEPT * 16:(p + 1) * KEPT * 16]
        if fault == "past_end":
            buf[o["out"] + a.size] = 1
        if fault == "before_start":
            buf[o["work"] - 1] = 1
        if fault == "item_past_end":
            buf[o["out"] + a.size + ITEM] = 1
        if fault == "stride_gap":
            buf[o["strided"] + STRIDE * 16 + KEPT * 16 + 3] = 1    # item 1's fifth limb
        if fault == "input":
            buf[o["a"] + 9] ^= np.uint64(1)
    return ar, kernel, {"out": want, "strided": want_strided}


def test_clean_stand_in_passes_under_both_patterns():
    ar, kernel, want = stand_in()
    first, second = run_both_patterns(ar, kernel, want)
    assert first[0] == PATTERNS[0] and second[0] == PATTERNS[1]                  # (word 0 is guard: each run really had its own pattern)
    assert np.array_equal(ar.view(first, "out"), ar.view(second, "out"))


PLANTED = {
    "past_end": ("out", "after", ITEM * ITEMS, ITEM * ITEMS),
    "before_start": ("work", "before", -1, -1),
    "item_past_end": ("out", "after", ITEM * ITEMS + ITEM, ITEM * ITEMS + ITEM),
    "stride_gap": ("strided", "gap", STRIDE * 16 + KEPT * 16 + 3, STRIDE * 16 + KEPT * 16 + 3),
    "input": ("a", "input", 9, 9),
    "unwritten": ("out", "unwritten", 200, 200),
    "reads_scratch": ("out", "wrong", 40, 40),
}


@pytest.mark.parametrize("fault", list(PLANTED))
def test_every_planted_fault_is_reported_with_its_buffer(fault):
    ar, kernel, want = stand_in(fault)
    with pytest.raises(FootprintError) as e:
        run_both_patterns(ar, kernel, want)
    buffer, kind, first, last = PLANTED[fault]
    assert (e.value.buffer, e.value.kind, e.value.first, e.value.last) == (buffer, kind, first, last), str(e.value)
    assert buffer in str(e.value) and str(first) in str(e.value)


def test_one_item_past_the_end_is_still_inside_the_guard():
    """the guard holds one whole item (and at least MIN_GUARD words), so the 'one item past the end' fault above lands in `out`'s own guard"""
    ar, _, _ = stand_in()
    for r in ar.regions.values():
        assert r.guard >= max(r.item_words, MIN_GUARD)
    nxt = ar.offset("strided") - ar.regions["strided"].guard
    assert ar.offset("out") + ITEM * ITEMS + ITEM < nxt


def test_patterns_are_no_residues():
    assert int(SENTINEL) == 0xDEADBEEFCAFEF00D and int(PATTERNS[1]) == 0x2152411035010FF2
    assert all(int(p) >= 1 << 60 for p in PATTERNS)


def test_carve_holds_the_guard_and_alignment_conditions():
    ar = Arena()
    at = ar.carve("x", 1000, "output", 2048)
    assert at % 4 == 2 and at >= 2048
    assert ar.carve("w", 33, "input", 8, data=np.zeros(33, np.uint64), align=8) % 2 == 1
    end = ar.total
    with pytest.raises(AssertionError, match="shorter than one item"):
        ar.carve("short", 100, "output", 4096, guard=4095)
    with pytest.raises(AssertionError, match="shorter than one item"):
        ar.carve("short", 100, "output", 16, guard=MIN_GUARD - 1)
    with pytest.raises(AssertionError, match="weakest legal alignment"):
        ar.carve("aligned", 100, "output", 16, offset=(end + MIN_GUARD + 63) // 64 * 64)       # a 512-byte aligned buffer
    with pytest.raises(AssertionError, match="weakest legal alignment"):
        ar.carve("aligned32", 100, "output", 16, offset=(end + MIN_GUARD + 3) // 4 * 4)
    with pytest.raises(AssertionError, match="leaves a guard"):
        ar.carve("close", 100, "output", 16, offset=end + 4 + (2 - end) % 4)                             # rightly aligned, 4 .. 7 words of guard
    with pytest.raises(AssertionError, match="needs its data"):
        ar.carve("nodata", 100, "inout", 16)
    with pytest.raises(AssertionError, match="32-byte aligned"):
        ar.address(16, "x")
    assert ar.address(4096, "x") % 32 == 16 and ar.address(4096, "w") % 16 == 8
    assert ar.total == end and set(ar.regions) == {"x", "w"}                                   # a refused carve leaves the arena as it was


# ---- the host twins through the arena -----------------------------------------------------------------------------------------------------------------------
def _moduli(p):
    return (C.c_uint64 * p.n_limbs)(*p.moduli)


def _host_call(ar, fn):
    def call(buf):
        base = buf.ctypes.data
        _cabi.check(fn(lambda name, extra=0: ar.address(base, name, extra)))
    return call


def _written_everywhere(ar, after, name):
    got = ar.view(after, name)
    assert not np.isin(got, np.array(PATTERNS, np.uint64)).any(), name


@pytest.mark.parametrize("batch,comps,comp", [(1, 2, 1), (3, 3, 0), (5, 2, 0)])
def test_expand_uniform_host_stays_inside_its_component(batch, comps, comp):
    p = ntt_primes(8, 3, 60)
    poly = p.n_limbs * p.n
    lib = _cabi.load()
    ar = Arena()
    ar.carve("buf", batch * comps * poly, "output", comps * poly, segments=[((b * comps + comp) * poly, poly) for b in range(batch)])
    want = ref_full(p, batch, comps, comp, SEED, 7)[:, comp]
    run_both_patterns(ar, _host_call(ar, lambda at: lib.dpfhe_expand_uniform_host(_moduli(p), p.n_limbs, p.log2_n, at("buf"), batch, comps, comp, SEED, 7)),
                      {"buf": want})


@pytest.mark.parametrize("batch,comps,plain_items", [(1, 2, 1), (3, 3, 1), (6, 2, 3)])
def test_add_plain_scaled_host_stays_inside_its_output(batch, comps, plain_items):
    p = ntt_primes(8, 3, 60)
    poly = p.n_limbs * p.n
    lib = _cabi.load()
    rng = np.random.default_rng(batch)
    ct = rng.integers(0, 1 << 62, (batch, comps, p.n_limbs, p.n), dtype=np.uint64) % np.array(p.moduli, np.uint64)[:, None]
    plain = rng.integers(0, 65537, (plain_items, p.n), dtype=np.uint64)
    ar = Arena()
    ar.carve("in", ct.size, "input", comps * poly, data=ct)
    ar.carve("plain", plain.size, "input", p.n, data=plain)
    ar.carve("out", ct.size, "output", comps * poly)
    fn = lambda at: lib.dpfhe_add_plain_scaled_host(_moduli(p), p.n_limbs, p.log2_n, at("out"), at("in"), at("plain"), batch, comps, plain_items, 65537, 0)
    first, second = run_both_patterns(ar, _host_call(ar, fn), {})
    _written_everywhere(ar, first, "out")
    _written_everywhere(ar, second, "out")
    got = ar.view(first, "out").reshape(ct.shape)
    assert np.array_equal(got, ar.view(second, "out").reshape(ct.shape)) and np.array_equal(got[:, 1:], ct[:, 1:])
    # the same call in place: one inout buffer
    ip = Arena()
    ip.carve("ct", ct.size, "inout", comps * poly, data=ct)
    ip.carve("plain", plain.size, "input", p.n, data=plain)
    fn = lambda at: lib.dpfhe_add_plain_scaled_host(_moduli(p), p.n_limbs, p.log2_n, at("ct"), at("ct"), at("plain"), batch, comps, plain_items, 65537, 0)
    run_both_patterns(ip, _host_call(ip, fn), {"ct": got})


@pytest.mark.parametrize("batch,bits", [(1, (8, 8)), (3, (60, 21)), (5, (33, 60))])
def test_compact_host_stays_inside_its_records(batch, bits):
    p = ntt_primes(8, 3, 60)
    poly = p.n_limbs * p.n
    lib = _cabi.load()
    rng = np.random.default_rng(batch)
    ct = rng.integers(0, 1 << 62, (batch, 2, p.n_limbs, p.n), dtype=np.uint64) % np.array(p.moduli, np.uint64)[:, None]
    rec = p.n * sum(bits) // 64                               # words per record (N is a multiple of 64)
    ar = Arena()
    ar.carve("in", ct.size, "input", 2 * poly, data=ct)
    ar.carve("out", batch * rec, "output", rec)
    fn = lambda at: lib.dpfhe_compact_host(_moduli(p), p.n_limbs, p.log2_n, at("out"), at("in"), batch, bits[0], bits[1])
    first, second = run_both_patterns(ar, _host_call(ar, fn), {})
    assert np.array_equal(ar.view(first, "out"), ar.view(second, "out"))
    _written_everywhere(ar, first, "out")


@pytest.mark.parametrize("items,flags", [(1, 0), (3, 0), (5, _cabi.ENCODE_PLAIN)])
def test_encode_slots_host_stays_inside_its_output(items, flags):
    p = ntt_primes(8, 3, 60)
    lib = _cabi.load()
    t = 65537
    slots = np.random.default_rng(items).integers(0, t, (items, p.n), dtype=np.uint64).astype(np.uint32)
    per = p.n if flags else p.n_limbs * p.n
    ar = Arena()
    ar.carve("slots", slots.size // 2, "input", p.n // 2, data=slots.view(np.uint64))
    ar.carve("out", items * per, "output", per)
    fn = lambda at: lib.dpfhe_encode_slots_host(_moduli(p), p.n_limbs, p.log2_n, t, at("out"), at("slots"), items, flags)
    first, second = run_both_patterns(ar, _host_call(ar, fn), {})
    _written_everywhere(ar, first, "out")
    assert np.array_equal(ar.view(first, "out"), ar.view(second, "out"))


@pytest.mark.parametrize("batch,comps,comp,kind", [(1, 2, 1, _cabi.NOISE_TERNARY), (3, 3, 0, _cabi.NOISE_CBD21), (5, 2, 0, _cabi.NOISE_FLOOD)])
def test_sample_noise_host_stays_inside_its_component(batch, comps, comp, kind):
    p = ntt_primes(8, 3, 60)
    poly = p.n_limbs * p.n
    lib = _cabi.load()
    ar = Arena()
    ar.carve("buf", batch * comps * poly, "output", comps * poly, segments=[((b * comps + comp) * poly, poly) for b in range(batch)])
    fn = lambda at: lib.dpfhe_sample_noise_host(_moduli(p), p.n_limbs, p.log2_n, at("buf"), batch, comps, comp, kind, 40, 2, SEED, 3, 0)
    first, second = run_both_patterns(ar, _host_call(ar, fn), {})
    _written_everywhere(ar, first, "buf")
    assert np.array_equal(ar.view(first, "buf"), ar.view(second, "buf"))
    assert (ar.view(first, "buf").reshape(batch, p.n_limbs, p.n) < np.array(p.moduli, np.uint64)[:, None]).all()
