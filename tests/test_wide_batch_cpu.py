"""tests/wide_batch.py must see planted defects (the house rule of tests/footprint.py and tests/stream_gate.py): the plan and the checker run here
against numpy model kernels at a scaled-down line (B31 = 2^16 bytes, so B32 = 2^14 words and W32 = 2^17 words).  One correct model, one model per 32-bit
defect a kernel or launcher can have.  The checker must pass the correct model and name EVERY defect - a condition, not a measurement: the share of
planted defects it may miss is zero.  The plan refuses an even period, and one test shows why.  Last, every case of tests/test_gpu_wide_batch.py is
planned here at the real lines: its batch stays within the entry's documented limits and its peak within the tier's cap, and the peaks are pinned, so the
memory condition under which a tier B case may skip cannot be loosened quietly."""
import numpy as np
import pytest
import torch

import wide_batch as wb

SMALL = wb.Lines(1 << 16)
WORDS = 256                     # a power-of-two item: a wrap moves an access by a whole number of items, the hard case
LIMB = 64
MASK = np.uint64((1 << 59) - 1)
DEFECTS = ("write_truncated", "write_sign_wrapped", "read_truncated", "slice_base_truncated", "store_race", "tail_overrun", "input_scribble")


def f(x):
    """the model operation, word by word: below 2^60, so never the sentinel"""
    return (x * np.uint64(3) + np.uint64(1)) & MASK


SLICE = 5                       # items per launch of the model launcher that works in slices


def model(out, inp, batch, words, wrap, defect=None, slice_items=SLICE):
    """out[i] = f(in[i]) with byte / word offsets that wrap at `wrap` words where the defect says so.  out, inp: CPU tensors as wide_batch makes them"""
    o = out.numpy().view(np.uint64).reshape(-1)
    x = inp.numpy().view(np.uint64).reshape(-1)
    order = list(range(batch))
    if defect == "store_race":                                   # the wrapped stores land first, the correct stores of the low items after them
        order.sort(key=lambda i: i * words < wrap)
    for i in order:
        r = w = i * words
        if defect == "read_truncated":
            r %= wrap
        if defect in ("write_truncated", "store_race"):
            w %= wrap
        if defect == "write_sign_wrapped" and w % wrap >= wrap // 2:   # a negative 32-bit offset: the store is skipped as out of range
            continue
        if defect == "slice_base_truncated":                      # the launcher's slice base wraps, the kernel's offsets inside the slice are right
            w = ((i // slice_items) * slice_items * words) % wrap + (i % slice_items) * words
        o[w: w + words] = f(x[r: r + words])
    if defect == "tail_overrun":
        o[batch * words] = f(x[0])
    if defect == "input_scribble":                                # a wrapped store that lands in an operand
        x[(batch - 1) * words % wrap] = np.uint64(7)


def run(tier, wrap_line, defect, period=3, words=WORDS, planned=True):
    margin = 2 * SLICE if defect == "slice_base_truncated" else 2   # a slice base must lie past the line: the plan's margin for sliced launchers
    pl = wb.plan({"in": words, "out": words}, tier, period=period, lines=SMALL, writable=("out",), margin=margin) if planned else \
        wb.Plan({"in": words, "out": words}, tier, -(-SMALL.highest(tier) // words) + 2, period, SMALL, 0)
    src = (np.random.default_rng(11).integers(0, 1 << 59, (period, words), dtype=np.uint64))
    inp = wb.tile(src, pl.batch, "cpu")
    out = wb.sentinel(pl.batch, words, "cpu")
    model(out, inp, pl.batch, words, SMALL.words[wrap_line], defect)
    wb.check_output("out", out, pl, f(src), LIMB)
    wb.check_input("in", inp, pl, src, LIMB)
    return pl


CROSSINGS = [("A", "B32"), ("B", "B32"), ("B", "W32")]          # (tier, the line at which the model's offsets wrap)


@pytest.mark.parametrize("tier,wrap", CROSSINGS)
def test_the_correct_model_passes(tier, wrap):
    pl = run(tier, wrap, None)
    assert pl.batch * WORDS >= SMALL.highest(tier) + 2 * WORDS and (pl.batch - 1) * WORDS < SMALL.highest(tier) + 2 * WORDS
    assert pl.period == 3


# what the checker must say: (kind, buffer, the line the first wrong word lies beyond - None: below every line) with `half` the line below `wrap`
NAMED = {
    "write_truncated": ("reference", "out", lambda wrap, half: None),          # a low item of the first period, overwritten by a high one
    "write_sign_wrapped": ("unwritten", "out", lambda wrap, half: half),       # the first item past the sign bit stays sentinel
    "read_truncated": ("period", "out", lambda wrap, half: wrap),              # the first item past the line holds the words of item 0, not of item i - 3
    "slice_base_truncated": ("low item", "out", lambda wrap, half: None),        # a low item overwritten by a slice past the line: in the first period or not
    "store_race": ("unwritten", "out", lambda wrap, half: wrap),               # the low item ends up right, the high one is never written
    "tail_overrun": ("tail", "out", lambda wrap, half: "top"),
    "input_scribble": ("input", "in", lambda wrap, half: "any"),
}
HALF = {"B32": "B31", "W32": "W31"}


@pytest.mark.parametrize("defect", DEFECTS)
@pytest.mark.parametrize("tier,wrap", CROSSINGS)
def test_every_planted_defect_is_named(tier, wrap, defect):
    with pytest.raises(wb.WideBatchError) as info:
        run(tier, wrap, defect)
    e = info.value
    kind, buffer, line = NAMED[defect]
    line = line(wrap, HALF[wrap])
    assert (e.kind, e.buffer) == (kind, buffer) or (kind == "low item" and e.kind == ("reference" if e.item < 3 else "period")), (defect, e.kind, e.buffer, str(e))
    if line == "top":
        assert e.line == SMALL.of_tier(tier)[-1] and e.item == -(-SMALL.highest(tier) // WORDS) + 2 and e.word == 0, str(e)
    elif line != "any":
        assert e.line == line, (defect, e.line, line, str(e))
        if line is not None:                                      # the very item that contains the line
            assert e.item == SMALL.words[line] // WORDS and (e.limb, e.word) == (0, 0), str(e)
    assert f"item {e.item}, limb {e.limb}, word {e.word}" in str(e)


def test_no_planted_defect_is_missed():
    """the share of missed defects is zero, over every tier and every wrap line, also with an item that is no power of two"""
    missed = []
    for tier, wrap in CROSSINGS:
        for words in (WORDS, 3 * 64):
            for defect in DEFECTS:
                try:
                    run(tier, wrap, defect, words=words)
                    missed.append((tier, wrap, words, defect))
                except wb.WideBatchError:
                    pass
    assert missed == []


def test_the_plan_refuses_an_even_period_and_why():
    """P = 2 and a power-of-two item: the truncated read fetches item i - 2^k, which has the parity of i - an equal item.  The output is right by accident
    and the checker cannot know; with P = 3 the same defect is named"""
    for period in (2, 4, 1, 0):
        with pytest.raises(AssertionError, match="odd"):
            wb.plan({"in": WORDS, "out": WORDS}, "A", period=period, lines=SMALL, writable=("out",))
    run("A", "B32", "read_truncated", period=2, planned=False)   # passes: the defect goes unseen
    with pytest.raises(wb.WideBatchError):
        run("A", "B32", "read_truncated", period=3)


def test_the_plan_holds_the_batch_to_the_entrys_limits_and_the_cap():
    with pytest.raises(AssertionError, match="exceeds the entry's limit"):
        wb.plan({"io": 8}, "A", lines=SMALL, limits=[("grid", lambda b: b * 4, 1000)])
    with pytest.raises(AssertionError, match="exceeds the cap"):
        wb.plan({"a": 1 << 13, "b": 1 << 13, "c": 1 << 14, "d": 1 << 14, "e": 1 << 14, "f": 1 << 14}, "A")
    pl = wb.plan({"a2": 1 << 14, "b2": 1 << 14, "out3": 3 << 13}, "A", writable=("out3",))       # the reference case: dpfhe_ct_mul at N = 4096, L = 2
    assert pl.batch == (1 << 15) + 2 and 14 << 30 < pl.peak < 16 << 30


def test_sampled_items_sit_on_every_line_of_every_buffer():
    pl = wb.plan({"small": 64, "large": 192}, "B", lines=SMALL)
    s = pl.sample_items()
    assert {0, 1, pl.batch - 2, pl.batch - 1} <= set(s)
    for words in (64, 192):
        for name in SMALL.of_tier("B"):
            at = SMALL.words[name] // words
            assert {at - 1, at, at + 1} <= set(s)
    out = wb.sentinel(pl.batch, 64, "cpu")
    o = out.numpy().view(np.uint64)
    o[: pl.batch] = np.arange(pl.batch, dtype=np.uint64)[:, None]
    wb.check_sampled("small", out, pl, lambda i: np.full(64, i, np.uint64))
    wb.check_no_sentinel("small", out, pl, 0, 64)
    at = SMALL.words["W31"] // 64
    o[at, 5] = np.uint64(wb.SENTINEL)
    with pytest.raises(wb.WideBatchError) as info:
        wb.check_sampled("small", out, pl, lambda i: np.full(64, i, np.uint64))
    assert (info.value.kind, info.value.item, info.value.word, info.value.line) == ("unwritten", at, 5, "W31")
    o[at, 5] = np.uint64(at)
    o[at + 7, 9] = np.uint64(wb.SENTINEL)                        # not a sampled item: only the device-side sentinel scan sees it
    wb.check_sampled("small", out, pl, lambda i: np.full(64, i, np.uint64))
    with pytest.raises(wb.WideBatchError) as info:
        wb.check_no_sentinel("small", out, pl, 0, 64)
    assert (info.value.item, info.value.word) == (at + 7, 9)


def test_reduction_reference_is_reps_times_the_period_plus_the_cut():
    pl = wb.plan({"in": 128}, "A", lines=SMALL)
    reps, cut = pl.reps_and_cut()
    assert reps * pl.period + cut == pl.batch and 0 <= cut < pl.period
    src = np.random.default_rng(3).integers(0, 1 << 40, (3, 128), dtype=np.uint64)
    t = wb.tile(src, pl.batch, "cpu").numpy().view(np.uint64)
    q = (1 << 59) - 55
    want = [(reps * sum(int(v) for v in src[:, w]) + sum(int(v) for v in src[:cut, w])) % q for w in range(128)]
    assert want == [sum(int(v) for v in t[:, w]) % q for w in range(128)]


# ---- the GPU module's cases, planned at the real lines -------------------------------------------------------------------------------------------------------
def _gpu_cases():
    import test_gpu_wide_batch as g
    return g.CASES


def test_every_gpu_case_is_within_its_limits_and_its_cap():
    cases = _gpu_cases()
    assert len({c.id for c in cases}) == len(cases)
    for c in cases:
        pl = c.plan()                                             # asserts the period, the entry's limits and the tier's cap
        assert pl.tier == c.tier and pl.peak <= wb.CAP[c.tier], c.id
        for name, words in pl.items.items():                      # every batched buffer ends two whole items past the highest line
            assert pl.batch * words >= wb.REAL.highest(c.tier) + 2 * words, (c.id, name)
    assert {c.tier for c in cases} == {"A", "B"}


def test_the_peaks_of_the_tier_b_cases_are_pinned():
    """a tier B case skips only when mem_get_info reports less than its peak + 8 GiB free: these are the peaks, in bytes"""
    import test_gpu_wide_batch as g
    got = {c.id: c.plan().peak for c in _gpu_cases() if c.tier == "B"}
    assert got == g.TIER_B_PEAKS, got
    assert wb.HEADROOM == 8 << 30 and wb.CAP == {"A": 24 << 30, "B": 70 << 30}
