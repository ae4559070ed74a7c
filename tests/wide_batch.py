"""Batches whose buffers cross the 4 GiB line (and the 2^31 / 2^32 word lines): the plan of such a batch and the check of what a call made of it.
A plain helper like tests/footprint.py (no conftest, no plugin, no GPU mark of its own: torch calls only, on whatever device the tensors live).
tests/test_wide_batch_cpu.py shows on numpy model kernels at a scaled-down line that the check names every planted 32-bit defect;
tests/test_gpu_wide_batch.py runs the device entry points of include/dpfhe.h through it at the real lines.

The lines (Lines(b31) scales all four together; REAL = Lines(2^31)):
  B31 = 2^31 bytes    B32 = 2^32 bytes    W31 = 2^31 words = 8 B32    W32 = 2^32 words = 16 B32
Tier 'A' crosses the two byte lines, tier 'B' all four.

  plan(items, tier, ...)   items: name -> words per item of every BATCHED buffer of the call.  The batch is the one at which the SMALLEST batched
                           buffer ends at least two whole items past the tier's highest line - so every batched pointer of the call crosses it, reads
                           as well as writes.  The period P of the tiling must be odd and >= 3 (asserted): a 32-bit wrap moves an access by 2^29 or
                           2^32 words, a power-of-two number of items whenever the item is a power of two words, and 2^k is never 0 mod an odd P > 1 -
                           the wrapped access lands on an item of another residue mod P, which holds other words.  The entry's own limits (the launch
                           grid, first_item + batch <= 2^32) are asserted through `limits`, a list of (what, value, bound).
  tile(period, batch)      P distinct items, uploaded, tiled on the device (repeat, cut to batch): nothing of the large size exists on the host
  sentinel(batch, words)   a writable buffer: batch + 1 items of 0xDEADBEEFCAFEF00D (>= 2^60: no residue), the last one the tail
  check_output / check_input / check_sampled / check_no_sentinel: see each; every compare runs on the device in slices of at most SLICE_WORDS words
                           (1 GiB), and a wrong word is a WideBatchError with the first differing (buffer, item, limb, word) and the line it lies beyond.
"""
import numpy as np

SENTINEL = 0xDEADBEEFCAFEF00D
assert SENTINEL >= 1 << 60
_SENT_I64 = SENTINEL - (1 << 64)          # the same bits as a torch int64
SLICE_WORDS = 1 << 27                     # 1 GiB of words per device compare
TIERS = ("A", "B")
CAP = {"A": 24 << 30, "B": 70 << 30}      # peak device bytes of one case (at the real lines)
HEADROOM = 8 << 30                        # a tier B case runs only with this much free memory beyond its peak: the card is shared
COMPARE_BYTES = 3 * SLICE_WORDS           # temporaries of one sliced compare: a bool per word and the index of the first difference, with room


class Lines:
    """the four lines in words, scaled by b31 (bytes)"""

    def __init__(self, b31=1 << 31):
        assert b31 >= 64 and b31 & (b31 - 1) == 0, b31
        self.b31 = b31
        self.words = {"B31": b31 // 8, "B32": b31 // 4, "W31": b31, "W32": 2 * b31}

    def of_tier(self, tier):
        assert tier in TIERS, tier
        return ("B31", "B32") if tier == "A" else ("B31", "B32", "W31", "W32")

    def highest(self, tier):
        return self.words[self.of_tier(tier)[-1]]

    def beyond(self, word):
        """the name of the highest line at or below word offset `word` (None below B31)"""
        best = None
        for name in ("B31", "B32", "W31", "W32"):
            if word >= self.words[name]:
                best = name
        return best


REAL = Lines()


class Plan:
    def __init__(self, items, tier, batch, period, lines, peak):
        self.items, self.tier, self.batch, self.period, self.lines, self.peak = dict(items), tier, batch, period, lines, peak

    def reps_and_cut(self):
        """batch = reps * period + cut: a reduction over the tiled batch is reps x (sum of the period) + (sum of the first `cut` items)"""
        return divmod(self.batch, self.period)

    def sample_items(self):
        """the items an aperiodic entry is held to its host twin on: the first two, the last two and, for each line crossed, the item that contains the
        line in each batched buffer with both its neighbours"""
        s = {0, 1, self.batch - 2, self.batch - 1}
        for words in self.items.values():
            for name in self.lines.of_tier(self.tier):
                at = self.lines.words[name] // words
                s.update(i for i in (at - 1, at, at + 1) if 0 <= i < self.batch)
        return sorted(s)


def check_period(period):
    assert isinstance(period, int) and period >= 3 and period % 2 == 1, (
        f"period {period}: the tiling period must be odd and >= 3 - a 32-bit wrap moves an access by a power-of-two number of items, which an even "
        f"period can divide: the wrapped access would land on an equal item and go unseen")


def plan(items, tier, period=3, lines=REAL, writable=(), extra_bytes=0, limits=(), cap=None, margin=2, low_items=None):
    """low_items: name -> words per item of batched buffers that, at the batch the `items` fix, must end `margin` items past the LOWEST line (B31) only - for
    calls whose buffers cannot all cross the highest line within the cap; the plan asserts that they do cross B31, and they count in the peak;
    margin: whole items past the line (>= 2; a launcher that works in slices of s items needs 2 s, so that a slice BASE lies past the line too);
    items: name -> words per item of every batched buffer; writable: the names that carry a sentinel tail item (outputs and in-out buffers);
    extra_bytes: what the case holds besides (shared operands, scratch the entry leases); limits: (what, value(batch), bound) the entry documents"""
    check_period(period)
    assert items and all(int(w) > 0 for w in items.values()), items
    smallest = min(int(w) for w in items.values())
    assert margin >= 2, margin
    batch = -(-lines.highest(tier) // smallest) + margin
    assert batch * smallest >= lines.highest(tier) + margin * smallest
    assert batch > 2 * period, (batch, period)
    low_items = dict(low_items or {})
    assert not set(low_items) & set(items) and set(writable) <= set(items) | set(low_items), (low_items, items, writable)
    for name, w in low_items.items():
        lowest = lines.words[lines.of_tier(tier)[0]]
        assert batch * int(w) >= lowest + margin * int(w), f"{name}: {batch} items of {w} words do not end {margin} items past {lines.of_tier(tier)[0]}"
    for what, value, bound in limits:
        v = value(batch) if callable(value) else value
        assert v <= bound, f"{what}: {v} exceeds the entry's limit {bound} at batch {batch}"
    peak = sum((batch + (1 if name in writable else 0)) * int(w) * 8 for name, w in {**items, **low_items}.items()) + int(extra_bytes) + COMPARE_BYTES
    if cap is None:
        cap = CAP[tier] if lines is REAL else None
    if cap is not None:
        assert peak <= cap, f"tier {tier}: a peak of {peak} bytes ({peak / 2**30:.1f} GiB) exceeds the cap of {cap} bytes: shrink the case"
    pl = Plan(items, tier, batch, period, lines, peak)
    pl.low_items = low_items
    return pl


# ---- device buffers ------------------------------------------------------------------------------------------------------------------------------------------
def _i64(a):
    return np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)


def tile_into(out, period_items, batch):
    """fills rows [0, batch) of the device tensor `out` [>= batch][words] with the tiling of period_items [P][words]: in place, no second copy of the large size"""
    import torch
    p = np.ascontiguousarray(period_items, dtype=np.uint64)
    p = p.reshape(p.shape[0], -1)
    P, words = p.shape
    assert out.shape[0] >= batch and out.shape[1] == words, (out.shape, batch, words)
    t = torch.from_numpy(_i64(p)).to(out.device)
    reps, cut = divmod(batch, P)
    out[: reps * P].view(reps, P, words).copy_(t.unsqueeze(0).expand(reps, P, words))
    if cut:
        out[reps * P: batch].copy_(t[:cut])
    return out


def tile(period_items, batch, device):
    """period_items [P][...] (uint64) -> a device tensor [batch][words]: item i holds period item i mod P"""
    import torch
    p = np.ascontiguousarray(period_items, dtype=np.uint64)
    p = p.reshape(p.shape[0], -1)
    return tile_into(torch.empty((batch, p.shape[1]), dtype=torch.int64, device=device), p, batch)


def sentinel(batch, words, device):
    """[batch + 1][words] of the sentinel: the buffer and, behind it, one item of tail"""
    import torch
    return torch.full((batch + 1, words), _SENT_I64, dtype=torch.int64, device=device)


class WideBatchError(AssertionError):
    """.buffer, .kind ('reference' | 'period' | 'tail' | 'input' | 'unwritten' | 'sample'), .item, .limb, .word, .line"""

    def __init__(self, buffer, kind, item, limb, word, line, message):
        super().__init__(message)
        self.buffer, self.kind, self.item, self.limb, self.word, self.line = buffer, kind, item, limb, word, line


def _raise(name, kind, flat_word, words, limb_words, lines, got, want, what, base=0):
    flat_word = int(flat_word) + base
    item, inside = divmod(int(flat_word), words)
    limb, word = divmod(inside, limb_words) if limb_words else (0, inside)
    line = lines.beyond(int(flat_word))
    unwritten = " (the sentinel: never written)" if int(got) == SENTINEL else ""
    raise WideBatchError(name, kind, item, limb, word, line,
                         f"{name}: {what}: first at item {item}, limb {limb}, word {word} (flat word {int(flat_word)}, "
                         f"{'beyond ' + line if line else 'below every line'}): got {int(got):#x}{unwritten}, want {int(want):#x}")


def _u64(v):
    return int(v) & ((1 << 64) - 1)


def _first_diff(a, b):
    """index of the first differing word of two equal-length flat tensors (or of a tensor and a scalar), None if equal; one slice at a time"""
    import torch
    n = a.numel()
    for s in range(0, n, SLICE_WORDS):
        e = min(n, s + SLICE_WORDS)
        x = a[s:e]
        y = b[s:e] if isinstance(b, torch.Tensor) else b
        ne = x != y
        if bool(ne.any()):
            return s + int(ne.nonzero()[0, 0])
        del ne
    return None


def _check_first_period(name, kind, t, first, words, limb_words, lines, what, base=0):
    first = np.ascontiguousarray(first, dtype=np.uint64).reshape(-1)
    got = t[: first.size // words].reshape(-1).cpu().numpy().view(np.uint64)
    assert got.size == first.size, (name, got.size, first.size)
    bad = np.flatnonzero(got != first)
    if bad.size:
        kind = "unwritten" if kind == "reference" and int(got[bad[0]]) == SENTINEL else kind
        _raise(name, kind, bad[0], words, limb_words, lines, got[bad[0]], first[bad[0]], what, base)


def _check_periodic(name, kind, t, batch, period, words, limb_words, lines, what, base=0):
    flat = t.reshape(-1)
    shift = period * words
    at = _first_diff(flat[shift: batch * words], flat[: batch * words - shift])
    if at is not None:
        got, want = _u64(flat[shift + at]), _u64(flat[at])
        _raise(name, "unwritten" if got == SENTINEL else kind, shift + at, words, limb_words, lines, got, want, what, base)


def check_output(name, t, pl, want_period, limb_words=0, lines=None):
    """(a) the first P items equal the reference word for word; (b) item i equals item i - P for every i >= P; (c) the tail item is all sentinel.
    t: [batch + 1][words] as sentinel() made it; want_period: [P][words]"""
    lines = lines or pl.lines
    words = t.shape[1]
    assert t.shape[0] == pl.batch + 1, (name, t.shape, pl.batch)
    _check_first_period(name, "reference", t, want_period, words, limb_words, lines, "differs from the reference in the first period")
    _check_periodic(name, "period", t, pl.batch, pl.period, words, limb_words, lines, f"item i differs from item i - {pl.period}")
    check_tail(name, t, pl, limb_words, lines)


def check_small_output(name, t, want, limb_words=0, lines=REAL):
    """an output that is NOT batched (the sum of a reduction): t [items + 1][words] as sentinel() made it equals `want` [items][words], tail untouched"""
    words = t.shape[1]
    want = np.ascontiguousarray(want, dtype=np.uint64).reshape(-1, words)
    assert t.shape[0] == want.shape[0] + 1, (name, t.shape, want.shape)
    _check_first_period(name, "reference", t, want, words, limb_words, lines, "differs from the reference")
    at = _first_diff(t[-1].reshape(-1), _SENT_I64)
    if at is not None:
        _raise(name, "tail", want.size + at, words, limb_words, lines, _u64(t[-1].reshape(-1)[at]), SENTINEL, "the sentinel tail behind the buffer changed")


def check_stretch(name, t, start, count, period, want_period, limb_words=0, lines=REAL):
    """an output made of several stretches, each periodic on its own (block 0 and the rotations of a rotation-major output; the products and the self
    products): items [start, start + count) of t - the first `period` equal want_period word for word, item i equals item i - period; a stretch shorter
    than a period is compared whole.  The caller checks the tail (check_tail_row)"""
    words = t.shape[1]
    v = t[start: start + count]
    want = np.ascontiguousarray(want_period, dtype=np.uint64).reshape(-1, words)[:count]
    _check_first_period(name, "reference", v, want, words, limb_words, lines, "differs from the reference in the first period of its stretch", start * words)
    if count > period:
        _check_periodic(name, "period", v, count, period, words, limb_words, lines, f"item i differs from item i - {period}", start * words)


def check_tail_row(name, t, limb_words=0, lines=REAL):
    """the last item of t (the tail sentinel() put behind the buffer) is untouched"""
    words = t.shape[1]
    at = _first_diff(t[-1].reshape(-1), _SENT_I64)
    if at is not None:
        _raise(name, "tail", (t.shape[0] - 1) * words + at, words, limb_words, lines, _u64(t[-1].reshape(-1)[at]), SENTINEL, "the sentinel tail behind the buffer changed")


def check_columns(name, t, pl, lo, hi, first_period=None, limb_words=0, lines=None):
    """words [lo, hi) of every item (a component the call must not write), over the WHOLE buffer, a slice of items at a time: all sentinel when first_period
    is None; otherwise equal to first_period [P][hi - lo] in the first period and periodic after it"""
    lines = lines or pl.lines
    words, P = t.shape[1], pl.period
    step = max(1, SLICE_WORDS // (hi - lo))
    if first_period is not None:
        want = np.ascontiguousarray(first_period, dtype=np.uint64).reshape(P, hi - lo)
        got = t[:P, lo:hi].cpu().numpy().view(np.uint64)
        bad = np.argwhere(got != want)
        if bad.size:
            r, c = (int(v) for v in bad[0])
            _raise(name, "input", r * words + lo + c, words, limb_words, lines, got[r, c], want[r, c], "a component the call must not write changed in its first period")
    for s in range(P if first_period is not None else 0, pl.batch, step):
        e = min(pl.batch, s + step)
        part = t[s:e, lo:hi]
        ne = part != (t[s - P: e - P, lo:hi] if first_period is not None else _SENT_I64)
        if bool(ne.any()):
            r, c = (int(v) for v in ne.nonzero()[0])
            _raise(name, "input", (s + r) * words + lo + c, words, limb_words, lines, _u64(part[r, c]), SENTINEL if first_period is None else _u64(t[s + r - P, lo + c]),
                   "a component the call must not write changed")
        del ne


def check_tail(name, t, pl, limb_words=0, lines=None):
    lines = lines or pl.lines
    words = t.shape[1]
    at = _first_diff(t[pl.batch].reshape(-1), _SENT_I64)
    if at is not None:
        _raise(name, "tail", pl.batch * words + at, words, limb_words, lines, _u64(t[pl.batch].reshape(-1)[at]), SENTINEL, "the sentinel tail behind the buffer changed")


def check_input(name, t, pl, period_items, limb_words=0, lines=None):
    """(d) an input is still periodic and its first period is bit-identical to what was uploaded"""
    lines = lines or pl.lines
    words = t.shape[1]
    assert t.shape[0] == pl.batch, (name, t.shape, pl.batch)
    _check_first_period(name, "input", t, period_items, words, limb_words, lines, "an input changed in its first period")
    _check_periodic(name, "input", t, pl.batch, pl.period, words, limb_words, lines, "an input changed: it is no longer periodic")


def check_sampled(name, t, pl, want_of_item, limb_words=0, lines=None):
    """the aperiodic entries: item i equals want_of_item(i) (the host twin) on pl.sample_items()"""
    lines = lines or pl.lines
    words = t.shape[1]
    for i in pl.sample_items():
        want = np.ascontiguousarray(want_of_item(i), dtype=np.uint64).reshape(-1)
        got = t[i].reshape(-1).cpu().numpy().view(np.uint64)
        assert got.size == want.size, (name, got.size, want.size)
        bad = np.flatnonzero(got != want)
        if bad.size:
            kind = "unwritten" if int(got[bad[0]]) == SENTINEL else "sample"
            _raise(name, kind, i * words + int(bad[0]), words, limb_words, lines, got[bad[0]], want[bad[0]], "differs from the host twin")


def check_no_sentinel(name, t, pl, lo, hi, limb_words=0, lines=None):
    """the samplers: no word of words [lo, hi) of any item (the written component) still holds the sentinel; one slice of items at a time"""
    lines = lines or pl.lines
    words = t.shape[1]
    step = max(1, SLICE_WORDS // (hi - lo))
    for s in range(0, pl.batch, step):
        part = t[s: min(pl.batch, s + step), lo:hi]
        eq = part == _SENT_I64
        if bool(eq.any()):
            r, c = (int(v) for v in eq.nonzero()[0])
            _raise(name, "unwritten", (s + r) * words + lo + c, words, limb_words, lines, SENTINEL, 0, "a word of the written component still holds the sentinel")
        del eq


def free_bytes():
    import torch
    return torch.cuda.mem_get_info()


def release():
    import gc
    import torch
    gc.collect()
    torch.cuda.empty_cache()
