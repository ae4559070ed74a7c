"""The memory footprint of one call: every pointer argument carved out of ONE contiguous uint64 array, so that what the call wrote - and what it must not
have touched - is read off a single download.  A plain helper like tests/class_edges.py (no conftest, no plugin); tests/test_footprint_cpu.py shows on
stand-in kernels that it reports every kind of fault, tests/test_gpu_footprint.py runs the device entry points of include/dpfhe.h through it.

  Arena.carve(name, words, role, item_words, data=...)   a buffer of `words` words; role 'input' | 'output' | 'scratch' | 'inout'
  Arena.fill(pattern)                                    the array: `pattern` in every word that is not input data; a snapshot of it is kept
  Arena.verify(after)                                    every word outside the output / scratch / inout regions is bit-identical to the snapshot
  Arena.check_outputs(after, expected)                   the named regions equal `expected` word for word; an unwritten word is named as such
  run_both_patterns(arena, call, expected)               the whole check, once per pattern

What carve itself asserts (conditions, not tuned numbers):
  * a guard band on BOTH sides of every buffer of at least one whole item of that buffer (item_words: 2 L N for a 2-component ciphertext item) and never
    fewer than MIN_GUARD = 512 words - a kernel that overshoots by one tile, one polynomial or one item lands in a guard;
  * the weakest alignment the C ABI admits: a word offset that is 2 mod 4 (16-byte aligned, NOT 32-byte aligned), or, with align=8 (d_w of
    dpfhe_matvec_scalar, documented as 8-byte aligned), an odd word offset.  Arena.address() asserts the base is 32-byte aligned, so the offsets hold
    for the addresses too.
A strided buffer (the item strides of dpfhe_base_extend / dpfhe_scale_round) is carved with segments=[(offset, words), ...]: only the segments have the
role, the stride gaps between them are guards.

The two patterns are SENTINEL = 0xDEADBEEFCAFEF00D and its complement 0x2152411035010FF2.  Both are >= 2^60 and every admissible prime is < 2^60, so
neither is a canonical residue: a word the kernel failed to write can never equal an oracle word.  A result that equals the oracle under BOTH patterns
does not depend on what its scratch and output buffers held before the call."""
import numpy as np

SENTINEL = np.uint64(0xDEADBEEFCAFEF00D)
PATTERNS = (SENTINEL, ~SENTINEL)
assert all(int(p) >= 1 << 60 for p in PATTERNS) and int(PATTERNS[0]) ^ int(PATTERNS[1]) == (1 << 64) - 1
MIN_GUARD = 512
ROLES = ("input", "output", "scratch", "inout")
WRITABLE = ("output", "scratch", "inout")


class FootprintError(AssertionError):
    """a violated footprint: .buffer names the carved buffer, .kind is 'before' | 'after' | 'gap' | 'input' | 'unwritten' | 'wrong'"""

    def __init__(self, buffer, kind, first, last, message):
        super().__init__(message)
        self.buffer, self.kind, self.first, self.last = buffer, kind, first, last


class _Region:
    def __init__(self, name, offset, words, role, item_words, guard, data, segments):
        self.name, self.offset, self.words, self.role, self.item_words, self.guard = name, offset, words, role, item_words, guard
        self.data, self.segments = data, segments


class Arena:
    def __init__(self):
        self.regions = {}
        self.total = 0
        self._snapshot = None
        self._pattern = None

    # ---- layout -----------------------------------------------------------------------------------------------------------------------------------------
    def carve(self, name, words, role, item_words, data=None, segments=None, align=16, guard=None, offset=None):
        """`guard` and `offset` default to the smallest admissible values; given explicitly they are held to the same conditions"""
        words, item_words = int(words), int(item_words)
        assert role in ROLES, role
        assert name not in self.regions, f"{name}: carved twice"
        assert words > 0 and item_words > 0, (name, words, item_words)
        need = max(item_words, MIN_GUARD)
        g = need if guard is None else int(guard)
        assert g >= need, f"{name}: a guard of {g} words is shorter than one item ({item_words} words) or than {MIN_GUARD} words"
        if offset is None:
            offset = self.total + g
            while not self._weakest(offset, align):
                offset += 1
        assert offset - self.total >= g, f"{name}: offset {offset} leaves a guard of {offset - self.total} words, needs {g}"
        assert self._weakest(offset, align), (f"{name}: word offset {offset} is not the weakest legal alignment "
                                               f"({'odd' if align == 8 else '2 mod 4: 16-byte aligned and not 32-byte aligned'})")
        if segments is None:
            segments = [(0, words)]
        segments = [(int(o), int(w)) for o, w in segments]
        end = 0
        for o, w in segments:
            assert o >= end and w > 0 and o + w <= words, f"{name}: segments must be ascending, disjoint and inside the buffer"
            end = o + w
        if role in ("input", "inout"):
            assert data is not None, f"{name}: an {role} buffer needs its data"
            data = np.ascontiguousarray(data, dtype=np.uint64).ravel()
            assert data.size == sum(w for _, w in segments), f"{name}: {data.size} data words for {sum(w for _, w in segments)} words of segments"
        else:
            assert data is None, f"{name}: an {role} buffer takes no data"
        self.regions[name] = _Region(name, offset, words, role, item_words, g, data, segments)
        self.total = offset + words + g
        return offset

    @staticmethod
    def _weakest(offset, align):
        assert align in (8, 16), align
        return offset % 2 == 1 if align == 8 else offset % 4 == 2

    def offset(self, name):
        return self.regions[name].offset

    def address(self, base, name, extra_words=0):
        """the byte address of buffer `name` in an upload of the array that starts at `base`"""
        assert base % 32 == 0, "the array's base must be 32-byte aligned for the carved offsets to be the weakest alignment"
        return base + 8 * (self.regions[name].offset + extra_words)

    # ---- fill and verify --------------------------------------------------------------------------------------------------------------------------------
    def fill(self, pattern):
        raw = np.empty(self.total + 8, dtype=np.uint64)            # (a 64-byte aligned start, so that host addresses keep the carved alignment too)
        skip = (-raw.ctypes.data % 64) // 8
        buf = raw[skip: skip + self.total]
        buf[:] = np.uint64(pattern)
        for r in self.regions.values():
            if r.data is not None:
                at = 0
                for o, w in r.segments:
                    buf[r.offset + o: r.offset + o + w] = r.data[at: at + w]
                    at += w
        self._snapshot, self._pattern = buf.copy(), np.uint64(pattern)
        return buf

    def _protected(self):
        """(start, stop, buffer, kind) of every stretch the call may not change, in address order"""
        out, regs = [], sorted(self.regions.values(), key=lambda r: r.offset)
        for i, r in enumerate(regs):
            out.append((r.offset - r.guard, r.offset, r, "before"))
            at = 0
            for o, w in r.segments:
                if o > at:
                    out.append((r.offset + at, r.offset + o, r, "gap"))
                if r.role not in WRITABLE:
                    out.append((r.offset + o, r.offset + o + w, r, "input"))
                at = o + w
            if at < r.words:
                out.append((r.offset + at, r.offset + r.words, r, "gap"))
            out.append((r.offset + r.words, r.offset + r.words + r.guard, r, "after"))
            # alignment padding between this buffer's guard and the next one's belongs to the nearer buffer
            nxt = regs[i + 1].offset - regs[i + 1].guard if i + 1 < len(regs) else self.total
            if nxt > r.offset + r.words + r.guard:
                out.append((r.offset + r.words + r.guard, nxt, r, "after"))
        first = regs[0].offset - regs[0].guard if regs else 0
        if first > 0:
            out.append((0, first, regs[0], "before"))
        return out

    def verify(self, after):
        """raises FootprintError naming the buffer, the side and the first and last changed word (offsets relative to the buffer's start)"""
        assert self._snapshot is not None, "fill() first"
        after = np.asarray(after)
        assert after.dtype == np.uint64 and after.shape == self._snapshot.shape, (after.dtype, after.shape)
        for a, b, r, kind in self._protected():
            bad = np.flatnonzero(after[a:b] != self._snapshot[a:b])
            if bad.size:
                first, last = a + int(bad[0]) - r.offset, a + int(bad[-1]) - r.offset
                what = {"before": "guard before the buffer", "after": "guard past the end", "gap": "stride gap", "input": "input words"}[kind]
                raise FootprintError(r.name, kind, first, last,
                                     f"{r.name} ({r.role}, {r.words} words): {what} changed: {bad.size} words, first at offset {first}, last at offset {last} "
                                     f"(relative to the buffer; word there now {int(after[r.offset + first]):#x})")

    def view(self, buf, name):
        """the words of buffer `name` (its segments back to back) in `buf`"""
        r = self.regions[name]
        return np.concatenate([buf[r.offset + o: r.offset + o + w] for o, w in r.segments]) if len(r.segments) > 1 else \
            buf[r.offset + r.segments[0][0]: r.offset + r.segments[0][0] + r.segments[0][1]]

    def check_outputs(self, after, expected):
        """expected: name -> the words the region must hold after the call"""
        for name, want in expected.items():
            r = self.regions[name]
            assert r.role in WRITABLE, f"{name}: expected words for a buffer the call may not write"
            want = np.ascontiguousarray(want, dtype=np.uint64).ravel()
            got = self.view(np.asarray(after), name)
            assert got.size == want.size, (name, got.size, want.size)
            bad = np.flatnonzero(got != want)
            if bad.size:
                first, last = int(bad[0]), int(bad[-1])
                unwritten = int(np.count_nonzero(got[bad] == self._pattern))
                kind = "unwritten" if got[first] == self._pattern else "wrong"
                raise FootprintError(name, kind, first, last,
                                     f"{name} ({r.role}): {bad.size} of {want.size} words differ from the reference under pattern {int(self._pattern):#x}, first at word "
                                     f"{first} (got {int(got[first]):#x}, want {int(want[first]):#x}), last at word {last}; {unwritten} of them still hold the "
                                     f"fill pattern (left unwritten)")


def run_both_patterns(arena, call, expected):
    """call(buf) runs the operation on the array (in place, or on a copy it returns) and returns the array afterwards.  Under each of the two fill
    patterns: verify, then the expected words.  Returns the two arrays."""
    results = []
    for pattern in PATTERNS:
        buf = arena.fill(pattern)
        after = call(buf)
        after = buf if after is None else after
        arena.verify(after)
        arena.check_outputs(after, expected)
        results.append(after)
    return results
