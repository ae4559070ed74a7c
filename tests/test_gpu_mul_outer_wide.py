"""-m gpu: one dpfhe_ct_mul_outer call whose OUTPUT crosses 2^32 bytes, on tests/wide_batch.py's buffers and checks (the operands of an outer product stay
small: 148 items are 19 MiB; it is the A x B pairs that reach the line, and every index that places a pair must be 64-bit).

At N = 4096, L = 2 a pair is 3 L N words = 196 608 bytes: 148 x 148 pairs end 58 pairs past the 4 GiB line.  DPFHE_IN_NTT | DPFHE_OUT_NTT: the streaming
kernel alone, no scratch.  Queries and keys tile with period 3 from items whose 9 products the oracle gives (transformed by the oracle), so the output has
period 3 in both indices: pair (i, j) holds product (i mod 3, j mod 3).  A 32-bit wrap of a pair's offset moves it by 2^32 bytes = 21845.33 pairs - never a
whole pair, let alone one of equal residues - so a wrapped store leaves its own pair unwritten (the sentinel) and breaks another.  All compares run on the
device: the first 3 x 3 pairs against the reference, every row against the row three above it, every row against itself shifted by three pairs, and the
sentinel item behind the output."""
import numpy as np
import pytest

import wide_batch as wb
from class_edges import Rig
from deeppowers_amd import _cabi

pytestmark = pytest.mark.gpu

P, SIDE = 3, 148


def fail(r, v, i, j, want_row, what):
    """the first differing word of pair (i, j) against want_row [words] (a device tensor), as a WideBatchError that names the line it lies beyond"""
    words = v.shape[2]
    ne = (v[i, j] != want_row).nonzero()
    w = int(ne[0, 0])
    wb._raise("out3", "period", (i * SIDE + j) * words + w, words, r.n, wb.REAL, wb._u64(v[i, j, w]), wb._u64(want_row[w]), what)


def test_output_crosses_the_4_gib_line():
    import torch
    r = Rig("fold2", 12)
    try:
        lib, h, orc, L, n = r.ctx._lib, r.ctx.handle, r.orc, r.L, r.n
        assert (L, n) == (2, 4096)
        words, pairs = 3 * L * n, SIDE * SIDE
        assert (pairs - 2) * words * 8 >= 1 << 32 and SIDE > 2 * P           # two whole pairs past the line at least
        wb.check_period(P)
        ntt = lambda v: orc.ntt_fwd(np.ascontiguousarray(v).reshape(-1, L, n), threads=0).reshape(v.shape)
        a, b = r.words(orc, (P, 2), 1300), r.words(orc, (P, 2), 1310)
        pa = np.ascontiguousarray(np.broadcast_to(a[:, None], (P, P) + a.shape[1:])).reshape(P * P, 2, L, n)
        pb = np.ascontiguousarray(np.broadcast_to(b[None], (P, P) + b.shape[1:])).reshape(P * P, 2, L, n)
        want = ntt(orc.ct_mul(pa, pb, threads=0)).reshape(P, P, words)       # product (i, j) of the period, NTT domain
        ta, tb = wb.tile(ntt(a), SIDE, r.ctx.device), wb.tile(ntt(b), SIDE, r.ctx.device)
        out = wb.sentinel(pairs, words, r.ctx.device)
        flags = _cabi.IN_NTT | _cabi.OUT_NTT
        _cabi.check(lib.dpfhe_ct_mul_outer(h, out.data_ptr(), ta.data_ptr(), tb.data_ptr(), SIDE, SIDE, flags, None), "dpfhe_ct_mul_outer")
        torch.cuda.synchronize()
        v = out[:pairs].view(SIDE, SIDE, words)
        dwant = torch.from_numpy(want.view(np.int64)).to(r.ctx.device)
        for i in range(P):
            for j in range(P):
                if not torch.equal(v[i, j], dwant[i, j]):
                    fail(r, v, i, j, dwant[i, j], "differs from the reference in the first period")
        for i in range(SIDE):
            if not torch.equal(v[i, P:], v[i, :-P]):                          # periodic in the key
                j = P + int((v[i, P:] != v[i, :-P]).any(dim=1).nonzero()[0, 0])
                fail(r, v, i, j, v[i, j - P], f"pair (i, j) differs from pair (i, j - {P})")
            if i >= P and not torch.equal(v[i], v[i - P]):                    # periodic in the query
                j = int((v[i] != v[i - P]).any(dim=1).nonzero()[0, 0])
                fail(r, v, i, j, v[i - P, j], f"pair (i, j) differs from pair (i - {P}, j)")
        wb.check_tail_row("out3", out, r.n)
        wb.check_input("a", ta, wb.Plan({"a": 2 * L * n}, "A", SIDE, P, wb.REAL, 0), ntt(a), r.n)
        wb.check_input("b", tb, wb.Plan({"b": 2 * L * n}, "A", SIDE, P, wb.REAL, 0), ntt(b), r.n)
        del v, out, ta, tb
    finally:
        r.close()
        wb.release()
