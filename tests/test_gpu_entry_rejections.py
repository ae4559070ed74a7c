"""-m gpu: the argument checks of the device entries of include/dpfhe.h, one table per family: an accepted call at the smallest shape (returns 0), then
one call per `return fail(...)` branch that a live context can reach - misaligned buffer, each overlap pair, unknown flag, bad Galois element, shape
mismatch, invalid state - held to the return code AND to the whole dpfhe_last_error() text ("<what>: <detail>"), because most branches share the code
2000 and only the text says WHICH check answered: the first failing check decides both.  The expected values are read from the source, not from a run.

Contexts (tests/test_gpu_footprint.py ParamsRig): the pinned primes at log2 N = 8 with L = 3 (the smallest extended context that still has a limb to
drop) for every case; L = 1 for the DPFHE_INVALID_STATE branches and L = 2 for the one of them that needs an extended context with nothing left to drop;
log2 N = 14, L = 3 for the entries that take another path above the fused limit (dpfhe_rotate_hybrid_hoisted accepts null d_work / d_rotated0 there);
log2 N = 12, L = 1 for dpfhe_ctx_autotune and dpfhe_ctx_set_ct_mul_variant, which have nothing to choose at any other ring degree.

Two classes of branch are left out on purpose.  A check of either class that went missing would turn into a wild launch, not into a wrong return code,
and this file must never be able to fault a machine:
  * null buffers - in almost every entry the null test and the misalignment test are ONE condition (`!p || misaligned(p)`), which the misaligned case
    (base + 8 bytes inside a live allocation) exercises; a null context is covered on the CPU (tests/test_cabi_cpu.py);
  * "too large for one launch".
One branch has no case because no exported entry reaches it: "batch must be n_elts * group" of the rotations' shared body - dpfhe_rotate_hybrid_batch
passes n_elts = batch with group 1, dpfhe_rotate_hybrid_grouped passes batch = n_elts * group, and group = 0 is an empty batch, which returns 0 first.
Every pointer of every call, accepted or rejected, points into a live allocation large enough for the call had it run: each context has one pool of
equal regions of 64 L N words, more than any buffer of any call below."""
import numpy as np
import pytest

import fused_rescale_ref as fr
import test_gpu_footprint as fp
from deeppowers_amd.params import ntt_primes

pytestmark = pytest.mark.gpu

ARG, STATE = 2000, 2002       # DPFHE_INVALID_ARGUMENT, DPFHE_INVALID_STATE
REGIONS, REGION_ITEMS = 10, 64
SENTINEL = 0x5EADBEEFCAFEF00D

EXTENDED = "the extended context needs at least one data limb and the special prime"
GALOIS = "galois elements must be odd and < 2N"
BUF = "null or misaligned buffer"


class Ctx:
    """a context, its pool of device regions and the checker"""

    def __init__(self, name, p):
        import torch
        self.rig = fp.ParamsRig(name, p)
        r = self.rig
        self.lib, self.h, self.L, self.Ld, self.n = r.ctx._lib, r.ctx.handle, r.L, r.L - 1, r.n
        self.region_words = REGION_ITEMS * self.L * self.n
        self.pool = torch.zeros(REGIONS * self.region_words, dtype=torch.int64, device=r.ctx.device)
        assert self.pool.data_ptr() % 32 == 0
        self.R = [self.pool.data_ptr() + 8 * i * self.region_words for i in range(REGIONS)]
        self.name = name

    def ok(self, what, rc):
        assert rc == 0, f"{what} on {self.name}: an accepted call returned {rc}: {self.lib.dpfhe_last_error().decode()}"

    def no(self, what, detail, rc, code=ARG):
        text = self.lib.dpfhe_last_error().decode() if rc else ""
        assert (rc, text) == (code, f"{what}: {detail}"), f"on {self.name}: want {code} '{what}: {detail}', got {rc} '{text}'"

    def each_misaligned(self, what, detail, f, ptrs, off=8):
        """f(*ptrs) with each pointer in turn `off` bytes past its region's start"""
        for i in range(len(ptrs)):
            self.no(what, detail, f(*[p + off if j == i else p for j, p in enumerate(ptrs)]))

    def close(self):
        import torch
        torch.cuda.synchronize()
        del self.pool
        self.rig.close()


@pytest.fixture(scope="module")
def ctxs():
    made = {}
    params = {"n256_l3": lambda: fr.pinned(8, 3), "n256_l1": lambda: fr.pinned(8, 1), "n256_l2": lambda: fr.pinned(8, 2),
              "n16384_l3": lambda: ntt_primes(14, 3), "n4096_l1": lambda: fr.pinned(12, 1)}

    def get(name):
        if name not in made:
            made[name] = Ctx(name, params[name]())
        return made[name]
    yield get
    for c in made.values():
        c.close()


BOTH = ["n256_l3", "n16384_l3"]


# ---- transforms and coefficient-wise entries -------------------------------------------------------------------------------------------------------------
def test_transforms(ctxs):
    x = ctxs("n256_l3")
    lib, h, R = x.lib, x.h, x.R
    for f in (lib.dpfhe_ntt_fwd, lib.dpfhe_ntt_inv):
        x.ok("ntt", f(h, R[0], 1, None))
        x.no("ntt", BUF, f(h, R[0] + 8, 1, None))
    for f in (lib.dpfhe_ntt_fwd_oop, lib.dpfhe_ntt_inv_oop):
        x.ok("ntt", f(h, R[0], R[1], 1, None))
        x.each_misaligned("ntt", BUF, lambda o, i: f(h, o, i, 1, None), (R[0], R[1]))


def test_dyadic_family(ctxs):
    x = ctxs("n256_l3")
    lib, h, R = x.lib, x.h, x.R
    for f in (lib.dpfhe_dyadic_mul, lib.dpfhe_dyadic_mul_add, lib.dpfhe_add, lib.dpfhe_sub, lib.dpfhe_multiply_plain):
        x.ok("dyadic", f(h, R[0], R[1], R[2], 1, None))
        x.ok("dyadic", f(h, R[0], R[0], R[1], 1, None))            # in place is legal
        x.each_misaligned("dyadic", BUF, lambda o, a, b: f(h, o, a, b, 1, None), (R[0], R[1], R[2]))
    x.ok("dyadic", lib.dpfhe_negate(h, R[0], R[1], 1, None))
    x.each_misaligned("dyadic", BUF, lambda o, a: lib.dpfhe_negate(h, o, a, 1, None), (R[0], R[1]))


def test_copy(ctxs):
    x = ctxs("n256_l3")
    f, h, R, w = x.lib.dpfhe_copy, x.h, x.R, "dpfhe_copy"
    x.ok(w, f(h, R[0], R[1], 2, None))
    x.each_misaligned(w, "null or misaligned buffer, or an odd word count", lambda d, s: f(h, d, s, 2, None), (R[0], R[1]))
    x.no(w, "null or misaligned buffer, or an odd word count", f(h, R[0], R[1], 3, None))
    x.no(w, "buffers overlap", f(h, R[0] + 16, R[0], 4, None))
    x.no(w, "buffers overlap", f(h, R[0], R[0], 2, None))


def test_apply_galois(ctxs):
    x = ctxs("n256_l3")
    f, h, R, w = x.lib.dpfhe_apply_galois, x.h, x.R, "dpfhe_apply_galois"
    x.ok(w, f(h, R[0], R[1], 1, 3, None))
    x.no(w, "galois_elt must be odd and < 2N", f(h, R[0], R[1], 1, 2, None))
    x.no(w, "galois_elt must be odd and < 2N", f(h, R[0], R[1], 1, 2 * x.n + 1, None))
    x.each_misaligned(w, "null, misaligned or aliased buffer", lambda o, i: f(h, o, i, 1, 3, None), (R[0], R[1]))
    x.no(w, "null, misaligned or aliased buffer", f(h, R[0], R[0], 1, 3, None))
    x.no(w, "null, misaligned or aliased buffer", f(h, R[0] + 16, R[0], 1, 3, None))


# ---- multiply and key switching --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BOTH)
def test_ct_mul(ctxs, name):
    x = ctxs(name)
    f, h, R, w = x.lib.dpfhe_ct_mul, x.h, x.R, "dpfhe_ct_mul"
    for flags in (0, 3):
        x.ok(w, f(h, R[0], R[1], R[2], 1, flags, None))
    x.ok(w, f(h, R[0], R[1], R[1], 1, 0, None))                    # a square
    x.no(w, "unknown flag", f(h, R[0], R[1], R[2], 1, 4, None))
    x.each_misaligned(w, BUF, lambda o, a, b: f(h, o, a, b, 1, 0, None), (R[0], R[1], R[2]))
    x.no(w, "output overlaps an operand", f(h, R[1], R[1], R[2], 1, 0, None))
    x.no(w, "output overlaps an operand", f(h, R[2], R[1], R[2], 1, 0, None))


def test_ct_mul_trace(ctxs):
    w = "dpfhe_debug_ct_mul_trace"
    x = ctxs("n256_l3")
    x.no(w, "FoldArith contexts at N = 4096 only", x.lib.dpfhe_debug_ct_mul_trace(x.h, x.R[0], x.R[1], x.R[2], 1, x.R[3], None), STATE)
    x = ctxs("n4096_l1")
    f, h, R = x.lib.dpfhe_debug_ct_mul_trace, x.h, x.R
    x.ok(w, f(h, R[0], R[1], R[2], 1, R[3], None))
    x.no(w, "bad batch", f(h, R[0], R[1], R[2], 0, R[3], None))
    x.no(w, "output overlaps an operand", f(h, R[1], R[1], R[2], 1, R[3], None))
    x.no(w, "output overlaps an operand", f(h, R[2], R[1], R[2], 1, R[3], None))


@pytest.mark.parametrize("name", BOTH)
def test_relinearize_and_switch_key(ctxs, name):
    x = ctxs(name)
    lib, h, R = x.lib, x.h, x.R
    f, w = lib.dpfhe_relinearize, "dpfhe_relinearize"
    x.ok(w, f(h, R[0], R[1], R[2], 1, None))
    x.each_misaligned(w, BUF, lambda o, i, k: f(h, o, i, k, 1, None), (R[0], R[1], R[2]))
    x.no(w, "output overlaps the input", f(h, R[1], R[1], R[2], 1, None))
    f, w = lib.dpfhe_switch_key, "dpfhe_switch_key"
    x.ok(w, f(h, R[0], R[1], R[2], 1, None))
    x.each_misaligned(w, "null, misaligned or aliased buffer", lambda o, i, k: f(h, o, i, k, 1, None), (R[0], R[1], R[2]))
    x.no(w, "null, misaligned or aliased buffer", f(h, R[1], R[1], R[2], 1, None))


def test_rescale(ctxs):
    x, one = ctxs("n256_l3"), ctxs("n256_l1")
    f, h, R, w = x.lib.dpfhe_rescale, x.h, x.R, "dpfhe_rescale"
    x.ok(w, f(h, R[0], R[1], 1, None))
    x.each_misaligned(w, BUF, lambda o, i: f(h, o, i, 1, None), (R[0], R[1]))
    one.no(w, "no limb left to drop", f(one.h, one.R[0], one.R[1], 1, None), STATE)


@pytest.mark.parametrize("name", BOTH)
@pytest.mark.parametrize("w", ["dpfhe_relinearize_hybrid", "dpfhe_switch_key_hybrid", "dpfhe_relinearize_rescale_hybrid"])
def test_hybrid_key_switching(ctxs, w, name):
    x, one, two = ctxs(name), ctxs("n256_l1"), ctxs("n256_l2")
    f, h, R = getattr(x.lib, w), x.h, x.R
    x.ok(w, f(h, R[0], R[1], R[2], R[3], 1, None))
    one.no(w, EXTENDED, f(one.h, one.R[0], one.R[1], one.R[2], one.R[3], 1, None), STATE)
    if w == "dpfhe_relinearize_rescale_hybrid":
        two.no(w, "no data limb left to drop (Ld < 2)", f(two.h, two.R[0], two.R[1], two.R[2], two.R[3], 1, None), STATE)
    else:
        two.ok(w, f(two.h, two.R[0], two.R[1], two.R[2], two.R[3], 1, None))
    x.each_misaligned(w, BUF, lambda o, i, k, wk: f(h, o, i, k, wk, 1, None), (R[0], R[1], R[2], R[3]))
    overlap = "output, input and work buffers must not overlap"
    x.no(w, overlap, f(h, R[1], R[1], R[2], R[3], 1, None))          # out / in
    x.no(w, overlap, f(h, R[0], R[1], R[2], R[1], 1, None))          # work / in
    x.no(w, overlap, f(h, R[0], R[1], R[2], R[0], 1, None))          # work / out


@pytest.mark.parametrize("name", BOTH)
def test_switch_key_qp(ctxs, name):
    x, one = ctxs(name), ctxs("n256_l1")
    f, h, R, w = x.lib.dpfhe_switch_key_qp, x.h, x.R, "dpfhe_switch_key_qp"
    x.ok(w, f(h, R[0], R[1], R[2], 1, 1, None))
    x.ok(w, f(h, R[0], R[1], R[2], 2, 2, None))
    one.no(w, EXTENDED, f(one.h, one.R[0], one.R[1], one.R[2], 1, 1, None), STATE)
    x.each_misaligned(w, BUF, lambda o, i, k: f(h, o, i, k, 1, 1, None), (R[0], R[1], R[2]))
    x.no(w, "output overlaps the input", f(h, R[1], R[1], R[2], 1, 1, None))


def test_rescale_bsgs(ctxs):
    x, one = ctxs("n256_l3"), ctxs("n256_l1")
    f, h, R, w = x.lib.dpfhe_rescale_bsgs, x.h, x.R, "dpfhe_rescale_bsgs"
    x.ok(w, f(h, R[0], R[1], R[2], 1, 1, None))
    x.ok(w, f(h, R[0], R[1], R[2], 0, 1, None))
    one.no(w, "no limb left to drop", f(one.h, one.R[0], one.R[1], one.R[2], 1, 1, None), STATE)
    x.each_misaligned(w, BUF, lambda o, i, a: f(h, o, i, a, 1, 1, None), (R[0], R[1], R[2]))
    x.no(w, "output overlaps an input", f(h, R[1], R[1], R[2], 1, 1, None))
    x.no(w, "output overlaps an input", f(h, R[2], R[1], R[2], 1, 1, None))


def test_lincomb_rescale(ctxs):
    x, one = ctxs("n256_l3"), ctxs("n256_l1")
    f, h, R, w = x.lib.dpfhe_lincomb_rescale, x.h, x.R, "dpfhe_lincomb_rescale"
    call = lambda o, i, wt, n_terms=2, batch=1: f(h, o, i, wt, n_terms, batch, None)
    ptrs = (R[0], R[1], R[2])
    x.ok(w, call(*ptrs))
    one.no(w, "no limb left to drop", f(one.h, one.R[0], one.R[1], one.R[2], 2, 1, None), STATE)
    x.no(w, "1 to 16 terms", call(*ptrs, n_terms=0))
    x.no(w, "1 to 16 terms", call(*ptrs, n_terms=17))
    x.no(w, "batch must be positive", call(*ptrs, batch=0))
    x.no(w, "output overlaps an input", call(R[1], R[1], R[2]))
    x.no(w, "output overlaps an input", call(R[2], R[1], R[2]))
    x.each_misaligned(w, "misaligned buffer", call, ptrs)             # (the last check: after the shapes and the overlaps)


# ---- rotations -------------------------------------------------------------------------------------------------------------------------------------------
def test_rotate_hybrid_batch_and_grouped(ctxs):
    x, one = ctxs("n256_l3"), ctxs("n256_l1")
    lib, h, R, n = x.lib, x.h, x.R, x.n
    good, even, big = fp.u32([3, 5, 7, 9]), fp.u32([3, 2]), fp.u32([3, 2 * n + 1])
    f, w = lib.dpfhe_rotate_hybrid_batch, "dpfhe_rotate_hybrid_batch"
    call = lambda o, i, k, wk, rot, n_in=1, batch=2, e=good: f(h, o, i, n_in, e, k, wk, rot, batch, None)
    ptrs = (R[0], R[1], R[2], R[3], R[4])
    x.ok(w, call(*ptrs))
    x.ok(w, call(*ptrs, n_in=2))
    one.no(w, EXTENDED, f(one.h, one.R[0], one.R[1], 1, good, one.R[2], one.R[3], one.R[4], 2, None), STATE)
    x.no(w, "n_in must be 1 (one input, many rotations) or equal to batch", call(*ptrs, n_in=2, batch=3))
    x.each_misaligned(w, "null, misaligned or aliased buffer", call, ptrs)
    x.no(w, "null, misaligned or aliased buffer", call(R[0], R[1], R[2], R[3], R[1]))          # d_rotated == d_in2
    x.no(w, GALOIS, call(*ptrs, e=even))
    x.no(w, GALOIS, call(*ptrs, e=big))
    x.no(w, "d_rotated overlaps the input", call(R[0], R[1], R[2], R[3], R[1] + 16, n_in=2))
    overlap = "output, input and work buffers must not overlap"                                # the key switch's own checks, on the rotated input
    x.no(w, overlap, call(R[0], R[1], R[2], R[3], R[0]))            # out / rotated
    x.no(w, overlap, call(R[0], R[1], R[2], R[4], R[4]))            # work / rotated
    x.no(w, overlap, call(R[0], R[1], R[2], R[0], R[4]))            # work / out
    f, w = lib.dpfhe_rotate_hybrid_grouped, "dpfhe_rotate_hybrid_grouped"
    call = lambda o, i, k, wk, rot, e=good, n_elts=2, group=2: f(h, o, i, e, n_elts, group, k, wk, rot, None)
    x.ok(w, call(*ptrs))
    x.ok(w, call(*ptrs, group=0))                                   # an empty batch
    one.no(w, EXTENDED, f(one.h, one.R[0], one.R[1], good, 2, 2, one.R[2], one.R[3], one.R[4], None), STATE)
    x.each_misaligned(w, "null, misaligned or aliased buffer", call, ptrs)
    x.no(w, GALOIS, call(*ptrs, e=even))
    x.no(w, GALOIS, call(*ptrs, e=big))
    x.no(w, "d_rotated overlaps the input", call(R[0], R[1], R[2], R[3], R[1] + 16))


@pytest.mark.parametrize("name", BOTH)
def test_rotate_hoisted_qp(ctxs, name):
    x, one = ctxs(name), ctxs("n256_l1")
    f, h, R, n, w = x.lib.dpfhe_rotate_hoisted_qp, x.h, x.R, x.n, "dpfhe_rotate_hoisted_qp"
    good, even, big = fp.u32([3, 5]), fp.u32([3, 2]), fp.u32([2 * n + 1, 3])
    call = lambda o, i, k, ntt, dig, e=good: f(h, o, i, 1, e, k, ntt, dig, 2, None)
    ptrs = (R[0], R[1], R[2], R[3], R[4])
    x.ok(w, call(*ptrs))
    one.no(w, EXTENDED, f(one.h, one.R[0], one.R[1], 1, good, one.R[2], one.R[3], one.R[4], 2, None), STATE)
    x.each_misaligned(w, BUF, call, ptrs)
    x.no(w, GALOIS, call(*ptrs, e=even))
    x.no(w, GALOIS, call(*ptrs, e=big))
    o, i, k, ntt, dig = ptrs
    for bad in ((i, i, k, ntt, dig), (ntt, i, k, ntt, dig), (dig, i, k, ntt, dig), (o, i, k, ntt, i), (o, i, k, dig, dig), (o, i, k, i, dig)):
        x.no(w, "buffers must not overlap", call(*bad))


def test_rotate_hybrid_hoisted(ctxs):
    x, one, big_ring = ctxs("n256_l3"), ctxs("n256_l1"), ctxs("n16384_l3")
    w = "dpfhe_rotate_hybrid_hoisted"
    for c in (x, big_ring):
        f, h, R, n = c.lib.dpfhe_rotate_hybrid_hoisted, c.h, c.R, c.n
        good, even, big = fp.u32([3, 5]), fp.u32([3, 2]), fp.u32([2 * n + 1, 3])
        call = lambda o, i, k, wk, rot, dig, e=good: f(h, o, i, 1, e, k, wk, rot, dig, 2, None)
        ptrs = (R[0], R[1], R[2], R[3], R[4], R[5])
        c.ok(w, call(*ptrs))
        c.each_misaligned(w, BUF, call, ptrs)
        c.no(w, GALOIS, call(*ptrs, e=even))
        c.no(w, GALOIS, call(*ptrs, e=big))
        o, i, k, wk, rot, dig = ptrs
        for bad in ((i, i, k, wk, rot, dig), (wk, i, k, wk, rot, dig), (rot, i, k, wk, rot, dig), (o, i, k, rot, rot, dig), (o, i, k, dig, rot, dig),
                    (dig, i, k, wk, rot, dig), (o, i, k, wk, dig, dig), (o, i, k, wk, rot, i), (o, i, k, wk, i, dig)):
            c.no(w, "buffers must not overlap", call(*bad))
    one.no(w, EXTENDED, one.lib.dpfhe_rotate_hybrid_hoisted(one.h, one.R[0], one.R[1], 1, fp.u32([3, 5]), one.R[2], one.R[3], one.R[4], one.R[5], 2, None), STATE)
    # above the fused limit the deferred-division pipeline never touches d_work / d_rotated0: both may be null there (and are refused below: a null case,
    # left to the reading of the diff like every other)
    c = big_ring
    c.ok(w, c.lib.dpfhe_rotate_hybrid_hoisted(c.h, c.R[0], c.R[1], 1, fp.u32([3, 5]), c.R[2], None, None, c.R[5], 2, None))
    c.no(w, BUF, c.lib.dpfhe_rotate_hybrid_hoisted(c.h, c.R[0], c.R[1], 1, fp.u32([3, 5]), c.R[2], c.R[3] + 8, None, c.R[5], 2, None))


def test_ntt_inv_galois(ctxs):
    x = ctxs("n256_l3")
    f, h, R, n, w = x.lib.dpfhe_ntt_inv_galois, x.h, x.R, x.n, "dpfhe_ntt_inv_galois"
    good = fp.u32([3, 5])
    x.ok(w, f(h, R[0], R[1], 1, good, 2, None))
    x.ok(w, f(h, R[0], R[0], 1, good, 2, None))
    x.each_misaligned(w, BUF, lambda o, i: f(h, o, i, 1, good, 2, None), (R[0], R[1]))
    x.no(w, GALOIS, f(h, R[0], R[1], 1, fp.u32([3, 2]), 2, None))
    x.no(w, GALOIS, f(h, R[0], R[1], 1, fp.u32([2 * n + 1, 3]), 2, None))
    x.no(w, "output must be the input buffer or disjoint from it", f(h, R[0] + 16, R[0], 1, good, 2, None))


# ---- matrix-vector products and sums ---------------------------------------------------------------------------------------------------------------------
def test_matvecs(ctxs):
    x = ctxs("n256_l3")
    lib, h, R = x.lib, x.h, x.R
    f, w = lib.dpfhe_matvec_plain, "dpfhe_matvec_plain"
    x.ok(w, f(h, R[0], R[1], R[2], 1, 1, None))
    x.ok(w, f(h, R[0], R[1], R[2], 5, 3, None))
    x.no(w, "cols must be > 0", f(h, R[0], R[1], R[2], 1, 0, None))
    x.each_misaligned(w, BUF, lambda y, W, v: f(h, y, W, v, 1, 1, None), (R[0], R[1], R[2]))
    f, w = lib.dpfhe_matvec_plain_multi, "dpfhe_matvec_plain_multi"
    x.ok(w, f(h, R[0], R[1], R[2], 1, 1, 3, None))
    x.no(w, "cols must be > 0", f(h, R[0], R[1], R[2], 1, 0, 3, None))
    x.each_misaligned(w, BUF, lambda y, W, v: f(h, y, W, v, 1, 1, 3, None), (R[0], R[1], R[2]))
    f, w = lib.dpfhe_matvec_scalar, "dpfhe_matvec_scalar"
    x.ok(w, f(h, R[0], R[1], R[2], 1, 1, None))
    x.ok(w, f(h, R[0], R[1] + 8, R[2], 1, 1, None))                # d_w is 8-byte aligned
    x.no(w, "cols must be > 0", f(h, R[0], R[1], R[2], 1, 0, None))
    x.no(w, BUF, f(h, R[0] + 8, R[1], R[2], 1, 1, None))
    x.no(w, BUF, f(h, R[0], R[1] + 4, R[2], 1, 1, None))
    x.no(w, BUF, f(h, R[0], R[1], R[2] + 8, 1, 1, None))


def test_reduce_sum_rejected_leaves_the_output_untouched(ctxs):
    import torch
    x = ctxs("n256_l3")
    f, h, R, w = x.lib.dpfhe_reduce_sum, x.h, x.R, "dpfhe_reduce_sum"
    out = x.pool[:x.region_words]
    assert out.data_ptr() == R[0]
    out.fill_(SENTINEL)
    x.no(w, "count and components must be > 0", f(h, R[0], R[1], 0, 1, None))
    x.no(w, "count and components must be > 0", f(h, R[0], R[1], 1, 0, None))
    x.each_misaligned(w, BUF, lambda o, i: f(h, o, i, 1, 1, None), (R[0], R[1]))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()), "a rejected dpfhe_reduce_sum wrote its output (the memset comes after the last check)"
    x.ok(w, f(h, R[0], R[1], 1, 1, None))
    x.ok(w, f(h, R[0], R[1], 9, 2, None))
    torch.cuda.synchronize()
    assert bool((out[:2 * x.L * x.n] != SENTINEL).all()) and bool((out[2 * x.L * x.n:] == SENTINEL).all())     # (a residue is < 2^60)
    out.zero_()
    f, w = x.lib.dpfhe_canonicalize_sum, "dpfhe_canonicalize_sum"
    x.ok(w, f(h, R[0], 1, None))
    x.no(w, BUF, f(h, R[0] + 8, 1, None))


# ---- base extension --------------------------------------------------------------------------------------------------------------------------------------
def test_base_extend_and_scale_round(ctxs):
    x = ctxs("n256_l3")
    lib, h, R = x.lib, x.h, x.R
    f, w = lib.dpfhe_base_extend, "dpfhe_base_extend"
    call = lambda o=R[0], os=1, i=R[1], is_=1, s0=0, ns=1, d0=1, nd=1: f(h, o, os, i, is_, s0, ns, d0, nd, 2, None)
    x.ok(w, call())
    x.ok(w, call(os=3, is_=2, ns=2, d0=2))
    limbs = "1..10 source limbs and 1..20 destination limbs inside the context"
    for bad in (dict(ns=0), dict(nd=0), dict(ns=11), dict(nd=21), dict(s0=4), dict(s0=2, ns=2), dict(d0=4), dict(d0=2, nd=2)):
        x.no(w, limbs, call(**bad))
    stride = "null or misaligned buffer, or an item stride shorter than its limbs"
    x.no(w, stride, call(o=R[0] + 8))
    x.no(w, stride, call(i=R[1] + 8))
    x.no(w, stride, call(os=1, nd=2))
    x.no(w, stride, call(is_=1, ns=2, d0=2))
    x.no(w, "output overlaps the input", call(o=R[1]))
    f, w = lib.dpfhe_scale_round, "dpfhe_scale_round"
    call = lambda o=R[0], os=2, i=R[1], dr0=2, ndr=1, k0=0, nk=2, mul=1: f(h, o, os, i, dr0, ndr, k0, nk, mul, 2, None)
    x.ok(w, call())
    x.ok(w, call(mul=3))
    x.no(w, "multiplier must be > 0", call(mul=0))
    for bad in (dict(ndr=0), dict(nk=0), dict(dr0=4), dict(dr0=2, ndr=2), dict(k0=4), dict(k0=2, nk=2)):
        x.no(w, limbs, call(**bad))
    x.no(w, "the dropped limbs and the kept limbs must be disjoint", call(dr0=1))
    x.no(w, "the dropped limbs and the kept limbs must be disjoint", call(k0=1))
    x.no(w, stride, call(o=R[0] + 8))
    x.no(w, stride, call(i=R[1] + 8))
    x.no(w, stride, call(os=1))
    x.no(w, "output overlaps the input", call(o=R[1]))


# ---- context setters -------------------------------------------------------------------------------------------------------------------------------------
def test_context_setters(ctxs):
    x, t = ctxs("n256_l3"), ctxs("n4096_l1")
    lib = x.lib
    w = "dpfhe_ctx_autotune"
    x.ok(w, lib.dpfhe_ctx_autotune(x.h, x.R[0], 7 * x.L * x.n, 1, None))                      # one form only: nothing to choose
    pair = 7 * t.L * t.n
    need = "d_work must hold at least 7 L N words (one ciphertext pair + its product)"
    try:
        t.ok(w, lib.dpfhe_ctx_autotune(t.h, t.R[0], pair, 1, None))
        t.no(w, need, lib.dpfhe_ctx_autotune(t.h, t.R[0] + 8, pair, 1, None))
        t.no(w, need, lib.dpfhe_ctx_autotune(t.h, t.R[0], pair - 1, 1, None))
    finally:
        lib.dpfhe_tune_cache_clear()           # (the probe's result is cached per shape for later contexts of this process)
    w = "dpfhe_ctx_set_ct_mul_variant"
    x.no(w, "this context has no such form of the fused multiply", lib.dpfhe_ctx_set_ct_mul_variant(x.h, 0))
    for v in (1, 0):
        t.ok(w, lib.dpfhe_ctx_set_ct_mul_variant(t.h, v))
        t.ok("dpfhe_ct_mul", lib.dpfhe_ct_mul(t.h, t.R[0], t.R[1], t.R[2], 1, 0, None))
    for v in (2, -1):
        t.no(w, "this context has no such form of the fused multiply", lib.dpfhe_ctx_set_ct_mul_variant(t.h, v))
    w = "dpfhe_ctx_set_scratch_limit"
    x.ok(w, lib.dpfhe_ctx_set_scratch_limit(x.h, 1024))                                       # the default
    x.no(w, "limit must be in [1 MiB, 1 TiB]", lib.dpfhe_ctx_set_scratch_limit(x.h, 0))
    x.no(w, "limit must be in [1 MiB, 1 TiB]", lib.dpfhe_ctx_set_scratch_limit(x.h, (1 << 20) + 1))
    w = "dpfhe_ctx_release_scratch"
    for flags in (0, 1):
        x.ok(w, lib.dpfhe_ctx_release_scratch(x.h, None, flags))
    x.no(w, "unknown flag", lib.dpfhe_ctx_release_scratch(x.h, None, 2))
