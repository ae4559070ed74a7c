"""-m gpu: the batched entry points of include/dpfhe.h on buffers that cross the 4 GiB line, and the flat-indexed ones past 2^31 and 2^32 words
(tests/wide_batch.py; tests/test_wide_batch_cpu.py shows that its check names every planted 32-bit defect, plans every case below at the real lines and
pins the tier B peaks).

Every other device test runs on buffers of a few MiB, so an offset that a kernel or a launcher forms in 32 bits passes them all.  Here P = 3 distinct items
are built on the host as the other tests build them (Rig.words: worst-case stripes, q - 1 everywhere), uploaded and tiled ON THE DEVICE to the batch at which
the SMALLEST batched buffer of the call ends two whole items past the highest line of the tier - every batched pointer crosses it.  Outputs and in-out
buffers start as 0xDEADBEEFCAFEF00D with one more item of it behind them.  After the call: the first P output items equal the oracle (oracle.cbind.Oracle,
threads = 0; Python integers for the reductions) word for word; item i equals item i - P for every i >= P; the tail still holds the sentinel; every input
is still periodic with its uploaded first period.  An unwritten item is a sentinel, a mis-addressed one breaks the period: together every item is held
to the reference.  The samplers, whose words depend on first_item + i, are held to their host twins on sampled items (the first two, the last two, the item
on each line and its neighbours) and to "no sentinel left in the written component" everywhere.  All compares run on the device in 1 GiB slices; nothing
of the large size exists on the host; a wrong word is a failed assertion naming (buffer, item, limb, word) and the line it lies beyond.

Tier A (B31 = 2^31 and B32 = 2^32 bytes; at most 24 GiB per case, never skipped: short memory is a failure with the figures of mem_get_info).
Tier B (W31 = 2^31 and W32 = 2^32 words: one buffer of 32 GiB + 2 items; at most 70 GiB; skipped only when less than peak + 8 GiB is free).

Entry -> cases (a batched entry of include/dpfhe.h that is in neither list is a gap):
  dpfhe_ntt_fwd / _inv / _fwd_oop / _inv_oop      A: ntt-*  fold N = 4096 (single kernel), 8192 (halves), 16384 (quarters), 65536 (split), mixed classes
                                                     (ntt_classes_kernel), generic primes;  B: in place at N = 4096 and 65536
  dpfhe_dyadic_mul / _mul_add / dpfhe_add / dpfhe_sub / dpfhe_negate / dpfhe_multiply_plain
                                                  A: dyadic-*;  B: negate in place, add with out == a
  dpfhe_apply_galois / dpfhe_rescale / dpfhe_copy A: galois, rescale, copy
  dpfhe_canonicalize_sum                          A and B: canonicalize
  dpfhe_reduce_sum                                A: reduce-partial (generic primes), reduce-thin (fold limbs, count > 512: the buffer-resource loads);  B: reduce-thin
  dpfhe_ct_mul                                    A: ct_mul-quad / -dual (N = 4096), -n8192, -generic, -composed (N = 16384, default scratch limit: slices of
                                                     1024 items, the ninth slice base exactly on B32 of the operands)
  dpfhe_relinearize / dpfhe_switch_key            A: relinearize, switch_key (two limbs)
  dpfhe_relinearize_hybrid / dpfhe_switch_key_hybrid   A: relinearize_hybrid, switch_key_hybrid (d_work batched too)
  dpfhe_matvec_plain / _scalar / _plain_multi     A: matvec-* (W tiled along rows; W and y cross, d_w of _scalar is tiled and small)
  dpfhe_base_extend / dpfhe_scale_round           A: base_extend, scale_round
  dpfhe_expand_uniform / dpfhe_sample_noise       A: expand, noise-* (three kinds, set and add; the component that is not written is held over the whole buffer);
                                                     B: expand, noise-ternary on one component
  dpfhe_ct_mul_sum                                A: ct_mul_sum-own (flags 0), -own-ntt (IN_NTT | OUT_NTT), -shared (the shared second operand): groups tiled
  dpfhe_ct_mul_complement                         A: ct_mul_complement (K = 1, flags 0), -ntt, -self (the self products alone), -both (the products, then the self
                                                     products: two stretches, each periodic): groups tiled
  dpfhe_relinearize_rescale_hybrid                A: relinearize_rescale_hybrid (three data limbs: the smallest with a limb left after the rescale)
  dpfhe_lincomb_rescale                           A: lincomb_rescale (one term)
  dpfhe_rotate_hybrid_grouped / dpfhe_rotate_add_hybrid / dpfhe_switch_key_qp / dpfhe_rescale_bsgs
                                                  A: their names, on a two-limb extended context (one data limb under the special prime)
  dpfhe_rotate_hoisted_qp                         A: rotate_hoisted_qp: one token, the rotations tiled - d_keys and d_out_qp (block 0, then the periodic rotations) cross B32
  dpfhe_rotate_hybrid_hoisted                     A: rotate_hybrid_hoisted-composed at N = 16384 (d_work / d_rotated0 unused there: NULL), one token, the rotations
                                                     tiled: d_keys and d_out2 cross B32, slices of 2046 rotations with a slice base past B32 of each;
                                                     rotate_hybrid_hoisted-fused at N = 4096, one token: d_keys, d_work and d_out2 cross B32, d_rotated0 crosses B31
                                                     (all four past B32 take 11 x 4 GiB)
  dpfhe_rotate_hybrid_batch                       A: rotate_hybrid_batch, one input: d_keys and d_work cross B32, d_rotated and d_out2 cross B31 (all four past B32
                                                     take 24.4 GiB, over the cap)
  dpfhe_ntt_inv_galois                            A: ntt_inv_galois apart and in place, one element per item tiled with the same odd period
  dpfhe_add_plain / dpfhe_add_plain_scaled        A: add_plain*-broadcast (out of place) and -one-to-one (in place: the plaintexts cross too)
  dpfhe_compact / dpfhe_encode_slots / dpfhe_encode_complex   A: compact, encode_slots, encode_complex (each with and without the forward transform)
  dpfhe_rerandomize                               A: rerandomize (sampled items against the definition; its d_work batched too)
  dpfhe_relinearize_lincomb_rescale_hybrid        A: one term: d_in, d_work and the term cross B32, d_out2 crosses B31 (all four past B32 take 27 GiB, over the cap)
Where a case says that a pointer crosses B31 only, a 32-bit defect that shows first past 2^32 bytes of THAT buffer is not held by it; every other batched
pointer of every case crosses the highest line of its tier.
Outside the table by design: the collectives (a world of one moves no offsets of ours), dpfhe_debug_ct_mul_trace, the _host twins."""
import numpy as np
import pytest

import wide_batch as wb
from class_edges import Rig, edge_moduli
from deeppowers_amd import _cabi, wire

pytestmark = pytest.mark.gpu

P = 3
K_MAX_GRID = 0x7FFFFFFF
SEED = bytes(range(7, 39))
SCRATCH_DEFAULT_BYTES = (1024 << 17) * 8     # dpfhe_ctx::scratch_limit_words at creation


def chunks_of(n):
    return max(n // 512, 1)


def ntt_widest(log2n, npolys):
    """cabi.h ntt_grid_fits: the widest grid a batched transform of npolys residue polynomials launches"""
    log_n1 = log2n - 12 if log2n > 14 else 0
    return max(npolys << log_n1, npolys << 4) if log_n1 else npolys


class WideCase:
    def __init__(self, id, tier, kind, log2n, shape, run):
        self.id, self.tier, self.kind, self.log2n, self.shape, self.run = id, tier, kind, log2n, shape, run

    def plan(self):
        p = edge_moduli(self.kind, self.log2n)
        s = self.shape(p.n_limbs, p.n)
        return wb.plan(s["items"], self.tier, period=P, writable=s.get("writable", ()), extra_bytes=s.get("extra", 0), limits=s.get("limits", ()),
                       margin=s.get("margin", 2), low_items=s.get("low_items"))


CASES = []


def case(id, tier, kind, log2n, shape):
    def register(fn):
        CASES.append(WideCase(id, tier, kind, log2n, shape, fn))
        return fn
    return register


# ---- one call on tiled buffers --------------------------------------------------------------------------------------------------------------------------------
class Call:
    """the buffers of one call: inp / out / inout / scratch name them, run() makes the call and checks everything"""

    def __init__(self, r, pl):
        self.r, self.pl, self.dev = r, pl, r.ctx.device
        self.t, self.inputs, self.outputs, self.tails, self.limb = {}, {}, {}, [], {}
        self.tail_rows, self.stretches = [], {}

    def inp(self, name, period_items, limb_words=None):
        a = np.ascontiguousarray(period_items, dtype=np.uint64).reshape(P, -1)
        self.t[name] = wb.tile(a, self.pl.batch, self.dev)
        self.inputs[name] = a
        self.limb[name] = limb_words or self.r.n
        return self.t[name].data_ptr()

    def shared(self, name, a):
        """an operand that is not batched (a key, a plaintext, the right-hand sides): uploaded as it is, compared whole afterwards"""
        import torch
        a = np.ascontiguousarray(a, dtype=np.uint64)
        self.t[name] = torch.from_numpy(a.view(np.int64).reshape(1, -1)).to(self.dev)
        self.inputs[name] = a.reshape(1, -1)
        self.limb[name] = self.r.n
        return self.t[name].data_ptr()

    def out(self, name, want_period, limb_words=None):
        w = np.ascontiguousarray(want_period, dtype=np.uint64).reshape(P, -1)
        self.t[name] = wb.sentinel(self.pl.batch, w.shape[1], self.dev)
        self.outputs[name] = w
        self.limb[name] = limb_words or self.r.n
        return self.t[name].data_ptr()

    def inout(self, name, period_items, want_period, limb_words=None):
        ptr = self.out(name, want_period, limb_words)
        a = np.ascontiguousarray(period_items, dtype=np.uint64).reshape(P, -1)
        wb.tile_into(self.t[name], a, self.pl.batch)
        return ptr

    def scratch(self, name, words):
        self.t[name] = wb.sentinel(self.pl.batch, words, self.dev)
        self.tails.append(name)
        return self.t[name].data_ptr()

    def small_scratch(self, name, words):
        """scratch that is not batched: its tail item must stay sentinel"""
        self.t[name] = wb.sentinel(1, words, self.dev)
        self.tail_rows.append(name)
        return self.t[name].data_ptr()

    def stretched_out(self, name, stretches, words):
        """an output of several stretches, each periodic on its own: stretches = [(items, want_period [<= P][words])], back to back; one tail item behind"""
        total = sum(c for c, _ in stretches)
        self.t[name] = wb.sentinel(total, words, self.dev)
        self.stretches[name] = stretches
        self.tail_rows.append(name)
        self.limb[name] = self.r.n
        return self.t[name].data_ptr()

    def small_out(self, name, want, limb_words=None):
        w = np.ascontiguousarray(want, dtype=np.uint64).reshape(1, -1)
        self.t[name] = wb.sentinel(1, w.shape[1], self.dev)
        self.small = (name, w)
        self.limb[name] = limb_words or self.r.n
        return self.t[name].data_ptr()

    def run(self, what, rc):
        import torch
        _cabi.check(rc or 0, what)
        torch.cuda.synchronize(self.dev)
        self.check(what)

    def check(self, what):
        pl = self.pl
        try:
            for name, want in self.outputs.items():
                wb.check_output(name, self.t[name], pl, want, self.limb[name])
            if getattr(self, "small", None):
                wb.check_small_output(self.small[0], self.t[self.small[0]], self.small[1], self.limb[self.small[0]])
            for name in self.tails:
                wb.check_tail(name, self.t[name], pl)
            for name, stretches in self.stretches.items():
                at = 0
                for count, want in stretches:
                    wb.check_stretch(name, self.t[name], at, count, P, want, self.limb[name])
                    at += count
            for name in self.tail_rows:
                wb.check_tail_row(name, self.t[name])
            for name, a in self.inputs.items():
                if a.shape[0] == 1:
                    got = self.t[name].cpu().numpy().view(np.uint64)
                    assert np.array_equal(got, a), f"{name}: a shared operand changed"
                else:
                    wb.check_input(name, self.t[name], pl, a, self.limb[name])
        except wb.WideBatchError as e:
            raise wb.WideBatchError(e.buffer, e.kind, e.item, e.limb, e.word, e.line, f"{what} on {self.r.kind} N = {self.r.n}, batch {pl.batch}: {e}") from e

    def close(self):
        self.t.clear()
        wb.release()


# ---- rigs: one context per (kind, ring) for the whole module --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rigs():
    made = {}

    def get(kind, log2n):
        if (kind, log2n) not in made:
            made[(kind, log2n)] = Rig(kind, log2n)
        return made[(kind, log2n)]
    yield get
    for r in made.values():
        r.close()


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------------------------------
def polys_shape(per_item_in, per_item_out=None, inplace=False, ntt_polys=None, extra=0):
    """buffers of whole RNS polynomials: per_item_* counted in L N words"""
    def shape(L, n):
        poly = L * n
        if inplace:
            items, writable = {"io": per_item_in * poly}, ("io",)
        else:
            items = {f"in{i}": w * poly for i, w in enumerate(per_item_in if isinstance(per_item_in, tuple) else (per_item_in,))}
            items["out"] = (per_item_out or 1) * poly
            writable = ("out",)
        log2n = n.bit_length() - 1
        lim = [("residue polynomials per launch", lambda b: b * max(items.values()) // n, K_MAX_GRID)]
        if ntt_polys:
            lim.append(("widest transform grid", lambda b: ntt_widest(log2n, b * ntt_polys * L), K_MAX_GRID))
        return {"items": items, "writable": writable, "limits": lim, "extra": extra}
    return shape


# ---- transforms -----------------------------------------------------------------------------------------------------------------------------------------------
NTT_CTX = [("fold2", 12), ("fold2", 13), ("fold2", 14), ("fold2", 16), ("mixed", 12), ("shoup60", 12)]


def _ntt(name, inplace):
    def run(r, pl, call):
        lib, h, orc = r.ctx._lib, r.ctx.handle, r.orc
        x = r.words(orc, (P,), 100)
        want = (orc.ntt_inv if "inv" in name else orc.ntt_fwd)(x, threads=0)
        if inplace:
            io = call.inout("io", x, want)
            call.run(name, getattr(lib, name)(h, io, pl.batch, None))
        else:
            i, o = call.inp("in0", x), call.out("out", want)
            call.run(name, getattr(lib, name)(h, o, i, pl.batch, None))
    return run


for _kind, _ln in NTT_CTX:
    for _name, _inplace in (("dpfhe_ntt_fwd", True), ("dpfhe_ntt_inv", True), ("dpfhe_ntt_fwd_oop", False), ("dpfhe_ntt_inv_oop", False)):
        case(f"ntt-{_name[6:]}-{_kind}-n{1 << _ln}", "A", _kind, _ln, polys_shape(1, 1, inplace=_inplace, ntt_polys=1))(_ntt(_name, _inplace))
for _ln in (12, 16):
    for _name in ("dpfhe_ntt_fwd", "dpfhe_ntt_inv"):
        case(f"B-ntt-{_name[6:]}-fold2-n{1 << _ln}", "B", "fold2", _ln, polys_shape(1, inplace=True, ntt_polys=1))(_ntt(_name, True))


# ---- the coefficient-wise entries -----------------------------------------------------------------------------------------------------------------------------
def _dyadic(op):
    def run(r, pl, call):
        lib, h, orc = r.ctx._lib, r.ctx.handle, r.orc
        x, y = r.words(orc, (P,), 401), r.words(orc, (P,), 411)
        y[0] = y[0][:, ::-1]
        if op == "mul_add":
            acc = r.words(orc, (P,), 421)
            a, b = call.inp("in0", x), call.inp("in1", y)
            io = call.inout("out", acc, orc.dyadic("mul_add", x, y, acc=acc))
            return call.run("dpfhe_dyadic_mul_add", lib.dpfhe_dyadic_mul_add(h, io, a, b, pl.batch, None))
        fn = getattr(lib, {"mul": "dpfhe_dyadic_mul", "add": "dpfhe_add", "sub": "dpfhe_sub"}[op])
        a, b, o = call.inp("in0", x), call.inp("in1", y), call.out("out", orc.dyadic(op, x, y))
        call.run(op, fn(h, o, a, b, pl.batch, None))
    return run


for _kind in ("fold2", "shoup60"):
    for _op in ("mul", "mul_add", "add", "sub"):
        case(f"dyadic-{_op}-{_kind}", "A", _kind, 12, polys_shape((1, 1), 1))(_dyadic(_op))


def _negate(inplace):
    def run(r, pl, call):
        lib, h, orc = r.ctx._lib, r.ctx.handle, r.orc
        x = r.words(orc, (P,), 402)
        want = orc.dyadic("negate", x)
        if inplace:
            io = call.inout("io", x, want)
            return call.run("dpfhe_negate in place", lib.dpfhe_negate(h, io, io, pl.batch, None))
        a, o = call.inp("in0", x), call.out("out", want)
        call.run("dpfhe_negate", lib.dpfhe_negate(h, o, a, pl.batch, None))
    return run


case("dyadic-negate-fold2", "A", "fold2", 12, polys_shape(1, 1))(_negate(False))
case("B-negate-in-place", "B", "fold2", 12, polys_shape(1, inplace=True))(_negate(True))


def add_in_place_shape(L, n):
    return {"items": {"io": L * n, "in1": L * n}, "writable": ("io",), "limits": [("residue polynomials per launch", lambda b: b * L, K_MAX_GRID)]}


@case("B-add-out-is-a", "B", "fold2", 12, add_in_place_shape)
def _add_in_place(r, pl, call):
    lib, h, orc = r.ctx._lib, r.ctx.handle, r.orc
    x, y = r.words(orc, (P,), 403), r.words(orc, (P,), 413)
    io, b = call.inout("io", x, orc.dyadic("add", x, y)), call.inp("in1", y)
    call.run("dpfhe_add, out == a", lib.dpfhe_add(h, io, io, b, pl.batch, None))


@case("dyadic-multiply_plain-fold2", "A", "fold2", 12, polys_shape(1, 1))
def _multiply_plain(r, pl, call):
    lib, h, orc = r.ctx._lib, r.ctx.handle, r.orc
    x = r.words(orc, (P,), 404)
    pt = r.words(orc, (2,), 430)[0]
    want = orc.dyadic("mul", x, np.ascontiguousarray(np.broadcast_to(pt, x.shape)))
    a, p, o = call.inp("in0", x), call.shared("pt", pt), call.out("out", want)
    call.run("dpfhe_multiply_plain", lib.dpfhe_multiply_plain(h, o, a, p, pl.batch, None))


@case("galois-fold2", "A", "fold2", 12, polys_shape(1, 1))
def _galois(r, pl, call):
    lib, h, orc = r.ctx._lib, r.ctx.handle, r.orc
    x = r.words(orc, (P,), 405)
    g = 2 * r.n - 1
    a, o = call.inp("in0", x), call.out("out", orc.apply_galois(x, g))
    call.run("dpfhe_apply_galois", lib.dpfhe_apply_galois(h, o, a, pl.batch, g, None))


def rescale_shape(L, n):
    return {"items": {"in0": L * n, "out": (L - 1) * n}, "writable": ("out",),
            "limits": [("workgroups", lambda b: b * L * chunks_of(n), K_MAX_GRID)]}


@case("rescale-fold2", "A", "fold2", 12, rescale_shape)
def _rescale(r, pl, call):
    lib, h, orc = r.ctx._lib, r.ctx.handle, r.orc
    x = r.words(orc, (P,), 406)
    a, o = call.inp("in0", x), call.out("out", orc.rescale(x))
    call.run("dpfhe_rescale", lib.dpfhe_rescale(h, o, a, pl.batch, None))


def canonicalize_shape(L, n):
    return {"items": {"io": L * n}, "writable": ("io",), "limits": [("workgroups", lambda b: b * L * chunks_of(n), K_MAX_GRID)]}


def _canonicalize(r, pl, call):
    lib, h, orc = r.ctx._lib, r.ctx.handle, r.orc
    x = r.words(orc, (P,), 407)
    terms = np.random.default_rng(5).integers(1, 16, x.shape, dtype=np.uint64)      # sums of up to 15 canonical residues (15 q < 2^64)
    terms[0] = 15
    sums = x * terms
    io = call.inout("io", sums, sums % r.qcol)
    call.run("dpfhe_canonicalize_sum", lib.dpfhe_canonicalize_sum(h, io, pl.batch, None))


case("canonicalize-fold2", "A", "fold2", 12, canonicalize_shape)(_canonicalize)
case("B-canonicalize-fold2", "B", "fold2", 12, canonicalize_shape)(_canonicalize)

COPY_ITEM = 8190      # words: even (16-byte items) and no power of two - the copy takes a flat word count


def copy_shape(L, n):
    return {"items": {"in0": COPY_ITEM, "out": COPY_ITEM}, "writable": ("out",), "limits": [("workgroups", lambda b: -(-b * COPY_ITEM // 4096), K_MAX_GRID)]}


@case("copy", "A", "fold2", 12, copy_shape)
def _copy(r, pl, call):
    lib, h = r.ctx._lib, r.ctx.handle
    src = np.random.default_rng(7).integers(0, 1 << 59, (P, COPY_ITEM), dtype=np.uint64)
    a, o = call.inp("in0", src, COPY_ITEM), call.out("out", src, COPY_ITEM)
    call.run("dpfhe_copy", lib.dpfhe_copy(h, o, a, pl.batch * COPY_ITEM, None))


# ---- the shard-local sum: the huge side is the input ----------------------------------------------------------------------------------------------------------
def reduce_shape(comps):
    def shape(L, n):
        return {"items": {"in0": comps * L * n}, "extra": 2 * comps * L * n * 8,
                "limits": [("work items", comps * L * chunks_of(n) * 15, K_MAX_GRID)]}
    return shape


def tiled_sum(period, pl, moduli):
    """sum over the tiled batch, in Python integers mod q_l: reps x (sum of the period) + (sum of the cut).  period [P][comps][L][N]"""
    reps, cut = pl.reps_and_cut()
    p = period.astype(object)
    total = reps * p.sum(axis=0)
    if cut:
        total = total + p[:cut].sum(axis=0)
    q = np.array(moduli, dtype=object)[None, :, None]
    return (total % q).astype(np.uint64)


def _reduce(comps):
    def run(r, pl, call):
        lib, h, orc, L, n = r.ctx._lib, r.ctx.handle, r.orc, r.L, r.n
        cts = orc.fill(P * comps, 440).reshape(P, comps, L, n)
        cts[:, :, :, : n // 2] = r.qcol - np.uint64(1)
        if r.ctx.uses_fold:
            assert pl.batch > 512                                          # reduce_thin_kernel: fold limbs and count > 512
        a, o = call.inp("in0", cts), call.small_out("sum", tiled_sum(cts, pl, r.p.moduli))
        call.run("dpfhe_reduce_sum", lib.dpfhe_reduce_sum(h, o, a, pl.batch, comps, None))
    return run


case("reduce-partial-shoup60", "A", "shoup60", 12, reduce_shape(2))(_reduce(2))
case("reduce-thin-fold2", "A", "fold2", 12, reduce_shape(3))(_reduce(3))
case("B-reduce-thin-fold2", "B", "fold2", 12, reduce_shape(2))(_reduce(2))


# ---- the multiply ---------------------------------------------------------------------------------------------------------------------------------------------
def ct_mul_shape(extra=0):
    def shape(L, n):
        poly, log2n = L * n, n.bit_length() - 1
        return {"items": {"a2": 2 * poly, "b2": 2 * poly, "out3": 3 * poly}, "writable": ("out3",), "extra": extra,
                "limits": [("workgroups", lambda b: b * L * (chunks_of(n) if log2n > 13 else 1), K_MAX_GRID),
                           ("widest transform grid", lambda b: ntt_widest(log2n, min(b, 1024) * 3 * L), K_MAX_GRID)]}
    return shape


def _ct_mul(variant=None):
    def run(r, pl, call):
        lib, h, orc, n = r.ctx._lib, r.ctx.handle, r.orc, r.n
        a, b = r.words(orc, (P, 2), 201), r.words(orc, (P, 2), 211)
        b[0] = np.roll(b[0], n // 16, axis=-1)
        pa, pb, po = call.inp("a2", a), call.inp("b2", b), call.out("out3", orc.ct_mul(a, b, threads=0))
        if variant:
            before = r.ctx.tune_info()["chosen"]                           # (the rig is shared by the whole module: put back what was there)
            r.ctx.set_ct_mul_variant(variant)
        try:
            call.run(f"dpfhe_ct_mul {variant or ''}", lib.dpfhe_ct_mul(h, po, pa, pb, pl.batch, 0, None))
        finally:
            if variant:
                r.ctx.set_ct_mul_variant(before)
                assert r.ctx.tune_info()["chosen"] == before
    return run


case("ct_mul-quad-fold2-n4096", "A", "fold2", 12, ct_mul_shape())(_ct_mul("quad"))
case("ct_mul-dual-fold2-n4096", "A", "fold2", 12, ct_mul_shape())(_ct_mul("dual"))
case("ct_mul-fold2-n8192", "A", "fold2", 13, ct_mul_shape())(_ct_mul())
case("ct_mul-generic-shoup60-n4096", "A", "shoup60", 12, ct_mul_shape())(_ct_mul())
case("ct_mul-composed-fold2-n16384", "A", "fold2", 14, ct_mul_shape(extra=SCRATCH_DEFAULT_BYTES))(_ct_mul())


# ---- key switching --------------------------------------------------------------------------------------------------------------------------------------------
def keyswitch_shape(comps):
    def shape(L, n):
        poly = L * n
        return {"items": {"in": comps * poly, "out2": 2 * poly}, "writable": ("out2",), "extra": L * 2 * poly * 8,
                "limits": [("workgroups", lambda b: 2 * b * L * chunks_of(n), K_MAX_GRID), ("digit transforms", lambda b: b * L * L, K_MAX_GRID)]}
    return shape


@case("relinearize-fold2", "A", "fold2", 12, keyswitch_shape(3))
def _relinearize(r, pl, call):
    lib, h, orc, L = r.ctx._lib, r.ctx.handle, r.orc, r.L
    c3 = orc.ct_mul(r.words(orc, (P, 2), 300), r.words(orc, (P, 2), 301), threads=0)
    evk = r.words(orc, (L, 2), 302)
    i, k, o = call.inp("in", c3), call.shared("evk", evk), call.out("out2", orc.relinearize(c3, evk, threads=0))
    call.run("dpfhe_relinearize", lib.dpfhe_relinearize(h, o, i, k, pl.batch, None))


@case("switch_key-fold2", "A", "fold2", 12, keyswitch_shape(2))
def _switch_key(r, pl, call):
    lib, h, orc, L = r.ctx._lib, r.ctx.handle, r.orc, r.L
    ct = r.words(orc, (P, 2), 305)
    key = r.words(orc, (L, 2), 306)
    i, k, o = call.inp("in", ct), call.shared("key", key), call.out("out2", orc.switch_key(ct, key, threads=0))
    call.run("dpfhe_switch_key", lib.dpfhe_switch_key(h, o, i, k, pl.batch, None))


def hybrid_shape(comps):
    def shape(L, n):
        Ld = L - 1
        return {"items": {"in": comps * Ld * n, "work": 2 * L * n, "out2": 2 * Ld * n}, "writable": ("work", "out2"), "extra": Ld * 2 * L * n * 8,
                "limits": [("workgroups", lambda b: b * Ld * L * chunks_of(n), K_MAX_GRID)]}
    return shape


def _hybrid(name, comps):
    def run(r, pl, call):
        from oracle.cbind import Oracle
        lib, h, orc, L = r.ctx._lib, r.ctx.handle, r.orc, r.L
        data = Oracle(r.p.log2_n, r.p.moduli[:-1], r.p.psi[:-1])
        key = r.words(orc, (L - 1, 2), 303)
        ct = r.words(data, (P, comps), 310 + comps)
        i, k, w = call.inp("in", ct), call.shared("key", key), call.scratch("work", 2 * L * r.n)
        o = call.out("out2", orc.keyswitch_hybrid(ct, key, comps, threads=0))
        call.run(name, getattr(lib, name)(h, o, i, k, w, pl.batch, None))
    return run


case("relinearize_hybrid-f64_under_fold", "A", "f64_under_fold", 12, hybrid_shape(3))(_hybrid("dpfhe_relinearize_hybrid", 3))
case("switch_key_hybrid-f64_under_fold", "A", "f64_under_fold", 12, hybrid_shape(2))(_hybrid("dpfhe_switch_key_hybrid", 2))


# ---- matrix-vector products: W tiled along rows ---------------------------------------------------------------------------------------------------------------
COLS = 3


def matvec_shape(n_rhs, scalar=False):
    def shape(L, n):
        poly = L * n
        items = {"y": n_rhs * 2 * poly}
        if not scalar:
            items["W"] = COLS * poly
        return {"items": items, "writable": ("y",), "extra": COLS * n_rhs * 2 * poly * 8 + (1 << 26 if scalar else 0),
                "limits": [("workgroups", lambda b: (-(-b // 4) + 8) * L * chunks_of(n) * 2 * n_rhs, K_MAX_GRID)]}
    return shape


def _matvec(n_rhs):
    def run(r, pl, call):
        lib, h, orc, L, n = r.ctx._lib, r.ctx.handle, r.orc, r.L, r.n
        qm1 = r.qcol - np.uint64(1)
        W = orc.fill(P * COLS, 510).reshape(P, COLS, L, n)
        W[0] = qm1
        x = orc.fill(COLS * n_rhs * 2, 501).reshape(COLS, n_rhs, 2, L, n)
        x[..., : n // 2] = qm1
        want = np.stack([orc.matvec_plain(W.ravel(), np.ascontiguousarray(x[:, t]).ravel(), P, COLS, threads=0).reshape(P, 2, L, n) for t in range(n_rhs)], axis=1)
        pw, px, py = call.inp("W", W), call.shared("x", x), call.out("y", want)
        if n_rhs == 1:
            call.run("dpfhe_matvec_plain", lib.dpfhe_matvec_plain(h, py, pw, px, pl.batch, COLS, None))
        else:
            call.run("dpfhe_matvec_plain_multi", lib.dpfhe_matvec_plain_multi(h, py, pw, px, pl.batch, COLS, n_rhs, None))
    return run


def _matvec_scalar(r, pl, call):
    lib, h, orc, L, n = r.ctx._lib, r.ctx.handle, r.orc, r.L, r.n
    q = np.array(r.p.moduli, np.uint64)
    w = np.random.default_rng(3).integers(0, 1 << 62, (P, COLS, L), dtype=np.uint64) % q
    w[0] = q - np.uint64(1)
    x = orc.fill(COLS * 2, 502).reshape(COLS, 2, L, n)
    x[..., : n // 2] = r.qcol - np.uint64(1)
    pw, px, py = call.inp("w", w, L), call.shared("x", x), call.out("y", orc.matvec_scalar(w, x, P, COLS, threads=0))
    call.run("dpfhe_matvec_scalar", lib.dpfhe_matvec_scalar(h, py, pw, px, pl.batch, COLS, None))


for _kind in ("fold2", "shoup60"):
    case(f"matvec-plain-{_kind}", "A", _kind, 12, matvec_shape(1))(_matvec(1))
    case(f"matvec-multi-{_kind}", "A", _kind, 12, matvec_shape(3))(_matvec(3))
    case(f"matvec-scalar-{_kind}", "A", _kind, 12, matvec_shape(1, scalar=True))(_matvec_scalar)


# ---- base extension and scale-and-round -----------------------------------------------------------------------------------------------------------------------
def bx_shape(ns, nd):
    def shape(L, n):
        return {"items": {"in0": (ns or L) * n, "out": (nd or L - 1) * n}, "writable": ("out",),
                "limits": [("workgroups", lambda b: b * max(ns or L, nd or L) * chunks_of(n), K_MAX_GRID)]}
    return shape


@case("base_extend-fold", "A", "fold", 12, bx_shape(2, 4))
def _base_extend(r, pl, call):
    lib, h, orc, L = r.ctx._lib, r.ctx.handle, r.orc, r.L
    xs = np.ascontiguousarray(r.words(orc, (P,), 408)[:, :2])
    i, o = call.inp("in0", xs), call.out("out", orc.base_extend(xs, 0, 0, L))
    call.run("dpfhe_base_extend", lib.dpfhe_base_extend(h, o, L, i, 2, 0, 2, 0, L, pl.batch, None))


@case("scale_round-fold", "A", "fold", 12, bx_shape(0, 0))
def _scale_round(r, pl, call):
    lib, h, orc, L = r.ctx._lib, r.ctx.handle, r.orc, r.L
    w = r.words(orc, (P,), 409)
    i, o = call.inp("in0", w), call.out("out", orc.scale_round(w, L - 1, 1, 0, L - 1, 65537))
    call.run("dpfhe_scale_round", lib.dpfhe_scale_round(h, o, L - 1, i, L - 1, 1, 0, L - 1, 65537, pl.batch, None))


# ---- the samplers: words depend on first_item + i -------------------------------------------------------------------------------------------------------------
FIRST_ITEM = 5


def sampler_shape(comps):
    def shape(L, n):
        return {"items": {"buf": comps * L * n}, "writable": ("buf",),
                "limits": [("first_item + batch", lambda b: FIRST_ITEM + b, 1 << 32), ("workgroups", lambda b: b * L * chunks_of(n), K_MAX_GRID)]}
    return shape


def _sampler(comps, comp, twin, launch, start=None):
    """twin(p, item) -> [comps][L][N] with only component `comp` written over `start_item`; the other components must still hold what they held"""
    def run(r, pl, call):
        L, n = r.L, r.n
        words = comps * L * n
        if start is None:
            buf = wb.sentinel(pl.batch, words, call.dev)
            first = np.full((P, comps, L, n), wb.SENTINEL, np.uint64)
        else:                                                              # DPFHE_NOISE_ADD: the start words are tiled
            first = start(r)
            buf = wb.sentinel(pl.batch, words, call.dev)
            wb.tile_into(buf, first.reshape(P, -1), pl.batch)
        call.t["buf"] = buf
        _cabi.check(launch(r, buf.data_ptr(), pl.batch), "sampler")
        import torch
        torch.cuda.synchronize(call.dev)
        what = f"sampler on {r.kind} N = {n}, batch {pl.batch}"
        try:
            wb.check_sampled("buf", buf, pl, lambda i: twin(r.p, i, first[i % P].copy()), n)
            wb.check_no_sentinel("buf", buf, pl, comp * L * n, (comp + 1) * L * n, n)
            wb.check_tail("buf", buf, pl, n)
            for other in range(comps):                                     # a component the call does not write: still sentinel (set) / the tiled start words (add),
                if other != comp:                                          # over the whole buffer, not only on the sampled items
                    lo, hi = other * L * n, (other + 1) * L * n
                    wb.check_columns("buf", buf, pl, lo, hi, None if start is None else first.reshape(P, -1)[:, lo:hi], n)
        except wb.WideBatchError as e:
            raise wb.WideBatchError(e.buffer, e.kind, e.item, e.limb, e.word, e.line, f"{what}: {e}") from e
    return run


def _expand(comps, comp):
    twin = lambda p, i, held: wire.expand_host(p, 1, comps, comp, SEED, first_item=FIRST_ITEM + i, out=held[None])[0]
    launch = lambda r, ptr, batch: r.ctx._lib.dpfhe_expand_uniform(r.ctx.handle, ptr, batch, comps, comp, SEED, FIRST_ITEM, None)
    return _sampler(comps, comp, twin, launch)


def _noise(comps, comp, kind, param, add):
    twin = lambda p, i, held: wire.noise_host(p, 1, comps, comp, kind, param, 2, SEED, first_item=FIRST_ITEM + i, add=add, out=held[None])[0]
    launch = lambda r, ptr, batch: r.ctx._lib.dpfhe_sample_noise(r.ctx.handle, ptr, batch, comps, comp, kind, param, 2, SEED, FIRST_ITEM,
                                                                   _cabi.NOISE_ADD if add else 0, None)
    start = (lambda r: r.words(r.orc, (P, comps), 450)) if add else None
    return _sampler(comps, comp, twin, launch, start)


case("expand-fold2", "A", "fold2", 12, sampler_shape(2))(_expand(2, 1))
case("B-expand-fold2", "B", "fold2", 12, sampler_shape(1))(_expand(1, 0))
for _kn, _kind_id, _param in (("ternary", _cabi.NOISE_TERNARY, 0), ("cbd21", _cabi.NOISE_CBD21, 0), ("flood", _cabi.NOISE_FLOOD, 100)):
    case(f"noise-{_kn}-set-fold2", "A", "fold2", 12, sampler_shape(2))(_noise(2, 1, _kind_id, _param, False))
    case(f"noise-{_kn}-add-fold2", "A", "fold2", 12, sampler_shape(2))(_noise(2, 0, _kind_id, _param, True))
case("B-noise-ternary-fold2", "B", "fold2", 12, sampler_shape(1))(_noise(1, 0, _cabi.NOISE_TERNARY, 0, False))


# ---- sums of products and products with a complement factor: the groups are tiled ------------------------------------------------------------------------------
TERMS = 2
IN_OUT_NTT = _cabi.IN_NTT | _cabi.OUT_NTT


def mul_sum_shape(shared, flags):
    def shape(L, n):
        poly = L * n
        items = {"a": TERMS * 2 * poly, "out3": 3 * poly}
        if not shared:
            items["b"] = TERMS * 2 * poly
        return {"items": items, "writable": ("out3",), "extra": (0 if flags else SCRATCH_DEFAULT_BYTES) + (TERMS * 2 * poly * 8 if shared else 0),
                "limits": [("groups x terms", lambda g: g * TERMS, K_MAX_GRID // (2 * L)), ("workgroups", lambda g: g * 3 * L * chunks_of(n), K_MAX_GRID)]}
    return shape


def _mul_sum(shared, flags):
    def run(r, pl, call):
        import test_gpu_mul_sum as ms
        lib, h, orc, L, n = r.ctx._lib, r.ctx.handle, r.orc, r.L, r.n
        ntt = lambda v: orc.ntt_fwd(v.reshape(-1, L, n), threads=0).reshape(v.shape)
        a = r.words(orc, (P, TERMS, 2), 600)
        b = r.words(orc, (1 if shared else P, TERMS, 2), 610)
        want = ms.reference(r, a, b)
        if flags:
            a, b, want = ntt(a), ntt(b), ntt(want)
        pa = call.inp("a", a)
        pb = call.shared("b", b) if shared else call.inp("b", b)
        po = call.out("out3", want)
        call.run(f"dpfhe_ct_mul_sum flags {flags}", lib.dpfhe_ct_mul_sum(h, po, pa, pb, pl.batch, TERMS, 1 if shared else pl.batch, flags, None))
    return run


case("ct_mul_sum-own-fold2", "A", "fold2", 12, mul_sum_shape(False, 0))(_mul_sum(False, 0))
case("ct_mul_sum-own-ntt-fold2", "A", "fold2", 12, mul_sum_shape(False, IN_OUT_NTT))(_mul_sum(False, IN_OUT_NTT))
case("ct_mul_sum-shared-fold2", "A", "fold2", 12, mul_sum_shape(True, 0))(_mul_sum(True, 0))


def complement_shape(K, flags):
    def shape(L, n):
        poly = L * n
        items = {"b": 2 * poly, "out3": max(K, 1) * 3 * poly}
        if K:
            items["a"] = K * 2 * poly
        return {"items": items, "writable": ("out3",), "extra": 0 if flags else SCRATCH_DEFAULT_BYTES,
                "limits": [("groups x (terms + 1)", lambda g: g * (K + 1), K_MAX_GRID // (3 * L))]}
    return shape


def _complement(K, flags):
    """K = 1 without the self products: out3 [G][1][3][L][N]; K = 0 with them: out3 [G][3][L][N] - both periodic in the group (with both, the output is
    the products and then the self products: two stretches)"""
    def run(r, pl, call):
        import test_gpu_mul_complement as mc
        lib, h, orc, L, n = r.ctx._lib, r.ctx.handle, r.orc, r.L, r.n
        ntt = lambda v: orc.ntt_fwd(v.reshape(-1, L, n), threads=0).reshape(v.shape)
        kap = mc.residues(r)
        b = r.words(orc, (P, 2), 910)
        a = r.words(orc, (P, max(K, 1), 2), 900)[:, :K]
        want = mc.layout(*mc.reference(r, a, b, kap), K == 0)
        if flags:
            a, b, want = ntt(np.ascontiguousarray(a)), ntt(b), ntt(want)
        pa = call.inp("a", np.ascontiguousarray(a)) if K else None
        pb, pk, po = call.inp("b", b), call.shared("kappa", kap), call.out("out3", want)
        call.run(f"dpfhe_ct_mul_complement K = {K} flags {flags}", lib.dpfhe_ct_mul_complement(h, po, pa, pb, pk, pl.batch, K, int(K == 0), flags, None))
    return run


case("ct_mul_complement-fold2", "A", "fold2", 12, complement_shape(1, 0))(_complement(1, 0))
case("ct_mul_complement-ntt-fold2", "A", "fold2", 12, complement_shape(1, IN_OUT_NTT))(_complement(1, IN_OUT_NTT))
case("ct_mul_complement-self-fold2", "A", "fold2", 12, complement_shape(0, 0))(_complement(0, 0))


def complement_both_shape(L, n):
    poly = L * n
    return {"items": {"a": 2 * poly, "b": 2 * poly, "out3": 2 * 3 * poly}, "writable": ("out3",), "extra": SCRATCH_DEFAULT_BYTES,
            "limits": [("groups x (terms + 1)", lambda g: g * 2, K_MAX_GRID // (3 * L))]}


@case("ct_mul_complement-both-fold2", "A", "fold2", 12, complement_both_shape)
def _complement_both(r, pl, call):
    """K = 1 with the self products: out3 is the G products and then the G self products - two stretches, each periodic in the group"""
    import test_gpu_mul_complement as mc
    lib, h, orc, L, n = r.ctx._lib, r.ctx.handle, r.orc, r.L, r.n
    kap = mc.residues(r)
    b = r.words(orc, (P, 2), 911)
    a = r.words(orc, (P, 1, 2), 901)
    prods, selfs = mc.reference(r, a, b, kap)
    G = pl.batch
    pa, pb, pk = call.inp("a", a), call.inp("b", b), call.shared("kappa", kap)
    po = call.stretched_out("out3", [(G, prods.reshape(P, -1)), (G, selfs.reshape(P, -1))], 3 * L * n)
    call.run("dpfhe_ct_mul_complement K = 1 with self", lib.dpfhe_ct_mul_complement(h, po, pa, pb, pk, G, 1, 1, 0, None))


# ---- the fused key-switching passes ----------------------------------------------------------------------------------------------------------------------------
def relin_rescale_shape(L, n):
    Ld = L - 1
    return {"items": {"in": 3 * Ld * n, "work": 2 * L * n, "out2": 2 * (Ld - 1) * n}, "writable": ("work", "out2"), "extra": Ld * 2 * L * n * 8,
            "limits": [("workgroups", lambda b: b * Ld * L * chunks_of(n), K_MAX_GRID)]}


@case("relinearize_rescale_hybrid-f64_under_fold", "A", "f64_under_fold", 12, relin_rescale_shape)
def _relin_rescale(r, pl, call):
    from oracle.cbind import Oracle
    lib, h, orc, L = r.ctx._lib, r.ctx.handle, r.orc, r.L
    data = Oracle(r.p.log2_n, r.p.moduli[:-1], r.p.psi[:-1])
    key = r.words(orc, (L - 1, 2), 303)
    ct3 = r.words(data, (P, 3), 313)
    want = data.rescale(orc.keyswitch_hybrid(ct3, key, 3, threads=0))
    i, k, w, o = call.inp("in", ct3), call.shared("key", key), call.scratch("work", 2 * L * r.n), call.out("out2", want)
    call.run("dpfhe_relinearize_rescale_hybrid", lib.dpfhe_relinearize_rescale_hybrid(h, o, i, k, w, pl.batch, None))


def lincomb_shape(L, n):
    return {"items": {"x": 2 * L * n, "out": 2 * (L - 1) * n}, "writable": ("out",), "limits": [("workgroups", lambda b: b * 2 * L * chunks_of(n), K_MAX_GRID)]}


@case("lincomb_rescale-fold", "A", "fold", 12, lincomb_shape)
def _lincomb(r, pl, call):
    import fused_rescale_ref as fr
    lib, h = r.ctx._lib, r.ctx.handle
    x, w = fr.lincomb_inputs(r.p, 1, P, 8)                                # x [1][P][2][L][N]: one term, the items behind each other
    px, pw, po = call.inp("x", x[0]), call.shared("w", w), call.out("out", fr.lincomb_rescale_twin(r.p, x, w))
    call.run("dpfhe_lincomb_rescale", lib.dpfhe_lincomb_rescale(h, po, px, pw, 1, pl.batch, None))


# ---- rotations on a two-limb extended context (one data limb under the special prime: the smallest legal limb count) ---------------------------------------------
def u32(values):
    import ctypes as C
    return (C.c_uint32 * max(len(values), 1))(*[int(v) for v in values])


def data_oracle(r):
    from oracle.cbind import Oracle
    return Oracle(r.p.log2_n, r.p.moduli[:-1], r.p.psi[:-1])


def rot_shape(**words_in_n):
    """per-item words of every batched buffer as (data limbs, extended limbs) multiples of N: name -> (a, b) means (a Ld + b L) N"""
    def shape(L, n):
        Ld = L - 1
        items = {k: (a * Ld + b * L) * n for k, (a, b) in words_in_n.items()}
        writable = tuple(k for k in items if k not in ("in2", "in_qp", "addends", "in"))
        return {"items": items, "writable": writable, "extra": Ld * 2 * L * n * 8,
                "limits": [("workgroups", lambda b: b * 2 * L * L * chunks_of(n), K_MAX_GRID), ("items", lambda b: b, 0xFFFFFFFF)]}
    return shape


@case("rotate_hybrid_grouped-fold2", "A", "fold2", 12, rot_shape(in2=(2, 0), work=(0, 2), rotated=(2, 0), out2=(2, 0)))
def _rotate_grouped(r, pl, call):
    """one key, the whole batch its group"""
    lib, h, orc, L, n = r.ctx._lib, r.ctx.handle, r.orc, r.L, r.n
    Ld, data = L - 1, data_oracle(r)
    g = 2 * n - 1
    key = r.words(orc, (Ld, 2), 321)
    cts = r.words(data, (P, 2), 341)
    want = orc.keyswitch_hybrid(data.apply_galois(cts.reshape(-1, Ld, n), g).reshape(cts.shape), key, 2, threads=0)
    i, k, w, t, o = call.inp("in2", cts), call.shared("keys", key), call.scratch("work", 2 * L * n), call.scratch("rotated", 2 * Ld * n), call.out("out2", want)
    call.run("dpfhe_rotate_hybrid_grouped", lib.dpfhe_rotate_hybrid_grouped(h, o, i, u32([g]), 1, pl.batch, k, w, t, None))


@case("rotate_add_hybrid-fold2", "A", "fold2", 12, rot_shape(in2=(2, 0), work=(0, 2), out2=(2, 0)))
def _rotate_add(r, pl, call):
    import test_gpu_rotate_add as ra
    lib, h, orc, L, n = r.ctx._lib, r.ctx.handle, r.orc, r.L, r.n
    Ld, data = L - 1, data_oracle(r)
    elts = ra.ladder_elements(n, 1)
    keys = r.words(orc, (1, Ld, 2), 304)
    ct = r.words(data, (P, 2), 314)
    i, k, w, o = call.inp("in2", ct), call.shared("keys", keys), call.scratch("work", 2 * L * n), call.out("out2", ra.reference(r, ct, elts, keys))
    call.run("dpfhe_rotate_add_hybrid", lib.dpfhe_rotate_add_hybrid(h, o, i, u32(elts), k, w, None, 1, pl.batch, None))


def hoisted_keys(r, seed):
    """P rotations: elements and keys [P][Ld][2][L][N], tiled with the same odd period (the 64-rotation launch slices never align with it)"""
    L, Ld, n = r.L, r.L - 1, r.n
    elts = [5, 2 * n - 1, pow(3, 7, 2 * n)]
    keys = r.orc.fill(P * Ld * 2, seed).reshape(P, Ld, 2, L, n)
    keys[P - 1] = r.words(r.orc, (Ld, 2), seed + 1)
    return elts, keys


def hoisted_qp_shape(L, n):
    Ld = L - 1
    return {"items": {"keys": Ld * 2 * L * n, "out_qp": 2 * L * n}, "writable": ("out_qp",), # (d_out_qp is block 0, the rotations and the tail: one item more than the batch + 1 of a writable buffer; then in2, in_ntt and digits with their tails)
            "extra": (2 * L + 2 * Ld + 2 * 2 * Ld + 2 * Ld * L) * n * 8,
            "limits": [("rotation workgroups", lambda b: (b + 1) * L * 8, K_MAX_GRID)]}


@case("rotate_hoisted_qp-fold2", "A", "fold2", 12, hoisted_qp_shape)
def _rotate_hoisted_qp(r, pl, call):
    """one token, the ROTATIONS tiled: d_keys [k][Ld][2][L][N] and d_out_qp [1 + k][1][2][L][N] cross B32 - the launcher's d_keys + first * key_words and
    d_out_qp + (1 + first) * ... bases and the hoisted_qp kernels' offsets.  d_out_qp is block 0 (the token's lift) and then the periodic rotations"""
    lib, h, orc, L, n = r.ctx._lib, r.ctx.handle, r.orc, r.L, r.n
    Ld, data = L - 1, data_oracle(r)
    elts3, keys = hoisted_keys(r, 700)
    ct = r.words(data, (1, 2), 702)
    want = orc.rotate_hoisted_qp(ct[0], elts3, keys, threads=0)            # [1 + P][2][L][N]
    k = pl.batch
    i, pk = call.shared("in2", ct), call.inp("keys", keys)
    a, d = call.small_scratch("in_ntt", 2 * Ld * n), call.small_scratch("digits", Ld * L * n)
    o = call.stretched_out("out_qp", [(1, want[:1]), (k, want[1:])], 2 * L * n)
    call.run("dpfhe_rotate_hoisted_qp", lib.dpfhe_rotate_hoisted_qp(h, o, i, 1, u32([elts3[j % P] for j in range(k)]), pk, a, d, k, None))


HOISTED_SLICE = 2046      # rotations per slice of the composed dpfhe_rotate_hybrid_hoisted at N = 16384, L = 2, one token, under the default scratch limit:
                          # scratch_limit_words / (T 2 L N) - 2 (cabi_rotate.hip)


def hoisted_shape(L, n):
    Ld = L - 1
    assert (SCRATCH_DEFAULT_BYTES // 8) // (2 * L * n) - 2 == HOISTED_SLICE
    b32_items = wb.REAL.words["B32"] // (2 * Ld * n)
    margin = -(-b32_items // HOISTED_SLICE) * HOISTED_SLICE - b32_items + 2   # the first slice base past B32 of d_out2, and two items
    return {"items": {"keys": Ld * 2 * L * n, "out2": 2 * Ld * n}, "writable": ("out2",), "margin": margin,
            "extra": SCRATCH_DEFAULT_BYTES + (2 * 2 * Ld + Ld * L + 2 * L) * n * 8,
            "limits": [("rotation workgroups", (HOISTED_SLICE + 1) * L * 8, K_MAX_GRID), ("widest transform grid", HOISTED_SLICE * 2 * L, K_MAX_GRID)]}


@case("rotate_hybrid_hoisted-composed-fold2-n16384", "A", "fold2", 14, hoisted_shape)
def _rotate_hoisted(r, pl, call):
    """N = 16384: the composed path (d_work and d_rotated0 unused: NULL), one token, the rotations tiled: d_keys and d_out2 cross B32, in slices of 2046
    rotations - the slice bases d_keys + r0 * key_words (past B32 from the sixth slice, r0 = 10230) and d_out2 + r0 * ... (the plan's margin puts the last one past B32)"""
    lib, h, orc, L, n = r.ctx._lib, r.ctx.handle, r.orc, r.L, r.n
    Ld, data = L - 1, data_oracle(r)
    elts3, keys = hoisted_keys(r, 350)
    ct = r.words(data, (1, 2), 352)
    want = orc.rotate_hoisted(ct[0], elts3, keys, threads=0)               # [P][2][Ld][N]
    k = pl.batch
    assert (k - 2) // HOISTED_SLICE * HOISTED_SLICE * 2 * Ld * n >= wb.REAL.words["B32"]
    i, pk, d, o = call.shared("in2", ct), call.inp("keys", keys), call.small_scratch("digits", Ld * L * n), call.out("out2", want)
    call.run("dpfhe_rotate_hybrid_hoisted", lib.dpfhe_rotate_hybrid_hoisted(h, o, i, 1, u32([elts3[j % P] for j in range(k)]), pk, None, None, d, k, None))


def hoisted_fused_shape(L, n):
    Ld = L - 1
    return {"items": {"keys": Ld * 2 * L * n, "work": 2 * L * n, "out2": 2 * Ld * n}, "low_items": {"rotated0": Ld * n}, "writable": ("work", "out2", "rotated0"),
            "extra": (2 * Ld + 2 * Ld * L) * n * 8,
            "limits": [("rescale workgroups", lambda b: b * 2 * Ld * chunks_of(n), K_MAX_GRID), ("key-switch workgroups", lambda b: b * L * 2 + 8, K_MAX_GRID)]}


@case("rotate_hybrid_hoisted-fused-fold2", "A", "fold2", 12, hoisted_fused_shape)
def _rotate_hoisted_fused(r, pl, call):
    """N = 4096: the fused path (launch_hoisted_ks, the d_work + first * ... and d_rotated0 + first * ... slice bases, the rescale with addend), one token, the
    rotations tiled.  With all four batched buffers past B32 the call takes 11 x 4 GiB: d_keys, d_work and d_out2 cross B32, d_rotated0 (Ld N words per
    rotation) crosses B31"""
    lib, h, orc, L, n = r.ctx._lib, r.ctx.handle, r.orc, r.L, r.n
    Ld, data = L - 1, data_oracle(r)
    elts3, keys = hoisted_keys(r, 360)
    ct = r.words(data, (1, 2), 362)
    want = orc.rotate_hoisted(ct[0], elts3, keys, threads=0)               # [P][2][Ld][N]
    k = pl.batch
    i, pk, w, t = call.shared("in2", ct), call.inp("keys", keys), call.scratch("work", 2 * L * n), call.scratch("rotated0", Ld * n)
    d, o = call.small_scratch("digits", Ld * L * n), call.out("out2", want)
    call.run("dpfhe_rotate_hybrid_hoisted", lib.dpfhe_rotate_hybrid_hoisted(h, o, i, 1, u32([elts3[j % P] for j in range(k)]), pk, w, t, d, k, None))


def rotate_batch_shape(L, n):
    Ld = L - 1
    return {"items": {"keys": Ld * 2 * L * n, "work": 2 * L * n}, "low_items": {"rotated": 2 * Ld * n, "out2": 2 * Ld * n}, "writable": ("work", "rotated", "out2"),
            "extra": 2 * Ld * n * 8, "limits": [("workgroups", lambda b: b * 2 * L * L * chunks_of(n), K_MAX_GRID)]}


@case("rotate_hybrid_batch-fold2", "A", "fold2", 12, rotate_batch_shape)
def _rotate_batch(r, pl, call):
    """one input, a key per rotation.  With all four batched buffers past B32 the call takes 24.4 GiB, over the cap: d_keys and d_work (4 N words per rotation)
    cross B32, d_rotated and d_out2 (2 N words) cross B31"""
    lib, h, orc, L, n = r.ctx._lib, r.ctx.handle, r.orc, r.L, r.n
    Ld, data = L - 1, data_oracle(r)
    elts3, keys = hoisted_keys(r, 320)
    ct = r.words(data, (1, 2), 331)
    want = np.stack([orc.keyswitch_hybrid(data.apply_galois(ct.reshape(-1, Ld, n), elts3[j]).reshape(ct.shape), np.ascontiguousarray(keys[j]), 2, threads=0)[0]
                     for j in range(P)])
    k = pl.batch
    i, pk, w, t, o = call.shared("in2", ct), call.inp("keys", keys), call.scratch("work", 2 * L * n), call.scratch("rotated", 2 * Ld * n), call.out("out2", want)
    call.run("dpfhe_rotate_hybrid_batch", lib.dpfhe_rotate_hybrid_batch(h, o, i, 1, u32([elts3[j % P] for j in range(k)]), pk, w, t, k, None))


def relin_lincomb_shape(L, n):
    Ld = L - 1
    return {"items": {"in": 3 * Ld * n, "work": 2 * L * n, "z0": 2 * Ld * n}, "low_items": {"out2": 2 * (Ld - 1) * n}, "writable": ("work", "out2"),
            "extra": Ld * 2 * L * n * 8, "limits": [("workgroups", lambda b: b * Ld * L * chunks_of(n), K_MAX_GRID)]}


@case("relinearize_lincomb_rescale_hybrid-f64_under_fold", "A", "f64_under_fold", 12, relin_lincomb_shape)
def _relin_lincomb(r, pl, call):
    """one term.  With every batched buffer past B32 the call takes 27 GiB, over the cap: d_in, d_work and the term cross B32, d_out2 (one limb fewer, two
    components) crosses B31"""
    import ctypes as C
    import relin_lincomb_ref as rl
    import test_gpu_relin_lincomb as tl
    lib, h, orc, L = r.ctx._lib, r.ctx.handle, r.orc, r.L
    Ld, data = L - 1, data_oracle(r)
    key = r.words(orc, (Ld, 2), 303)
    ct3 = r.words(data, (P, 3), 313)
    terms, w = rl.terms_and_weights(r.p, 1, P, 324)
    assert len(terms) == 1 and terms[0].shape[2] == Ld
    want = tl.reference(r, ct3, key, terms, w)
    i, k, z, pw = call.inp("in", ct3), call.shared("key", key), call.inp("z0", terms[0]), call.shared("w", w)
    sc, o = call.scratch("work", 2 * L * r.n), call.out("out2", want)
    ptrs, limbs = (C.c_void_p * 1)(z), u32([Ld])
    call.run("dpfhe_relinearize_lincomb_rescale_hybrid", lib.dpfhe_relinearize_lincomb_rescale_hybrid(h, o, i, k, sc, ptrs, limbs, 1, pw, pl.batch, None))


@case("switch_key_qp-fold2", "A", "fold2", 12, rot_shape(in2=(2, 0), out_qp=(0, 2)))
def _switch_key_qp(r, pl, call):
    lib, h, orc, L = r.ctx._lib, r.ctx.handle, r.orc, r.L
    Ld, data = L - 1, data_oracle(r)
    keys = r.words(orc, (2, Ld, 2), 731)[:1]
    items = r.words(data, (P, 2), 741)
    i, k, o = call.inp("in2", items), call.shared("keys", keys), call.out("out_qp", orc.switch_key_qp(items, keys[0], threads=0))
    call.run("dpfhe_switch_key_qp", lib.dpfhe_switch_key_qp(h, o, i, k, 1, pl.batch, None))


@case("rescale_bsgs-fold2", "A", "fold2", 12, rot_shape(in_qp=(0, 2), addends=(2, 0), out2=(2, 0)))
def _rescale_bsgs(r, pl, call):
    from class_edges import rescale_bsgs_reference
    lib, h, orc = r.ctx._lib, r.ctx.handle, r.orc
    data = data_oracle(r)
    rot = r.words(data, (1, P, 2), 750)
    t_qp = r.words(orc, (P, 2), 751)
    i, a, o = call.inp("in_qp", t_qp), call.inp("addends", rot[0]), call.out("out2", rescale_bsgs_reference(orc, data, t_qp, rot))
    call.run("dpfhe_rescale_bsgs", lib.dpfhe_rescale_bsgs(h, o, i, a, 1, pl.batch, None))


def galois_shape(inplace):
    def shape(L, n):
        items = {"io": L * n} if inplace else {"in": L * n, "out": L * n}
        return {"items": items, "writable": ("io",) if inplace else ("out",), "limits": [("residue polynomials", lambda b: b * L, K_MAX_GRID)]}
    return shape


def _ntt_inv_galois(inplace):
    """one element per item, tiled with the same odd period: the 64-element launch slices (kMaxGaloisBatch) never align with it"""
    def run(r, pl, call):
        lib, h, orc, n = r.ctx._lib, r.ctx.handle, r.orc, r.n
        elts3 = [5, 2 * n - 1, pow(3, 7, 2 * n)]
        x = r.words(orc, (P, 1), 720)
        inv = orc.ntt_inv(x, threads=0)
        want = np.stack([orc.apply_galois(inv[e], elts3[e]) for e in range(P)])
        elts = u32([elts3[i % P] for i in range(pl.batch)])
        if inplace:
            io = call.inout("io", x, want)
            return call.run("dpfhe_ntt_inv_galois in place", lib.dpfhe_ntt_inv_galois(h, io, io, 1, elts, pl.batch, None))
        i, o = call.inp("in", x), call.out("out", want)
        call.run("dpfhe_ntt_inv_galois", lib.dpfhe_ntt_inv_galois(h, o, i, 1, elts, pl.batch, None))
    return run


case("ntt_inv_galois-fold2", "A", "fold2", 12, galois_shape(False))(_ntt_inv_galois(False))
case("ntt_inv_galois-in-place-fold2", "A", "fold2", 12, galois_shape(True))(_ntt_inv_galois(True))


# ---- plaintext adds, compact records, the encoders: held to their host twins on the period ----------------------------------------------------------------------
T_PLAIN = 65537


def plain_add_shape(scaled, one_to_one):
    def shape(L, n):
        ct, pt = 2 * L * n, (n if scaled else L * n)
        items = {"io": ct, "plain": pt} if one_to_one else {"in": ct, "out": ct}
        return {"items": items, "writable": ("io",) if one_to_one else ("out",), "extra": 0 if one_to_one else pt * 8,
                "limits": [("workgroups", lambda b: b * chunks_of(n), K_MAX_GRID)]}
    return shape


def _plain_add(scaled, one_to_one):
    """one_to_one: a plaintext per ciphertext, in place (the plaintexts are the smallest buffer); otherwise one broadcast plaintext, out of place"""
    def run(r, pl, call):
        import ctypes as C
        lib, h, orc, L, n = r.ctx._lib, r.ctx.handle, r.orc, r.L, r.n
        rng = np.random.default_rng(21)
        ct = r.words(orc, (P, 2), 460)
        items = P if one_to_one else 1
        plain = rng.integers(0, 1 << 32, (items, n), dtype=np.uint64) if scaled else r.words(orc, (items,), 461)
        want = ct.copy()
        m = (C.c_uint64 * L)(*r.p.moduli)
        if scaled:
            rc = lib.dpfhe_add_plain_scaled_host(m, L, r.p.log2_n, want.ctypes.data, ct.ctypes.data, plain.ctypes.data, P, 2, items, T_PLAIN, 1)
        else:
            rc = lib.dpfhe_add_plain_host(m, L, r.p.log2_n, want.ctypes.data, ct.ctypes.data, plain.ctypes.data, P, 2, items, 1)
        _cabi.check(rc, "the host twin")
        if one_to_one:
            io, pp = call.inout("io", ct, want), call.inp("plain", plain)
            pin, plain_items = io, pl.batch
        else:
            pin, pp, io = call.inp("in", ct), call.shared("plain", plain), call.out("out", want)
            plain_items = 1
        if scaled:
            call.run("dpfhe_add_plain_scaled", lib.dpfhe_add_plain_scaled(h, io, pin, pp, pl.batch, 2, plain_items, T_PLAIN, 1, None))
        else:
            call.run("dpfhe_add_plain", lib.dpfhe_add_plain(h, io, pin, pp, pl.batch, 2, plain_items, 1, None))
    return run


for _scaled in (False, True):
    for _one in (False, True):
        case(f"add_plain{'_scaled' if _scaled else ''}-{'one-to-one' if _one else 'broadcast'}-fold2", "A", "fold2", 12,
             plain_add_shape(_scaled, _one))(_plain_add(_scaled, _one))

BITS = (60, 60)


def compact_shape(L, n):
    return {"items": {"in": 2 * L * n, "out": n * sum(BITS) // 64}, "writable": ("out",), "limits": [("workgroups", lambda b: b * chunks_of(n) * 2, K_MAX_GRID)]}


@case("compact-fold2", "A", "fold2", 12, compact_shape)
def _compact(r, pl, call):
    lib, h, orc, n = r.ctx._lib, r.ctx.handle, r.orc, r.n
    words = r.words(orc, (P, 2), 470)
    want = wire.compact_host(r.p, words, *BITS)
    assert want.dtype == np.uint8 and want.size == P * n * sum(BITS) // 8
    i, o = call.inp("in", words), call.out("out", np.ascontiguousarray(want).view(np.uint64), n * BITS[0] // 64)
    call.run("dpfhe_compact", lib.dpfhe_compact(h, o, i, pl.batch, BITS[0], BITS[1], None))


def encode_shape(slot_words_per_n, plain):
    def shape(L, n):
        return {"items": {"slots": n // slot_words_per_n, "out": n if plain else L * n}, "writable": ("out",),
                "limits": [("items", lambda b: b, K_MAX_GRID // n), ("residue polynomials", lambda b: b * L, K_MAX_GRID)]}
    return shape


def _encode_slots(flags):
    def run(r, pl, call):
        import encode_ref
        lib, n = r.ctx._lib, r.n
        slots = np.random.default_rng(31).integers(0, T_PLAIN, (P, n), dtype=np.uint32)
        slots[0, :4] = [0, 1, T_PLAIN - 1, T_PLAIN // 2]
        want = encode_ref.twin(r.p.moduli, r.p.log2_n, T_PLAIN, slots)
        if flags & _cabi.ENCODE_NTT:
            want = r.orc.ntt_fwd(want, threads=0)
        i, o = call.inp("slots", slots.view(np.uint64), n // 2), call.out("out", want)
        call.run(f"dpfhe_encode_slots flags {flags}", lib.dpfhe_encode_slots(r.ctx.encoder(T_PLAIN), o, i, pl.batch, flags, None))
    return run


def _encode_complex(flags):
    def run(r, pl, call):
        import complex_encode_ref
        lib, n = r.ctx._lib, r.n
        rng = np.random.default_rng(41)
        z = (rng.standard_normal((P, n // 2)) + 1j * rng.standard_normal((P, n // 2))).astype(np.complex128)
        scale = 2.0 ** 45
        want = complex_encode_ref.twin(r.p.moduli, r.p.log2_n, z, scale)
        if flags & _cabi.ENCODE_NTT:
            want = r.orc.ntt_fwd(want, threads=0)
        i, o = call.inp("slots", np.ascontiguousarray(z).view(np.uint64), n), call.out("out", want)
        call.run(f"dpfhe_encode_complex flags {flags}", lib.dpfhe_encode_complex(r.ctx.complex_encoder(), o, i, pl.batch, scale, flags, None))
    return run


for _flags, _tag in ((0, ""), (_cabi.ENCODE_NTT, "-ntt")):
    case(f"encode_slots{_tag}-fold2", "A", "fold2", 12, encode_shape(2, False))(_encode_slots(_flags))
    case(f"encode_complex{_tag}-fold2", "A", "fold2", 12, encode_shape(1, False))(_encode_complex(_flags))


# ---- re-randomisation: in place, words depend on first_item + i --------------------------------------------------------------------------------------------------
FLOOD_BITS = 100


def rerandomize_shape(L, n):
    return {"items": {"ct": 2 * L * n, "work": 3 * L * n}, "writable": ("ct", "work"), "extra": 2 * L * n * 8,
            "limits": [("first_item + batch", lambda b: FIRST_ITEM + b, 1 << 32), ("residue polynomials", lambda b: b * 4 * L, K_MAX_GRID)]}


@case("rerandomize-fold2", "A", "fold2", 12, rerandomize_shape)
def _rerandomize(r, pl, call):
    import torch
    from test_gpu_rerandomize import _rerandomize_ref
    lib, h, orc, L, n = r.ctx._lib, r.ctx.handle, r.orc, r.L, r.n
    ct = r.words(orc, (P, 2), 480)
    pk = r.words(orc, (2,), 481)
    buf = wb.sentinel(pl.batch, 2 * L * n, call.dev)
    wb.tile_into(buf, ct.reshape(P, -1), pl.batch)
    call.t["ct"] = buf
    ppk, pw = call.shared("pk", pk), call.scratch("work", 3 * L * n)
    _cabi.check(lib.dpfhe_rerandomize(h, buf.data_ptr(), ppk, pl.batch, FLOOD_BITS, SEED, FIRST_ITEM, pw, None), "dpfhe_rerandomize")
    torch.cuda.synchronize(call.dev)
    wb.check_sampled("ct", buf, pl, lambda i: _rerandomize_ref(r.p, ct[i % P][None], pk, FLOOD_BITS, SEED, FIRST_ITEM + i)[0], n)
    wb.check_tail("ct", buf, pl, n)
    call.check("dpfhe_rerandomize")


# the peaks the CPU test pins (bytes): buffers + one sentinel tail item per writable buffer + the compare temporaries
TIER_B_PEAKS = {
    "B-ntt-ntt_fwd-fold2-n4096": 34762588160,
    "B-ntt-ntt_inv-fold2-n4096": 34762588160,
    "B-ntt-ntt_fwd-fold2-n65536": 34765537280,
    "B-ntt-ntt_inv-fold2-n65536": 34765537280,
    "B-negate-in-place": 34762588160,
    "B-add-out-is-a": 69122457600,
    "B-canonicalize-fold2": 34762588160,
    "B-reduce-thin-fold2": 34762915840,
    "B-expand-fold2": 34762588160,
    "B-noise-ternary-fold2": 34762588160,
}


# ---- the test: every case, one after another in one process --------------------------------------------------------------------------------------------------
PEAKS = {}      # id -> (planned peak, measured torch peak)


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_wide(rigs, c):
    import torch
    pl = c.plan()
    wb.release()
    free, total = wb.free_bytes()
    if c.tier == "A":
        assert free >= pl.peak, f"{c.id}: {free} bytes free of {total}, the case needs {pl.peak}: a tier A case never skips"
    elif free < pl.peak + wb.HEADROOM:
        pytest.skip(f"{c.id}: {free} bytes free of {total}, the case needs {pl.peak} + {wb.HEADROOM} of headroom for the other jobs on the card")
    r = rigs(c.kind, c.log2n)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    call = Call(r, pl)
    try:
        c.run(r, pl, call)
        peak = torch.cuda.max_memory_allocated() - base
        PEAKS[c.id] = (pl.peak, peak)
        print(f"{c.id}: batch {pl.batch}, planned peak {pl.peak}, torch peak {peak}")
        assert peak <= pl.peak, f"{c.id}: the buffers and the compares took {peak} bytes, the plan says {pl.peak}"
    finally:
        call.close()
