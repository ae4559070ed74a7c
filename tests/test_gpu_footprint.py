"""-m gpu: every device entry point of include/dpfhe.h held to its declared memory footprint (tests/footprint.py).

The value tests hand the C ABI buffers of exactly the documented size from torch's caching allocator: 512-byte aligned, rounded up, most often still
holding the previous answer of the same shape.  Here all pointer arguments of a call are carved out of ONE uploaded array, each at the weakest alignment
the header admits (16 bytes and not 32; d_w of dpfhe_matvec_scalar 8 bytes and not 16), each between guard bands of at least one whole item, every
scratch buffer at exactly the header's size.  The call runs twice, the array filled with 0xDEADBEEFCAFEF00D and then with its complement (neither is a
residue: both are >= 2^60).  Both times
  * the outputs equal the oracle (oracle.cbind.Oracle, threads=0) word for word - an unwritten word cannot, and a result that read its scratch or its
    output before writing it cannot under both patterns;
  * every word outside the output / scratch / in-out regions - guards, inputs, stride gaps - is bit-identical to the host snapshot.
Nothing is compared with the library's own earlier output, and there is no tolerance anywhere.  Contexts come from class_edges.edge_moduli, so the
per-class kernels are the ones launched; shapes come from the constants in the code (kMaxGaloisBatch = 64, kQpRotGroup = 16, kReduceSplits = 15,
kHalvesMinPolys = 2304, kQuartersMinPolys = 768, the 4-row / 2-token matvec tiles, 1024-word streaming tiles) so that every tail path has a case.

Entry -> test (an entry of include/dpfhe.h that writes device memory and is not in this table is a gap):
  dpfhe_ntt_fwd / _inv / _fwd_oop / _inv_oop                          test_transforms
  dpfhe_dyadic_mul / _mul_add / dpfhe_add / dpfhe_sub / dpfhe_negate   test_streaming_entries (out apart, out == a, out == b)
  dpfhe_multiply_plain / dpfhe_apply_galois / dpfhe_rescale            test_streaming_entries
  dpfhe_canonicalize_sum / dpfhe_copy / dpfhe_reduce_sum               test_streaming_entries, test_reduce_sum
  dpfhe_ct_mul                                                         test_ct_mul, test_composed_forms_do_not_depend_on_the_scratch_arena
  dpfhe_debug_ct_mul_trace / dpfhe_ctx_autotune                        test_diagnostic_and_tuning_entries
  dpfhe_relinearize / dpfhe_switch_key                                 test_key_switching, test_composed_forms_...
  dpfhe_relinearize_hybrid / dpfhe_switch_key_hybrid                   test_hybrid_key_switching
  dpfhe_rotate_hybrid_batch / _grouped / _hoisted                      test_hybrid_rotations, test_composed_forms_...
  dpfhe_rotate_hoisted_qp / dpfhe_switch_key_qp / dpfhe_rescale_bsgs   test_deferred_division_stages, test_composed_forms_...
  dpfhe_ntt_inv_galois                                                 test_deferred_division_stages (d_out apart and d_out == d_in)
  dpfhe_base_extend / dpfhe_scale_round                                test_base_extension_strides, test_exact_multiplier_calls
  dpfhe_matvec_plain / _scalar / _plain_multi                          test_matvec
  dpfhe_comm_allgather / dpfhe_comm_allreduce_sum                      test_collectives_world_of_one
  dpfhe_expand_uniform / dpfhe_add_plain_scaled / dpfhe_compact / dpfhe_encode_slots / dpfhe_sample_noise / dpfhe_rerandomize
                                                                       their own sentinel tests (test_gpu_seeded / _plain_add / _compact / _encode / _rerandomize)
The same table (dpfhe_ctx_autotune apart: a set-up call that synchronises) is held to the stream contract of the header - the caller's stream, enqueue
only, no allocation in steady state - by tests/test_gpu_stream_contract.py, which runs these test bodies with Case.gate set (tests/stream_gate.py).
Read-side overruns of inputs cannot be seen without a fault and are not looked for."""
import ctypes as C

import numpy as np
import pytest

from class_edges import Rig, catalogue, reported_classes, rescale_bsgs_reference
from deeppowers_amd import _cabi
from deeppowers_amd.params import FheParams
from footprint import Arena, run_both_patterns
from oracle.cbind import Oracle

pytestmark = pytest.mark.gpu


# ---- rigs ---------------------------------------------------------------------------------------------------------------------------------------------------
class ParamsRig(Rig):
    """a Rig over given parameters (class_edges.Rig takes a kind)"""

    def __init__(self, kind, p):
        from deeppowers_amd.evaluator import Context, Evaluator
        self.kind, self.p = kind, p
        self.L, self.n = p.n_limbs, p.n
        self.orc = Oracle.from_params(p)
        self.ctx = Context(p, 0)
        self.ev = Evaluator(self.ctx)
        self.qcol = np.array(p.moduli, np.uint64)[:, None]
        assert self.ctx.limb_classes == reported_classes(p), (kind, self.ctx.limb_classes)


def _pick(log2n, entries):
    cat = catalogue(log2n)
    ps = [cat[name][i] for name, i in entries]
    assert len({q for q, _ in ps}) == len(ps)
    return FheParams(log2n, tuple(q for q, _ in ps), tuple(w for _, w in ps))


def make_rig(kind, log2n):
    """class_edges kinds, and: fold3 (three fold edge primes: 768 words per polynomial at N = 256, so word totals that are no multiple of 1024),
    fold5 / shoup5 (five limbs: the exact multiply with two level limbs)"""
    if kind == "fold3":
        return ParamsRig(kind, _pick(log2n, [("fold_edge", i) for i in range(3)]))
    if kind == "fold5":
        return ParamsRig(kind, _pick(log2n, [("fold_edge", i) for i in range(4)] + [("fold_near", 0)]))
    if kind == "shoup5":
        return ParamsRig(kind, _pick(log2n, [("shoup60", i) for i in range(4)] + [("shoup_above_59", 0)]))
    return Rig(kind, log2n)


@pytest.fixture
def rig():
    made = []

    def make(kind, log2n):
        r = make_rig(kind, log2n)
        made.append(r)
        return r
    yield make
    for r in made:
        r.close()


def ids(ctxs):
    return [f"{k}_n{1 << ln}" for k, ln in ctxs]


SMALL = [(k, ln) for ln in (8, 12, 13) for k in ("fold", "mixed")]          # one launch per class on the mixture
HYBRID = [("f64_under_fold", 12)]                                            # data limbs of one class under a special prime of another
COMPOSED = [("fold", 14), ("shoup", 14)]                                     # composed forms, scratch from the per-stream arena
HUGE = [("fold", 16)]                                                        # the two-kernel split transform; streaming entries


# ---- one call through the arena ------------------------------------------------------------------------------------------------------------------------------
class At:
    """the address callable a case's fn gets: at(name[, extra_words]) is a device address; at.stream is the stream argument of the call - None (the null
    stream) in footprint mode, the gated stream's pointer in gated mode"""

    def __init__(self, arena, base, stream=None):
        self.arena, self.base, self.stream = arena, base, stream

    def __call__(self, name, extra=0):
        return self.arena.address(self.base, name, extra)


class Case:
    """the buffers of one call and what its outputs must hold; run(what, fn): fn(at) makes the call(s), at(name[, extra_words]) is a device address and
    at.stream the stream to pass.  tests/test_gpu_stream_contract.py sets Case.gate (a stream_gate.Gate) for the time of a test: run() is then
    run_gated(), the same buffers and the same expected words held to the stream contract instead of the two fill patterns"""
    gate = None

    def __init__(self, r):
        self.r, self.ar, self.want = r, Arena(), {}

    def inp(self, name, a, item, **kw):
        self.ar.carve(name, a.size, "input", item, data=a, **kw)

    def out(self, name, words, item, want, **kw):
        self.ar.carve(name, words, "output", item, **kw)
        self.want[name] = want

    def scratch(self, name, words, item):
        self.ar.carve(name, words, "scratch", item)

    def inout(self, name, a, item, want):
        self.ar.carve(name, a.size, "inout", item, data=a)
        self.want[name] = want

    def run(self, what, fn):
        if Case.gate is not None:
            return self.run_gated(what, fn, Case.gate)
        import torch
        dev = self.r.ctx.device

        def call(buf):
            t = torch.from_numpy(buf.view(np.int64)).to(dev)
            rc = fn(At(self.ar, t.data_ptr()))
            _cabi.check(rc or 0, what)
            torch.cuda.synchronize(dev)
            return t.cpu().numpy().view(np.uint64)
        try:
            return run_both_patterns(self.ar, call, self.want)
        except AssertionError as e:
            raise AssertionError(f"{what} on {self.r.kind} N = {self.r.n}: {e}") from e

    def run_gated(self, what, fn, gate):
        """the same call through stream_gate.run_gated: on the gate's stream, behind the gate, with the inputs arriving after it (one fill pattern)"""
        from stream_gate import run_gated

        def call(t, stream):
            rc = fn(At(self.ar, t.data_ptr(), stream))
            _cabi.check(rc or 0, what)
        return run_gated(gate, self.ar, self.want, call, scratch_bytes=lambda: self.r.ctx.scratch_bytes, what=f"{what} on {self.r.kind} N = {self.r.n}")


def data_oracle(r):
    return Oracle(r.p.log2_n, r.p.moduli[:-1], r.p.psi[:-1])


def u32(values):
    return (C.c_uint32 * max(len(values), 1))(*[int(v) for v in values])


# ---- transforms ---------------------------------------------------------------------------------------------------------------------------------------------
THRESHOLD = {13: 2304, 14: 768}     # kHalvesMinPolys / kQuartersMinPolys residue polynomials (fold contexts)


@pytest.mark.parametrize("kind,log2n", SMALL + COMPOSED + HUGE, ids=ids(SMALL + COMPOSED + HUGE))
def test_transforms(rig, kind, log2n):
    """in place (in-out) and out of place, both directions on non-image data, 1, 3 and 5 RNS polynomials; on the fold contexts at N = 8192 / 16384 also
    an odd count one item past the halves / quarters threshold"""
    r = rig(kind, log2n)
    lib, h, poly = r.ctx._lib, r.ctx.handle, r.L * r.n
    counts = [1, 3, 5]
    if kind == "fold" and log2n in THRESHOLD:
        counts.append(-(-THRESHOLD[log2n] // r.L) + 1)
        assert counts[-1] % 2 == 1 and counts[-1] * r.L >= THRESHOLD[log2n]
    for count in counts:
        x = r.words(r.orc, (count,), 100 + count)
        for name, want in (("dpfhe_ntt_fwd", r.orc.ntt_fwd(x, threads=0)), ("dpfhe_ntt_inv", r.orc.ntt_inv(x, threads=0))):
            c = Case(r)
            c.inout("io", x, poly, want)
            c.run(f"{name} x{count}", lambda at: getattr(lib, name)(h, at("io"), count, at.stream))
            c = Case(r)
            c.inp("in", x, poly)
            c.out("out", x.size, poly, want)
            c.run(f"{name}_oop x{count}", lambda at: getattr(lib, name + "_oop")(h, at("out"), at("in"), count, at.stream))


# ---- streaming entries ---------------------------------------------------------------------------------------------------------------------------------------
STREAMING = SMALL + [("fold3", 8)] + HUGE


@pytest.mark.parametrize("kind,log2n", STREAMING, ids=ids(STREAMING))
def test_streaming_entries(rig, kind, log2n):
    """the dyadic family with every aliasing the header allows (out apart, out == a, out == b; the accumulator of mul_add in-out), multiply_plain and
    negate apart and in place, apply_galois, rescale, canonicalize_sum, copy: 1 and 3 polynomials (on fold3 at N = 256: 768 and 2304 words, no multiple
    of 1024)"""
    r = rig(kind, log2n)
    lib, h, L, n, orc = r.ctx._lib, r.ctx.handle, r.L, r.n, r.orc
    poly = L * n
    for count in (1, 3):
        x = r.words(orc, (count,), 400 + count)
        y = r.words(orc, (count,), 410 + count)
        y[0] = y[0][:, ::-1]
        acc = r.words(orc, (count,), 420 + count)
        for op in ("mul", "add", "sub"):
            fn = getattr(lib, {"mul": "dpfhe_dyadic_mul", "add": "dpfhe_add", "sub": "dpfhe_sub"}[op])
            want = orc.dyadic(op, x, y)
            c = Case(r)
            c.inp("a", x, poly)
            c.inp("b", y, poly)
            c.out("out", x.size, poly, want)
            c.run(f"{op} x{count}", lambda at: fn(h, at("out"), at("a"), at("b"), count, at.stream))
            c = Case(r)
            c.inout("a", x, poly, want)
            c.inp("b", y, poly)
            c.run(f"{op} x{count}, out == a", lambda at: fn(h, at("a"), at("a"), at("b"), count, at.stream))
            c = Case(r)
            c.inp("a", x, poly)
            c.inout("b", y, poly, want)
            c.run(f"{op} x{count}, out == b", lambda at: fn(h, at("b"), at("a"), at("b"), count, at.stream))
        c = Case(r)
        c.inout("acc", acc, poly, orc.dyadic("mul_add", x, y, acc=acc))
        c.inp("a", x, poly)
        c.inp("b", y, poly)
        c.run(f"dpfhe_dyadic_mul_add x{count}", lambda at: lib.dpfhe_dyadic_mul_add(h, at("acc"), at("a"), at("b"), count, at.stream))
        want = orc.dyadic("negate", x)
        c = Case(r)
        c.inp("a", x, poly)
        c.out("out", x.size, poly, want)
        c.run(f"dpfhe_negate x{count}", lambda at: lib.dpfhe_negate(h, at("out"), at("a"), count, at.stream))
        c = Case(r)
        c.inout("a", x, poly, want)
        c.run(f"dpfhe_negate x{count}, out == a", lambda at: lib.dpfhe_negate(h, at("a"), at("a"), count, at.stream))
        pt = r.words(orc, (2,), 430)[1]                                   # q - 1 in every word
        want = orc.dyadic("mul", x, np.ascontiguousarray(np.broadcast_to(pt, x.shape)))
        c = Case(r)
        c.inp("a", x, poly)
        c.inp("pt", pt, poly)
        c.out("out", x.size, poly, want)
        c.run(f"dpfhe_multiply_plain x{count}", lambda at: lib.dpfhe_multiply_plain(h, at("out"), at("a"), at("pt"), count, at.stream))
        c = Case(r)
        c.inout("a", x, poly, want)
        c.inp("pt", pt, poly)
        c.run(f"dpfhe_multiply_plain x{count}, out == a", lambda at: lib.dpfhe_multiply_plain(h, at("a"), at("a"), at("pt"), count, at.stream))
        for g in (5, 2 * n - 1):
            c = Case(r)
            c.inp("in", x, poly)
            c.out("out", x.size, poly, orc.apply_galois(x, g))
            c.run(f"dpfhe_apply_galois x{count} g = {g}", lambda at: lib.dpfhe_apply_galois(h, at("out"), at("in"), count, g, at.stream))
        c = Case(r)
        c.inp("in", x, poly)
        c.out("out", count * (L - 1) * n, (L - 1) * n, orc.rescale(x))
        c.run(f"dpfhe_rescale x{count}", lambda at: lib.dpfhe_rescale(h, at("out"), at("in"), count, at.stream))
        # sums of up to 15 canonical residues (15 q < 2^64): the reference is the exact remainder
        terms = np.random.default_rng(count).integers(1, 16, x.shape, dtype=np.uint64)
        terms[0] = 15
        sums = x * terms
        c = Case(r)
        c.inout("io", sums, poly, sums % r.qcol)
        c.run(f"dpfhe_canonicalize_sum x{count}", lambda at: lib.dpfhe_canonicalize_sum(h, at("io"), count, at.stream))
    src = np.random.default_rng(7).integers(0, 1 << 63, 1024 * 7 + 2, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    for words in (2, 1022, 1024 * 7 + 2):
        c = Case(r)
        c.inp("src", src[:words], words)
        c.out("dst", words, words, src[:words])
        c.run(f"dpfhe_copy {words} words", lambda at: lib.dpfhe_copy(h, at("dst"), at("src"), words, at.stream))


@pytest.mark.parametrize("kind,log2n", SMALL + HUGE, ids=ids(SMALL + HUGE))
def test_reduce_sum(rig, kind, log2n):
    """count 1, 17 and (where the input stays small) 520, 2 and 3 components: 17 and 520 put more than one item in each of the 15 splits"""
    r = rig(kind, log2n)
    lib, h, L, n, orc = r.ctx._lib, r.ctx.handle, r.L, r.n, r.orc
    for comps in (2, 3):
        for count in (1, 17, 520):
            if count * comps * L * n > (1 << 24) + (1 << 20):             # 520 at N = 256 everywhere and, with 2 components, on fold at N = 4096
                continue
            cts = orc.fill(count * comps, 440 + count).reshape(count, comps, L, n)
            cts[:, :, :, : n // 2] = r.qcol - np.uint64(1)
            c = Case(r)
            c.inp("in", cts, comps * L * n)
            c.out("out", comps * L * n, comps * L * n, orc.reduce_sum(cts.ravel(), comps))
            c.run(f"dpfhe_reduce_sum {count} x {comps}", lambda at: lib.dpfhe_reduce_sum(h, at("out"), at("in"), count, comps, at.stream))


# ---- the fused / composed multiply --------------------------------------------------------------------------------------------------------------------------
def ct_mul_cases(r, batches, squares):
    """(label, a, b or None for squaring, flags, want) over both input and both output domains"""
    L, n, orc = r.L, r.n, r.orc
    ntt = lambda v: orc.ntt_fwd(v.reshape(-1, L, n), threads=0).reshape(v.shape)
    for batch in batches:
        a = r.words(orc, (batch, 2), 200 + batch)
        b = r.words(orc, (batch, 2), 210 + batch)
        b[0] = np.roll(b[0], n // 16, axis=-1)
        an, bn = ntt(a), ntt(b)
        for other, othern, tag in ((b, bn, ""),) + (((None, None, " squared"),) if batch in squares else ()):
            want = orc.ct_mul(a, a if other is None else other, threads=0)
            wantn = ntt(want)
            for flags in range(4):
                yield (f"dpfhe_ct_mul x{batch}{tag} flags {flags}", an if flags & 1 else a, (othern if flags & 1 else other), flags, wantn if flags & 2 else want)


def run_ct_mul(r, label, a, b, flags, want):
    lib, h, poly = r.ctx._lib, r.ctx.handle, r.L * r.n
    batch = a.shape[0]
    c = Case(r)
    c.inp("a2", a, 2 * poly)
    if b is not None:
        c.inp("b2", b, 2 * poly)
    c.out("out3", batch * 3 * poly, 3 * poly, want)
    c.run(label, lambda at: lib.dpfhe_ct_mul(h, at("out3"), at("a2"), at("b2" if b is not None else "a2"), batch, flags, at.stream))


@pytest.mark.parametrize("kind,log2n", SMALL + COMPOSED, ids=ids(SMALL + COMPOSED))
def test_ct_mul(rig, kind, log2n):
    """batch 1, 3 and 5, both input and both output domains, squaring with d_a2 == d_b2; on the fold contexts at N = 4096 / 8192 the quad and the dual
    form of the coefficient-domain multiply"""
    r = rig(kind, log2n)
    two_forms = r.ctx.uses_fold and log2n in (12, 13)
    try:
        for label, a, b, flags, want in ct_mul_cases(r, (1, 3, 5), (3,)):
            for form in (("quad", "dual") if two_forms and flags == 0 else (None,)):
                if form:
                    r.ctx.set_ct_mul_variant(form)
                run_ct_mul(r, f"{label} {form or ''}", a, b, flags, want)
    finally:
        if two_forms:
            r.ctx.set_ct_mul_variant("quad" if log2n == 12 else "dual")


def test_diagnostic_and_tuning_entries(rig):
    """dpfhe_debug_ct_mul_trace: the product as usual, the 12 words per workgroup of d_trace are timestamps (writable, not compared);
    dpfhe_ctx_autotune: overwrites caller scratch of work_words words and nothing else"""
    r = rig("fold", 12)
    lib, h, poly, orc = r.ctx._lib, r.ctx.handle, r.L * r.n, r.orc
    batch = 3
    a, b = r.words(orc, (batch, 2), 250), r.words(orc, (batch, 2), 251)
    c = Case(r)
    c.inp("a2", a, 2 * poly)
    c.inp("b2", b, 2 * poly)
    c.out("out3", batch * 3 * poly, 3 * poly, orc.ct_mul(a, b, threads=0))
    c.scratch("trace", batch * r.L * 12, 12)
    c.run("dpfhe_debug_ct_mul_trace", lambda at: lib.dpfhe_debug_ct_mul_trace(h, at("out3"), at("a2"), at("b2"), batch, at("trace"), at.stream))
    words = 2 * 7 * poly                                                  # two synthetic ciphertext pairs with their products
    c = Case(r)
    c.scratch("work", words, 7 * poly)
    try:
        c.run("dpfhe_ctx_autotune", lambda at: lib.dpfhe_ctx_autotune(h, at("work"), words, 2, at.stream))
    finally:
        lib.dpfhe_tune_cache_clear()                                      # (the probe's result must not reach contexts that later tests create)


# ---- key switching -------------------------------------------------------------------------------------------------------------------------------------------
def run_relinearize(r, batch, seed=300):
    lib, h, L, orc = r.ctx._lib, r.ctx.handle, r.L, r.orc
    poly = L * r.n
    c3 = orc.ct_mul(r.words(orc, (batch, 2), seed), r.words(orc, (batch, 2), seed + 1), threads=0)
    evk = r.words(orc, (L, 2), seed + 2)
    c = Case(r)
    c.inp("in3", c3, 3 * poly)
    c.inp("evk", evk, 2 * poly)
    c.out("out2", batch * 2 * poly, 2 * poly, orc.relinearize(c3, evk, threads=0))
    c.run(f"dpfhe_relinearize x{batch}", lambda at: lib.dpfhe_relinearize(h, at("out2"), at("in3"), at("evk"), batch, at.stream))


@pytest.mark.parametrize("kind,log2n", SMALL + COMPOSED, ids=ids(SMALL + COMPOSED))
def test_key_switching(rig, kind, log2n):
    """dpfhe_relinearize and dpfhe_switch_key, batch 1 and 3"""
    r = rig(kind, log2n)
    lib, h, L, orc = r.ctx._lib, r.ctx.handle, r.L, r.orc
    poly = L * r.n
    for batch in (1, 3):
        run_relinearize(r, batch)
        ct = r.words(orc, (batch, 2), 305)
        key = r.words(orc, (L, 2), 306)
        c = Case(r)
        c.inp("in2", ct, 2 * poly)
        c.inp("key", key, 2 * poly)
        c.out("out2", batch * 2 * poly, 2 * poly, orc.switch_key(ct, key, threads=0))
        c.run(f"dpfhe_switch_key x{batch}", lambda at: lib.dpfhe_switch_key(h, at("out2"), at("in2"), at("key"), batch, at.stream))


EXTENDED = SMALL + HYBRID + COMPOSED


@pytest.mark.parametrize("kind,log2n", EXTENDED, ids=ids(EXTENDED))
def test_hybrid_key_switching(rig, kind, log2n):
    """dpfhe_relinearize_hybrid / dpfhe_switch_key_hybrid, batch 1 and 3, d_work at exactly batch * 2 * L * N words"""
    r = rig(kind, log2n)
    lib, h, L, n, orc = r.ctx._lib, r.ctx.handle, r.L, r.n, r.orc
    Ld, data = L - 1, data_oracle(r)
    key = r.words(orc, (Ld, 2), 303)
    for batch in (1, 3):
        for comps, name in ((3, "dpfhe_relinearize_hybrid"), (2, "dpfhe_switch_key_hybrid")):
            ct = r.words(data, (batch, comps), 310 + comps)
            c = Case(r)
            c.inp("in", ct, comps * Ld * n)
            c.inp("key", key, 2 * L * n)
            c.scratch("work", batch * 2 * L * n, 2 * L * n)
            c.out("out2", batch * 2 * Ld * n, 2 * Ld * n, orc.keyswitch_hybrid(ct, key, comps, threads=0))
            c.run(f"{name} x{batch}", lambda at: getattr(lib, name)(h, at("out2"), at("in"), at("key"), at("work"), batch, at.stream))


def rotation_keys(r, k, seed):
    L, Ld, n = r.L, r.L - 1, r.n
    elts = [pow(3, i + 1, 2 * n) for i in range(k)]
    elts[-1] = 2 * n - 1
    keys = r.orc.fill(k * Ld * 2, seed).reshape(k, Ld, 2, L, n)
    keys[k - 1] = r.words(r.orc, (Ld, 2), seed + 1)
    return elts, keys


def run_rotate_hoisted(r, k, T, seed=350):
    lib, h, L, n, orc = r.ctx._lib, r.ctx.handle, r.L, r.n, r.orc
    Ld, data = L - 1, data_oracle(r)
    elts, keys = rotation_keys(r, k, seed)
    cts = r.words(data, (T, 2), seed + 2)
    want = np.stack([orc.rotate_hoisted(cts[t], elts, keys, threads=0) for t in range(T)], axis=1)      # [k][T][2][Ld][N]: rotation-major
    c = Case(r)
    c.inp("in2", cts, 2 * Ld * n)
    c.inp("keys", keys, Ld * 2 * L * n)
    c.scratch("work", k * T * 2 * L * n, 2 * L * n)
    c.scratch("rotated0", k * T * Ld * n, Ld * n)
    c.scratch("digits", T * Ld * L * n, Ld * L * n)
    c.out("out2", k * T * 2 * Ld * n, 2 * Ld * n, want)
    c.run(f"dpfhe_rotate_hybrid_hoisted {k} rotations of {T}",
          lambda at: lib.dpfhe_rotate_hybrid_hoisted(h, at("out2"), at("in2"), T, u32(elts), at("keys"), at("work"), at("rotated0"), at("digits"), k, at.stream))


@pytest.mark.parametrize("kind,log2n", EXTENDED, ids=ids(EXTENDED))
def test_hybrid_rotations(rig, kind, log2n):
    """dpfhe_rotate_hybrid_batch (one input and one per rotation), _grouped (groups of 1 and 3), _hoisted (1 and 3 tokens): 1 and 5 rotations and, at
    N = 4096 on the four-limb contexts, 65 - one past the 64-rotation launch group; every scratch buffer at exactly the header's size"""
    r = rig(kind, log2n)
    lib, h, L, n, orc = r.ctx._lib, r.ctx.handle, r.L, r.n, r.orc
    Ld, data = L - 1, data_oracle(r)
    ct_words, key_words = 2 * Ld * n, Ld * 2 * L * n
    rotated = lambda ct, g, key: orc.keyswitch_hybrid(data.apply_galois(ct[None], g), key, 2, threads=0)[0]
    for k in (1, 5) + ((65,) if log2n == 12 and L <= 4 else ()):
        elts, keys = rotation_keys(r, k, 320 + k)
        for n_in in sorted({1, k}):
            cts = r.words(data, (n_in, 2), 330 + n_in)
            c = Case(r)
            c.inp("in2", cts, ct_words)
            c.inp("keys", keys, key_words)
            c.scratch("work", k * 2 * L * n, 2 * L * n)
            c.scratch("rotated", k * ct_words, ct_words)
            c.out("out2", k * ct_words, ct_words, np.stack([rotated(cts[i if n_in > 1 else 0], elts[i], keys[i]) for i in range(k)]))
            c.run(f"dpfhe_rotate_hybrid_batch {k} rotations of {n_in}",
                  lambda at: lib.dpfhe_rotate_hybrid_batch(h, at("out2"), at("in2"), n_in, u32(elts), at("keys"), at("work"), at("rotated"), k, at.stream))
        for group in (1, 3):
            items = r.words(data, (k * group, 2), 340 + group)
            c = Case(r)
            c.inp("in2", items, ct_words)
            c.inp("keys", keys, key_words)
            c.scratch("work", k * group * 2 * L * n, 2 * L * n)
            c.scratch("rotated", k * group * ct_words, ct_words)
            c.out("out2", k * group * ct_words, ct_words, np.stack([rotated(items[i], elts[i // group], keys[i // group]) for i in range(k * group)]))
            c.run(f"dpfhe_rotate_hybrid_grouped {k} x {group}",
                  lambda at: lib.dpfhe_rotate_hybrid_grouped(h, at("out2"), at("in2"), u32(elts), k, group, at("keys"), at("work"), at("rotated"), at.stream))
        for T in (1, 3):
            run_rotate_hoisted(r, k, T)


# ---- the deferred-division stages --------------------------------------------------------------------------------------------------------------------------
def run_rotate_hoisted_qp(r, k, T, seed=700):
    lib, h, L, n, orc = r.ctx._lib, r.ctx.handle, r.L, r.n, r.orc
    Ld, data = L - 1, data_oracle(r)
    elts, keys = rotation_keys(r, k, seed) if k else ([], None)
    cts = r.words(data, (T, 2), seed + 2)
    want = np.stack([orc.rotate_hoisted_qp(cts[t], elts, keys, threads=0) for t in range(T)], axis=1)   # [1 + k][T][2][L][N]
    c = Case(r)
    c.inp("in2", cts, 2 * Ld * n)
    if k:
        c.inp("keys", keys, Ld * 2 * L * n)
    c.scratch("in_ntt", T * 2 * Ld * n, 2 * Ld * n)
    c.scratch("digits", T * Ld * L * n, Ld * L * n)
    c.out("out_qp", (1 + k) * T * 2 * L * n, T * 2 * L * n, want)
    c.run(f"dpfhe_rotate_hoisted_qp {k} rotations of {T}",
          lambda at: lib.dpfhe_rotate_hoisted_qp(h, at("out_qp"), at("in2"), T, u32(elts), at("keys") if k else None, at("in_ntt"), at("digits"), k, at.stream))


@pytest.mark.parametrize("kind,log2n", EXTENDED, ids=ids(EXTENDED))
def test_deferred_division_stages(rig, kind, log2n):
    """dpfhe_rotate_hoisted_qp at (rotations, tokens) = (0, 2), (5, 1), (17, 3) - the last one past the 16-rotation group -, dpfhe_switch_key_qp at
    (keys, group) = (1, 3), (5, 1), (9, 4), dpfhe_rescale_bsgs with 0, 1 and 6 addends of batch 3, dpfhe_ntt_inv_galois at 70 x 3 and 1 x 1, apart and
    in place"""
    r = rig(kind, log2n)
    lib, h, L, n, orc = r.ctx._lib, r.ctx.handle, r.L, r.n, r.orc
    Ld, data = L - 1, data_oracle(r)
    for k, T in ((0, 2), (5, 1), (17, 3)):
        run_rotate_hoisted_qp(r, k, T)
    for k, group in ((1, 3), (5, 1), (9, 4)):
        keys = r.words(orc, (max(k, 2), Ld, 2), 730 + k)[:k]
        items = r.words(data, (k * group, 2), 740 + k)
        want = np.concatenate([orc.switch_key_qp(items[i * group:(i + 1) * group], keys[i], threads=0) for i in range(k)])
        c = Case(r)
        c.inp("in2", items, 2 * Ld * n)
        c.inp("keys", keys, Ld * 2 * L * n)
        c.out("out_qp", k * group * 2 * L * n, 2 * L * n, want)
        c.run(f"dpfhe_switch_key_qp {k} x {group}", lambda at: lib.dpfhe_switch_key_qp(h, at("out_qp"), at("in2"), at("keys"), k, group, at.stream))
    batch = 3
    rot = r.words(data, (6, batch, 2), 750)
    t_qp = r.words(orc, (batch, 2), 751)
    for n_add in (0, 1, 6):
        c = Case(r)
        c.inp("in_qp", t_qp, 2 * L * n)
        if n_add:
            c.inp("addends", rot[:n_add], 2 * Ld * n)
        c.out("out2", batch * 2 * Ld * n, 2 * Ld * n, rescale_bsgs_reference(orc, data, t_qp, rot[:n_add]))
        c.run(f"dpfhe_rescale_bsgs {n_add} addends",
              lambda at: lib.dpfhe_rescale_bsgs(h, at("out2"), at("in_qp"), at("addends") if n_add else None, n_add, batch, at.stream))
    for k, per in ((70, 3), (1, 1)):
        elts = [pow(3, 5 * i, 2 * n) for i in range(k)]
        if k > 2:
            elts[2] = elts[k - 1] = 2 * n - 1
        x = r.words(orc, (k, per), 720)
        inv = orc.ntt_inv(x, threads=0)
        want = np.stack([orc.apply_galois(inv[e], elts[e]) for e in range(k)])
        c = Case(r)
        c.inp("in", x, per * L * n)
        c.out("out", x.size, per * L * n, want)
        c.run(f"dpfhe_ntt_inv_galois {k} x {per}", lambda at: lib.dpfhe_ntt_inv_galois(h, at("out"), at("in"), per, u32(elts), k, at.stream))
        c = Case(r)
        c.inout("io", x, per * L * n, want)
        c.run(f"dpfhe_ntt_inv_galois {k} x {per}, d_out == d_in", lambda at: lib.dpfhe_ntt_inv_galois(h, at("io"), at("io"), per, u32(elts), k, at.stream))


# ---- base extension and scale-and-round: the item strides ------------------------------------------------------------------------------------------------------
def strided(n_items, stride_limbs, limbs, n):
    """(buffer words, segments) of n_items items of `limbs` limbs, stride_limbs limbs apart: the stride gaps are guards"""
    return ((n_items - 1) * stride_limbs + limbs) * n, [(p * stride_limbs * n, limbs * n) for p in range(n_items)]


def run_base_extend(r, label, xs, src0, dst0, nd, in_stride, out_stride, want):
    lib, h, n = r.ctx._lib, r.ctx.handle, r.n
    ns, items = xs.shape[-2], xs.size // (xs.shape[-2] * n)
    c = Case(r)
    words, seg = strided(items, in_stride, ns, n)
    c.ar.carve("in", words, "input", in_stride * n, data=xs, segments=seg)
    words, seg = strided(items, out_stride, nd, n)
    c.out("out", words, out_stride * n, want, segments=seg)
    c.run(f"dpfhe_base_extend {label} strides {in_stride} -> {out_stride}",
          lambda at: lib.dpfhe_base_extend(h, at("out"), out_stride, at("in"), in_stride, src0, ns, dst0, nd, items, at.stream))


def run_scale_round(r, label, w, drop0, ndrop, keep0, nkeep, mul, out_stride, want):
    lib, h, L, n = r.ctx._lib, r.ctx.handle, r.L, r.n
    items = w.size // (L * n)
    c = Case(r)
    c.inp("in", w, L * n)
    words, seg = strided(items, out_stride, nkeep, n)
    c.out("out", words, out_stride * n, want, segments=seg)
    c.run(f"dpfhe_scale_round {label} stride {out_stride}",
          lambda at: lib.dpfhe_scale_round(h, at("out"), out_stride, at("in"), drop0, ndrop, keep0, nkeep, mul, items, at.stream))


@pytest.mark.parametrize("kind,log2n", SMALL, ids=ids(SMALL))
def test_base_extension_strides(rig, kind, log2n):
    """the three range cases of test_streaming_operations_at_the_class_edges, each with stride == limbs, with out_stride_limbs = n_dst + 3 and, for
    dpfhe_base_extend, also with in_stride_limbs = n_src + 2: the gaps hold the fill pattern before and must hold it after (a read from an input gap gives
    a wrong word under at least one pattern)"""
    r = rig(kind, log2n)
    L, orc = r.L, r.orc
    w = r.words(orc, (3,), 407)
    for src0, ns, dst0, nd in ((0, 2, 0, L), (L - 2, 2, 0, L - 2), (0, L - 1, L - 1, 1)):
        xs = np.ascontiguousarray(w[:, src0:src0 + ns])
        want = orc.base_extend(xs, src0, dst0, nd)
        for in_stride, out_stride in ((ns, nd), (ns, nd + 3), (ns + 2, nd + 3)):
            run_base_extend(r, (src0, ns, dst0, nd), xs, src0, dst0, nd, in_stride, out_stride, want)
    for drop0, ndrop, keep0, nkeep, mul in ((L - 1, 1, 0, L - 1, 65537), (0, 2, 2, L - 2, 1), (0, 1, 1, L - 1, (1 << 20) + 7)):
        want = orc.scale_round(w, drop0, ndrop, keep0, nkeep, mul)
        for out_stride in (nkeep, nkeep + 3):
            run_scale_round(r, (drop0, ndrop, keep0, nkeep, mul), w, drop0, ndrop, keep0, nkeep, mul, out_stride, want)


@pytest.mark.parametrize("kind", ["fold5", "shoup5"])
def test_exact_multiplier_calls(rig, kind):
    """the three calls ExactMultiplier::multiply makes around dpfhe_ct_mul (fhe_api.cpp), at its strides, for two level limbs on a five-limb context at
    N = 4096, each fed the oracle's output of the step before: operands [batch * 2][2][N] -> all five limbs, the product [batch * 3][5][N] scaled by t / q
    onto the three workspace limbs, and those back to the level"""
    r = rig(kind, 12)
    L, ll, t, n, orc = r.L, 2, 65537, r.n, r.orc
    assert L == 5
    level = Oracle(12, r.p.moduli[:ll], r.p.psi[:ll])
    batch = 3
    a, b = r.words(level, (batch, 2), 770), r.words(level, (batch, 2), 771)
    A, B = orc.base_extend(a, 0, 0, L), orc.base_extend(b, 0, 0, L)
    run_base_extend(r, "operand -> work", a.reshape(batch * 2, ll, n), 0, 0, L, ll, L, A)
    T = orc.ct_mul(np.ascontiguousarray(A), np.ascontiguousarray(B), threads=0)
    W = orc.scale_round(T, 0, ll, ll, L - ll, t)
    run_scale_round(r, "product -> workspace", T.reshape(batch * 3, L, n), 0, ll, ll, L - ll, t, L - ll, W)
    run_base_extend(r, "workspace -> level", W.reshape(batch * 3, L - ll, n), ll, 0, ll, L - ll, ll, orc.base_extend(W, ll, 0, ll))


# ---- matrix-vector products ---------------------------------------------------------------------------------------------------------------------------------
def run_matvec(r, rows, cols):
    lib, h, L, n, orc = r.ctx._lib, r.ctx.handle, r.L, r.n, r.orc
    poly = L * n
    qm1 = r.qcol - np.uint64(1)
    x = orc.fill(cols * 2, 500 + cols).reshape(cols, 2, L, n)
    x[..., : n // 2] = qm1
    W = orc.fill(rows * cols, 510 + cols).reshape(rows, cols, L, n)
    W[0] = qm1
    c = Case(r)
    c.inp("W", W, poly)
    c.inp("x", x, 2 * poly)
    c.out("y", rows * 2 * poly, 2 * poly, orc.matvec_plain(W.ravel(), x.ravel(), rows, cols, threads=0))
    c.run(f"dpfhe_matvec_plain {rows} x {cols}", lambda at: lib.dpfhe_matvec_plain(h, at("y"), at("W"), at("x"), rows, cols, at.stream))
    q = np.array(r.p.moduli, np.uint64)
    w = np.random.default_rng(cols).integers(0, 1 << 62, (rows, cols, L), dtype=np.uint64) % q
    w[: rows - 1] = q - np.uint64(1)
    c = Case(r)
    c.inp("w", w, L, align=8)                                             # d_w is documented as 8-byte aligned: an odd word offset
    c.inp("x", x, 2 * poly)
    c.out("y", rows * 2 * poly, 2 * poly, orc.matvec_scalar(w, x, rows, cols, threads=0))
    c.run(f"dpfhe_matvec_scalar {rows} x {cols}", lambda at: lib.dpfhe_matvec_scalar(h, at("y"), at("w"), at("x"), rows, cols, at.stream))


def run_matvec_multi(r, rows, cols, n_rhs):
    lib, h, L, n, orc = r.ctx._lib, r.ctx.handle, r.L, r.n, r.orc
    poly = L * n
    qm1 = r.qcol - np.uint64(1)
    W = orc.fill(rows * cols, 600 + cols).reshape(rows, cols, L, n)
    W[0] = qm1
    x = orc.fill(cols * n_rhs * 2, 601 + cols).reshape(cols, n_rhs, 2, L, n)
    x[..., : n // 2] = qm1
    want = np.stack([orc.matvec_plain(W.ravel(), np.ascontiguousarray(x[:, t]).ravel(), rows, cols, threads=0) for t in range(n_rhs)], axis=1)
    c = Case(r)
    c.inp("W", W, poly)
    c.inp("x", x, 2 * poly)
    c.out("y", rows * n_rhs * 2 * poly, 2 * poly, want)
    c.run(f"dpfhe_matvec_plain_multi {rows} x {cols} x {n_rhs}", lambda at: lib.dpfhe_matvec_plain_multi(h, at("y"), at("W"), at("x"), rows, cols, n_rhs, at.stream))


MULTI = ((8, 264, 2), (5, 257, 3), (4, 8, 1))                                # the full form, a ragged one, the smallest


@pytest.mark.parametrize("kind", ["fold", "mixed"])
def test_matvec(rig, kind):
    """matvec_plain and matvec_scalar at rows 5 and 8 (off and on the row tile) x cols 127, 129 and 257; matvec_plain_multi at its full, ragged and
    smallest shapes - on the small ring, where W stays small"""
    r = rig(kind, 8)
    for rows in (5, 8):
        for cols in (127, 129, 257):
            run_matvec(r, rows, cols)
    for rows, cols, n_rhs in MULTI:
        run_matvec_multi(r, rows, cols, n_rhs)


@pytest.mark.parametrize("kind", ["fold2", "shoup60"])
def test_matvec_at_n4096(rig, kind):
    """the same entries at N = 4096 on two limbs (the fold and the generic kernels): rows 5 and 8 x 129 columns, and every matvec_plain_multi shape"""
    r = rig(kind, 12)
    for rows in (5, 8):
        run_matvec(r, rows, 129)
    for rows, cols, n_rhs in MULTI:
        run_matvec_multi(r, rows, cols, n_rhs)


# ---- the composed forms and the per-stream scratch arena ------------------------------------------------------------------------------------------------------
def _ct_mul_3(r):
    for label, a, b, flags, want in ct_mul_cases(r, (3,), ()):
        if flags == 0:
            run_ct_mul(r, label, a, b, flags, want)


def _ct_mul_12(r):
    for label, a, b, flags, want in ct_mul_cases(r, (12,), ()):
        if flags == 0:                                                    # coefficient domain in and out: the form that takes the most scratch
            run_ct_mul(r, label, a, b, flags, want)


COMPOSED_CASES = {
    # name: (the case, a larger call of a DIFFERENT entry that dirties the arena first)
    "ct_mul": (_ct_mul_3, lambda r: run_relinearize(r, 6, seed=360)),
    "relinearize": (lambda r: run_relinearize(r, 3), _ct_mul_12),
    "rotate_hybrid_hoisted": (lambda r: run_rotate_hoisted(r, 5, 3), _ct_mul_12),
    "rotate_hoisted_qp": (lambda r: run_rotate_hoisted_qp(r, 5, 3), _ct_mul_12),
}


@pytest.mark.parametrize("entry", list(COMPOSED_CASES))
@pytest.mark.parametrize("kind", ["fold", "shoup"])
def test_composed_forms_do_not_depend_on_the_scratch_arena(rig, kind, entry):
    """N = 16384: the case on a fresh context; on a second context whose per-stream arena a larger call of a different entry has used; and once more after
    set_scratch_limit(2), which forces slices of one item.  Every run must give the oracle's words under both fill patterns - so all runs give the same
    words - and stay inside its footprint"""
    case, dirty = COMPOSED_CASES[entry]
    fresh = rig(kind, 14)
    assert fresh.ctx.scratch_bytes == 0
    case(fresh)
    used = rig(kind, 14)
    dirty(used)
    held = used.ctx.scratch_bytes
    assert held > 0
    case(used)
    assert used.ctx.scratch_bytes >= held
    used.ctx.set_scratch_limit(2)
    case(used)


# ---- the collectives, world size 1 ---------------------------------------------------------------------------------------------------------------------------
def test_collectives_world_of_one(rig):
    """dpfhe_comm_allgather writes words_per_rank words of d_recv; dpfhe_comm_allreduce_sum (all-reduce in place + the mod-q pass) its n_rns_polys
    polynomials - on one rank the reference is the input itself, reduced"""
    r = rig("fold", 12)
    lib, h, poly, orc = r.ctx._lib, r.ctx.handle, r.L * r.n, r.orc
    uid = (C.c_uint8 * 128)()
    _cabi.check(lib.dpfhe_comm_unique_id(uid), "dpfhe_comm_unique_id")
    comm = C.c_void_p()
    _cabi.check(lib.dpfhe_comm_create(C.byref(comm), uid, 0, 1, 0), "dpfhe_comm_create")
    try:
        x = r.words(orc, (3,), 800)
        c = Case(r)
        c.inp("send", x, poly)
        c.out("recv", x.size, poly, x)
        c.run("dpfhe_comm_allgather", lambda at: lib.dpfhe_comm_allgather(comm, at("recv"), at("send"), x.size, at.stream))
        c = Case(r)
        c.inout("io", x, poly, x)
        c.run("dpfhe_comm_allreduce_sum", lambda at: lib.dpfhe_comm_allreduce_sum(comm, h, at("io"), 3, at.stream))
    finally:
        lib.dpfhe_comm_destroy(comm)
