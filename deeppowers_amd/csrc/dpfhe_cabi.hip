// dpfhe_cabi.hip - libdpfhe_hip.so: the C ABI declared in include/dpfhe.h over the gfx950 kernels.  The families whose kernels are kernels_misc.h and
// kernels_large.h: multiply and key switching, rotations, matrix-vector products and sums.  The other families have a unit each (cabi.h lists them
// and states the ABI's conventions).
#include "cabi.h"
#include "fused_rescale.h"
#include "kernels_large.h"
#include "kernels_misc.h"

// ------------------------------------------------------------------------------------------------
// words per thread of the FoldArith matvec kernels: 2 right-hand-side polynomials per workgroup / 4 (kernels_misc.h matvec_fold_kernel)
constexpr int kMatvecWpt2 = 2, kMatvecWpt4 = 1;
constexpr int kMatvecWd = 1;     // columns of W lookahead in the multi-right-hand-side product (2 measured no faster: profiles/r04_ab_matvec_full.txt)
constexpr int kMatvecRt4 = 4;    // rows per workgroup of the 4-polynomial (2-token) kernel (8 measured slower)

// relin_kernel launches (`blocks` = items x L): on the context's policy, or - a MIXTURE of classes - one launch per class present, each over its own limbs
// (relin_kernel maps its workgroups through DevTables::active_map: the digits of every limb still enter every limb's transforms)
static int relin_launch(const dpfhe_ctx* c, int mode, u64* out, const u64* in, const u64* evk, size_t key_stride, unsigned key_group, size_t blocks, hipStream_t s) {
    if (class_mixture(c)) {
        const size_t items = blocks / c->n_limbs;
        return for_each_class(c, c->n_limbs, [&](const auto& tb) { return launch_relin((int)c->log2n, mode, out, in, evk, key_stride, key_group, items * (size_t)tb.n_active, tb, s); });
    }
    return with_policy(c, [&](const auto& tb) { return launch_relin((int)c->log2n, mode, out, in, evk, key_stride, key_group, blocks, tb, s); });
}

// ------------------------------------------------------------------------------------------------
// ---- ring degrees above 8192: the fused kernels stop there (kernels_large.h); the same operations composed from the batched transforms
// and one-pass streaming kernels.  Their scratch comes from per-stream arenas (cabi.h StreamScratch).

static int ct_mul_composed_slice(dpfhe_ctx* c, uint64_t* d_out3, const uint64_t* d_a2, const uint64_t* d_b2, size_t batch, uint32_t flags, hipStream_t s) {
    const size_t L = c->n_limbs, n = (size_t)1 << c->log2n, poly = L * n;
    const int chunks = chunks_of(n);
    const size_t grid = batch * L * (size_t)chunks;
    if (grid > kMaxGrid || !ntt_grid_fits(c, batch * 3 * L)) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_ct_mul", "batch too large for one launch");
    StreamScratch ws(c, s);
    const u64 *pa = d_a2, *pb = d_b2;
    if (!(flags & DPFHE_IN_NTT)) {   // transformed copies of the operands: [a | b], 2 * batch * 2 * L residue polynomials
        const bool square = d_a2 == d_b2;
        if (int rc = ws.alloc((square ? 2 : 4) * batch * poly, "dpfhe_ct_mul (scratch for the transformed operands)")) return rc;
        if (int rc = ntt_launch(c, false, ws.p, d_a2, batch * 2 * L, s)) return rc;
        if (!square) if (int rc = ntt_launch(c, false, ws.p + 2 * batch * poly, d_b2, batch * 2 * L, s)) return rc;
        pa = ws.p;
        pb = square ? ws.p : ws.p + 2 * batch * poly;
    }
    with_ctx_arith(c, [&](auto arith) { hipLaunchKernelGGL((tensor3_kernel<decltype(arith)>), dim3((unsigned)grid), dim3(256), 0, s, d_out3, pa, pb, c->lc, (int)L, (int)n, chunks); });
    if (int rc = check_launch("tensor product kernel launch")) return rc;
    if (!(flags & DPFHE_OUT_NTT)) return ntt_launch(c, true, d_out3, d_out3, batch * 3 * L, s);
    return DPFHE_SUCCESS;
}

// RNS-digit key switch: out2 = [mask-selected components of in] + sum_j NTT^-1( NTT([in_{last comp}]_j mod q_i) (.) evk[j] )
static int key_switch_composed_slice(dpfhe_ctx* c, uint64_t* d_out2, const uint64_t* d_in, int in_comps, int add_mask, const uint64_t* d_evk, size_t batch,
                                     hipStream_t s, const char* what) {
    const size_t L = c->n_limbs, n = (size_t)1 << c->log2n;
    const int chunks = chunks_of(n);
    const size_t lift_grid = batch * L * L * (size_t)chunks;
    if (lift_grid > kMaxGrid || 2 * batch * L * (size_t)chunks > kMaxGrid || !ntt_grid_fits(c, batch * L * L)) return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    StreamScratch ws(c, s);
    if (int rc = ws.alloc(batch * L * L * n, what)) return rc;
    with_ctx_arith(c, [&](auto arith) {
        hipLaunchKernelGGL((lift_rns_digits_kernel<decltype(arith)>), dim3((unsigned)lift_grid), dim3(256), 0, s, ws.p, d_in, in_comps, in_comps - 1, c->lc, (int)L, (int)n, chunks);
    });
    if (int rc = check_launch("digit lift kernel launch")) return rc;
    if (int rc = ntt_launch(c, false, ws.p, ws.p, batch * L * L, s)) return rc;
    const unsigned grid = (unsigned)(batch * L * (size_t)chunks);
    with_ctx_arith(c, [&](auto arith) { hipLaunchKernelGGL((key_inner_product_kernel<decltype(arith)>), dim3(grid), dim3(256), 0, s, d_out2, ws.p, d_evk, c->lc, (int)L, (int)L, (int)n, chunks); });
    if (int rc = check_launch("key inner product kernel launch")) return rc;
    if (int rc = ntt_launch(c, true, d_out2, d_out2, batch * 2 * L, s)) return rc;
    hipLaunchKernelGGL(add_back_kernel, dim3(2 * grid), dim3(256), 0, s, d_out2, d_in, in_comps, add_mask, c->lc, (int)L, (int)n, chunks);
    return check_launch("add-back kernel launch");
}

static int ct_mul_composed(dpfhe_ctx* c, uint64_t* d_out3, const uint64_t* d_a2, const uint64_t* d_b2, size_t batch, uint32_t flags, hipStream_t s) {
    const size_t poly = (size_t)c->n_limbs << c->log2n, per = slice_items(c, batch, 4 * poly);
    return for_slices(batch, per, [&](size_t i, size_t m) { return ct_mul_composed_slice(c, d_out3 + i * 3 * poly, d_a2 + i * 2 * poly, d_b2 + i * 2 * poly, m, flags, s); });
}
static int key_switch_composed(dpfhe_ctx* c, uint64_t* d_out2, const uint64_t* d_in, int in_comps, int add_mask, const uint64_t* d_evk, size_t batch,
                               hipStream_t s, const char* what) {
    const size_t poly = (size_t)c->n_limbs << c->log2n, per = slice_items(c, batch, c->n_limbs * poly);
    return for_slices(batch, per, [&](size_t i, size_t m) {
        return key_switch_composed_slice(c, d_out2 + i * 2 * poly, d_in + i * (size_t)in_comps * poly, in_comps, add_mask, d_evk, m, s, what);
    });
}

// output items are 3 L N words apart, input items 2 L N: a workgroup would overwrite operands another one has not read yet
static bool ct_mul_output_overlaps(const dpfhe_ctx* c, const uint64_t* d_out3, const uint64_t* d_a2, const uint64_t* d_b2, size_t batch) {
    const size_t poly = (size_t)c->n_limbs << c->log2n;
    return overlaps(d_out3, batch * 3 * poly, d_a2, batch * 2 * poly) || overlaps(d_out3, batch * 3 * poly, d_b2, batch * 2 * poly);
}

extern "C" int dpfhe_ct_mul(dpfhe_ctx* c, uint64_t* d_out3, const uint64_t* d_a2, const uint64_t* d_b2, size_t batch,
                            uint32_t flags, void* stream) {
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_ct_mul", "null context");
    if (flags & ~(DPFHE_IN_NTT | DPFHE_OUT_NTT)) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_ct_mul", "unknown flag");
    if (batch == 0) return DPFHE_SUCCESS;
    if (!d_out3 || !d_a2 || !d_b2 || misaligned(d_out3) || misaligned(d_a2) || misaligned(d_b2))
        return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_ct_mul", "null or misaligned buffer");
    if (ct_mul_output_overlaps(c, d_out3, d_a2, d_b2, batch)) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_ct_mul", "output overlaps an operand");
    const size_t blocks = batch * c->n_limbs;
    if (blocks > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_ct_mul", "batch too large for one launch");
    DPFHE_ON_DEVICE(c, "dpfhe_ct_mul");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (c->log2n > kMaxFusedLog2N) return ct_mul_composed(c, d_out3, d_a2, d_b2, batch, flags, s);
    if (flags == 0 && c->fold) {   // coefficient domain in and out: the form chosen for this box (bit-identical results)
        const int v = c->ct_mul_variant.load(std::memory_order_relaxed);
        if (v != ct_mul_default_variant((int)c->log2n) && ct_mul_variant_compiled(c, v)) {
            if (launch_ct_mul_variant<FoldArith>((int)c->log2n, v, d_out3, d_a2, d_b2, blocks, c->foldt, s)) return fail(DPFHE_INVALID_STATE, "dpfhe_ct_mul", "variant not compiled");
            return check_launch("ct_mul kernel launch");
        }
    }
    int rc;
    if (c->classes) {   // one launch per arithmetic class of the limbs (dpfhe_ctx::classes)
        const size_t pairs = blocks / c->n_limbs;
        rc = for_each_class(c, c->n_limbs, [&](const auto& tb) { return launch_ct_mul((int)c->log2n, flags, d_out3, d_a2, d_b2, pairs * (size_t)tb.n_active, tb, s); });
    } else {
        rc = with_ctx_arith(c, [&](auto arith) { return launch_ct_mul((int)c->log2n, flags, d_out3, d_a2, d_b2, blocks, tables_of<decltype(arith)>(c), s); });
    }
    if (rc) return fail(DPFHE_INVALID_STATE, "dpfhe_ct_mul", "no kernel geometry for this log2_n");
    return check_launch("ct_mul kernel launch");
}

// diagnostics: the quad form with per-workgroup timestamps (kernels.h ct_mul_quad_kernel<..., TRACE>); FoldArith contexts at N = 4096
extern "C" int dpfhe_debug_ct_mul_trace(dpfhe_ctx* c, uint64_t* d_out3, const uint64_t* d_a2, const uint64_t* d_b2, size_t batch, uint64_t* d_trace, void* stream) {
    if (!c || !d_out3 || !d_a2 || !d_b2 || !d_trace) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_debug_ct_mul_trace", "null argument");
    if (!c->fold || c->log2n != 12) return fail(DPFHE_INVALID_STATE, "dpfhe_debug_ct_mul_trace", "FoldArith contexts at N = 4096 only");
    const size_t blocks = batch * c->n_limbs;
    if (batch == 0 || blocks > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_debug_ct_mul_trace", "bad batch");
    if (ct_mul_output_overlaps(c, d_out3, d_a2, d_b2, batch)) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_debug_ct_mul_trace", "output overlaps an operand");
    DPFHE_ON_DEVICE(c, "dpfhe_debug_ct_mul_trace");
    if (launch_ct_mul_trace<FoldArith>((int)c->log2n, d_out3, d_a2, d_b2, blocks, c->foldt, d_trace, static_cast<hipStream_t>(stream)))
        return fail(DPFHE_INVALID_STATE, "dpfhe_debug_ct_mul_trace", "not compiled");
    return check_launch("traced ct_mul kernel launch");
}

// RNS-digit key switching behind dpfhe_relinearize (in_comps = 3: c2 is switched, c0 and c1 added back) and dpfhe_switch_key (in_comps = 2: c1 is
// switched, c0 added back).  The two entries report a bad buffer in their own words.
static int key_switch_entry(dpfhe_ctx* c, const char* what, int in_comps, uint64_t* d_out2, const uint64_t* d_in, const uint64_t* d_key, size_t batch, void* stream) {
    const bool relin = in_comps == 3;
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    if (batch == 0) return DPFHE_SUCCESS;
    const size_t poly = (size_t)c->n_limbs << c->log2n;
    const bool bad = !d_out2 || !d_in || !d_key || misaligned(d_out2) || misaligned(d_in) || misaligned(d_key);
    // input items are in_comps L N words apart, output items 2 L N: any overlap lets one workgroup overwrite another's unread input
    const bool aliased = overlaps(d_out2, batch * 2 * poly, d_in, batch * (size_t)in_comps * poly);
    if (relin) {
        if (bad) return fail(DPFHE_INVALID_ARGUMENT, what, "null or misaligned buffer");
        if (aliased) return fail(DPFHE_INVALID_ARGUMENT, what, "output overlaps the input");
    } else if (bad || aliased) {
        return fail(DPFHE_INVALID_ARGUMENT, what, "null, misaligned or aliased buffer");
    }
    const size_t blocks = batch * c->n_limbs;
    if (blocks > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    DPFHE_ON_DEVICE(c, what);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (c->log2n > kMaxFusedLog2N) return key_switch_composed(c, d_out2, d_in, in_comps, relin ? 3 : 1, d_key, batch, s, what);
    const int rc = relin_launch(c, relin ? 0 : 1, d_out2, d_in, d_key, 0, 1, blocks, s);
    if (rc) return fail(DPFHE_INVALID_STATE, what, "no kernel geometry for this log2_n");
    return check_launch(relin ? "relin kernel launch" : "switch_key kernel launch");
}

extern "C" int dpfhe_relinearize(dpfhe_ctx* c, uint64_t* d_out2, const uint64_t* d_in3, const uint64_t* d_evk, size_t batch, void* stream) {
    return key_switch_entry(c, "dpfhe_relinearize", 3, d_out2, d_in3, d_evk, batch, stream);
}
extern "C" int dpfhe_switch_key(dpfhe_ctx* c, uint64_t* d_out2, const uint64_t* d_in2, const uint64_t* d_key, size_t batch, void* stream) {
    return key_switch_entry(c, "dpfhe_switch_key", 2, d_out2, d_in2, d_key, batch, stream);
}

// rescale_kernel over `blocks` (polynomial, kept limb, 512-word chunk) workgroups; `add` (add_comps components per item, null: none) as add_mask selects
static void launch_rescale(const dpfhe_ctx* c, size_t blocks, hipStream_t s, u64* out, const u64* in, const u64* add, int add_comps, int add_mask) {
    const int n = 1 << c->log2n, chunks = chunks_of(n);
    with_ctx_arith(c, [&](auto arith) {
        hipLaunchKernelGGL((rescale_kernel<decltype(arith)>), dim3((unsigned)blocks), dim3(256), 0, s, out, in, add, add_comps, add_mask, c->lc, c->d_rescale, (int)c->n_limbs, n, chunks);
    });
}

extern "C" int dpfhe_rescale(dpfhe_ctx* c, uint64_t* d_out, const uint64_t* d_in, size_t n_rns_polys, void* stream) {
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_rescale", "null context");
    if (c->n_limbs < 2) return fail(DPFHE_INVALID_STATE, "dpfhe_rescale", "no limb left to drop");
    if (n_rns_polys == 0) return DPFHE_SUCCESS;
    if (!d_out || !d_in || misaligned(d_out) || misaligned(d_in)) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_rescale", "null or misaligned buffer");
    const int n = 1 << c->log2n;
    const int chunks = chunks_of(n);
    const size_t blocks = n_rns_polys * (c->n_limbs - 1) * (size_t)chunks;
    if (blocks > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_rescale", "batch too large for one launch");
    DPFHE_ON_DEVICE(c, "dpfhe_rescale");
    hipStream_t s = static_cast<hipStream_t>(stream);
    launch_rescale(c, blocks, s, d_out, d_in, nullptr, 0, 0);
    return check_launch("rescale kernel launch");
}

// lift_digits_kernel over `grid` (digit, limb, chunk) workgroups: the Ld digits of the component at `comp` (items `item_stride` words apart) into `digits`
static void launch_lift_digits(const dpfhe_ctx* c, size_t grid, hipStream_t s, u64* digits, const u64* comp, size_t item_stride, int chunks) {
    with_ctx_arith(c, [&](auto arith) {
        hipLaunchKernelGGL((lift_digits_kernel<decltype(arith)>), dim3((unsigned)grid), dim3(256), 0, s, digits, comp, item_stride, c->lc, (int)c->n_limbs, 1 << c->log2n, chunks);
    });
}

// Above N = 8192 (no fused key-switch kernel): out[item][2][L][N] (NTT domain over Q P) = sum_j NTT(lift(digit_j of item)) (.) key_j, the digits being the Ld
// limbs of one component (`comp0`: component pointer of item 0, items `item_stride` words apart), keys per item group (key_stride / key_group as in
// launch_relin; 0 / 1 = one key).  Composed from lift_digits_kernel, the batched forward transform and key_inner_product_kernel; scratch from the
// context's pool, batch sliced so that a slice's Ld L N words per item stay below the scratch limit.
static int key_products_composed(dpfhe_ctx* c, uint64_t* d_out_qp, const uint64_t* comp0, size_t item_stride, const uint64_t* d_keys, size_t key_stride, unsigned key_group,
                                 size_t batch, hipStream_t s, const char* what) {
    const size_t L = c->n_limbs, Ld = L - 1;
    const int n = 1 << c->log2n, ch = chunks_of(n);
    const size_t per = slice_items(c, batch, Ld * L * (size_t)n);
    return for_slices(batch, per, [&](size_t i0, size_t m) -> int {
        const size_t lift_grid = m * Ld * L * (size_t)ch;
        if (lift_grid > kMaxGrid || !ntt_grid_fits(c, m * Ld * L)) return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch (lower the scratch limit)");
        StreamScratch ws(c, s);
        if (int rc = ws.alloc(m * Ld * L * n, what)) return rc;
        const u64* comp = comp0 + i0 * item_stride;
        launch_lift_digits(c, lift_grid, s, ws.p, comp, item_stride, ch);
        if (int rc = check_launch("digit lift kernel launch")) return rc;
        if (int rc = ntt_launch(c, false, ws.p, ws.p, m * Ld * L, s)) return rc;
        const unsigned grid = (unsigned)(m * L * (size_t)ch);
        u64* o = d_out_qp + i0 * 2 * L * n;
        with_ctx_arith(c, [&](auto arith) {
            hipLaunchKernelGGL((key_inner_product_kernel<decltype(arith)>), dim3(grid), dim3(256), 0, s, o, ws.p, d_keys, c->lc, (int)Ld, (int)L, n, ch, key_stride, key_group, (unsigned)i0);
        });
        return check_launch("key inner product kernel launch");
    });
}

// hybrid key switching = inner product over all L limbs (relin_kernel MODE 2/3) + divide by the special prime and add (c0, c1);
// drop_last (relinearisation only): the last pass also divides by the last data prime, d_out2 is [batch][2][Ld-1][N] (relin_rescale_kernel)
static int hybrid_entry(dpfhe_ctx* c, const char* what, int in_comps, uint64_t* d_out2, const uint64_t* d_in, const uint64_t* d_key,
                        uint64_t* d_work, size_t batch, void* stream, size_t key_stride = 0, unsigned key_group = 1, bool drop_last = false) {
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    if (int rc = check_extended(c, what)) return rc;
    if (drop_last && c->n_limbs < 3) return fail(DPFHE_INVALID_STATE, what, "no data limb left to drop (Ld < 2)");
    if (batch == 0) return DPFHE_SUCCESS;
    if (!d_out2 || !d_in || !d_key || !d_work || misaligned(d_out2) || misaligned(d_in) || misaligned(d_key) || misaligned(d_work))
        return fail(DPFHE_INVALID_ARGUMENT, what, "null or misaligned buffer");
    const size_t L = c->n_limbs, Ld = L - 1;
    const int n = 1 << c->log2n;
    {   // the rescale-add pass reads (c0, c1) of the input while it writes the output; the work buffer is written by pass 1
        const size_t in_words = batch * (size_t)in_comps * Ld * n, out_words = batch * 2 * (drop_last ? Ld - 1 : Ld) * n, work_words = batch * 2 * L * n;
        if (overlaps(d_out2, out_words, d_in, in_words) || overlaps(d_work, work_words, d_in, in_words) || overlaps(d_work, work_words, d_out2, out_words))
            return fail(DPFHE_INVALID_ARGUMENT, what, "output, input and work buffers must not overlap");
    }
    const size_t blocks = batch * L;
    // the grouped and key-major launches pad the grid to whole XCD rounds: the launcher's own plan (a launch per limb class is no larger)
    const size_t kg = key_group ? key_group : 1;
    if (blocks > kMaxGrid || RelinMap::plan(blocks, (unsigned)L, key_stride, key_group).grid > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    DPFHE_ON_DEVICE(c, "hybrid key switch");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int mode = in_comps == 3 ? 2 : 3;
    if (c->log2n > kMaxFusedLog2N) {
        // no fused kernel: digits lifted to Q P -> one batched transform -> inner products with the key(s) -> batched inverse into `work`;
        // in slices whose scratch (Ld L N words per item) stays below the context's limit
        if (int rc = key_products_composed(c, d_work, d_in + (size_t)(in_comps - 1) * Ld * n, (size_t)in_comps * Ld * n, d_key, key_stride, (unsigned)kg, batch, s, what)) return rc;
        if (!ntt_grid_fits(c, batch * 2 * L)) return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
        if (int rc = ntt_launch(c, true, d_work, d_work, batch * 2 * L, s)) return rc;
    } else {
        const int rc = relin_launch(c, mode, d_work, d_in, d_key, key_stride, key_group, blocks, s);
        if (rc) return fail(DPFHE_INVALID_STATE, what, "no kernel geometry for this log2_n");
        int e = check_launch("hybrid key-switch kernel launch");
        if (e) return e;
    }
    // divide by P with rounding and add c0 (and c1 for relinearisation): one pass over the 2*batch polynomials of `work`
    const int chunks = chunks_of(n);
    const size_t rblocks = batch * 2 * Ld * (size_t)chunks;
    if (rblocks > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    if (drop_last) {   // ... and by the last data prime in the same pass
        with_ctx_arith(c, [&](auto arith) {
            hipLaunchKernelGGL((relin_rescale_kernel<decltype(arith)>), dim3((unsigned)(batch * 2 * (Ld - 1) * (size_t)chunks)), dim3(256), 0, s, d_out2, d_work, d_in, c->lc,
                               c->d_rescale, c->d_rescale2, (int)L, n, chunks);
        });
        return check_launch("hybrid rescale-twice launch");
    }
    launch_rescale(c, rblocks, s, d_out2, d_work, d_in, in_comps, in_comps == 3 ? 3 : 1);
    return check_launch("hybrid rescale launch");
}

extern "C" int dpfhe_relinearize_hybrid(dpfhe_ctx* c, uint64_t* d_out2, const uint64_t* d_in3, const uint64_t* d_key, uint64_t* d_work, size_t batch,
                                        void* stream) {
    return hybrid_entry(c, "dpfhe_relinearize_hybrid", 3, d_out2, d_in3, d_key, d_work, batch, stream);
}
extern "C" int dpfhe_switch_key_hybrid(dpfhe_ctx* c, uint64_t* d_out2, const uint64_t* d_in2, const uint64_t* d_key, uint64_t* d_work, size_t batch,
                                       void* stream) {
    return hybrid_entry(c, "dpfhe_switch_key_hybrid", 2, d_out2, d_in2, d_key, d_work, batch, stream);
}
extern "C" int dpfhe_relinearize_rescale_hybrid(dpfhe_ctx* c, uint64_t* d_out2, const uint64_t* d_in3, const uint64_t* d_key, uint64_t* d_work, size_t batch,
                                                void* stream) {
    return hybrid_entry(c, "dpfhe_relinearize_rescale_hybrid", 3, d_out2, d_in3, d_key, d_work, batch, stream, 0, 1, true);
}

// automorphism launch: polynomials up to 64 KiB are staged through LDS, larger ones gathered from global memory
static void launch_galois_multi(hipStream_t s, unsigned grid, u64* out, const u64* in, size_t in_item_stride, const LimbConst* lc, int n_limbs, int n,
                                int polys_per_item, const GaloisInvs& inv, unsigned in_mod, unsigned item0) {
    if (n <= 8192)
        hipLaunchKernelGGL(galois_multi_kernel<true>, dim3(grid), dim3(256), (size_t)n * 8, s, out, in, in_item_stride, lc, n_limbs, n, polys_per_item, inv, in_mod, item0);
    else
        hipLaunchKernelGGL(galois_multi_kernel<false>, dim3(grid), dim3(256), 0, s, out, in, in_item_stride, lc, n_limbs, n, polys_per_item, inv, in_mod, item0);
}

static unsigned galois_inverse(unsigned g, unsigned two_n) {  // g^-1 mod 2N by Newton iteration (g odd): x <- x (2 - g x)
    unsigned inv = 1;
    for (int i = 0; i < 5; ++i) inv *= 2u - g * inv;
    return inv & (two_n - 1u);
}

// N3: `batch` rotations in one pass - item i = key-switched sigma_{g_(i / group)}(input item i, or the single input when n_in == 1);
// `group` consecutive items share an element and its key (several tokens, rotation-major order)
static int rotate_batch_impl(dpfhe_ctx* c, const char* what, uint64_t* d_out2, const uint64_t* d_in2, size_t n_in, const uint32_t* galois_elts, size_t n_elts,
                             size_t group, const uint64_t* d_keys, uint64_t* d_work, uint64_t* d_rotated, size_t batch, void* stream) {
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    if (int rc = check_extended(c, what)) return rc;
    if (batch == 0) return DPFHE_SUCCESS;
    if (n_in != 1 && n_in != batch) return fail(DPFHE_INVALID_ARGUMENT, what, "n_in must be 1 (one input, many rotations) or equal to batch");
    if (group == 0 || n_elts * group != batch) return fail(DPFHE_INVALID_ARGUMENT, what, "batch must be n_elts * group");
    if (!d_out2 || !d_in2 || !galois_elts || !d_keys || !d_work || !d_rotated || misaligned(d_out2) || misaligned(d_in2) || misaligned(d_keys) ||
        misaligned(d_work) || misaligned(d_rotated) || d_rotated == d_in2)
        return fail(DPFHE_INVALID_ARGUMENT, what, "null, misaligned or aliased buffer");
    const size_t L = c->n_limbs, Ld = L - 1;
    const int n = 1 << c->log2n;
    const unsigned two_n = 2u << c->log2n;
    if (int rc = check_galois_elts(c, galois_elts, n_elts, what)) return rc;
    const size_t ct_words = 2 * Ld * (size_t)n, key_words = Ld * 2 * L * (size_t)n;
    if (n_in == batch && overlaps(d_rotated, batch * ct_words, d_in2, batch * ct_words)) return fail(DPFHE_INVALID_ARGUMENT, what, "d_rotated overlaps the input");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DPFHE_ON_DEVICE(c, what);
    const int rc = for_slices(batch, kMaxGaloisBatch, [&](size_t first, size_t cnt) {   // the elements travel as kernel arguments, 64 at a time
        GaloisInvs inv{};
        for (size_t i = 0; i < cnt; ++i) inv.v[i] = galois_inverse(galois_elts[(first + i) / group], two_n);
        const uint64_t* src = d_in2 + (n_in == 1 ? 0 : first * ct_words);
        launch_galois_multi(s, (unsigned)(cnt * 2 * Ld), d_rotated + first * ct_words, src, n_in == 1 ? (size_t)0 : ct_words, c->lc, (int)Ld, n, (int)(2 * Ld), inv, 0u, 0u);
        return check_launch("galois kernel launch");
    });
    if (rc) return rc;
    return hybrid_entry(c, what, 2, d_out2, d_rotated, d_keys, d_work, batch, stream, key_words, (unsigned)group);
}

extern "C" int dpfhe_rotate_hybrid_batch(dpfhe_ctx* c, uint64_t* d_out2, const uint64_t* d_in2, size_t n_in, const uint32_t* galois_elts,
                                         const uint64_t* d_keys, uint64_t* d_work, uint64_t* d_rotated, size_t batch, void* stream) {
    return rotate_batch_impl(c, "dpfhe_rotate_hybrid_batch", d_out2, d_in2, n_in, galois_elts, batch, 1, d_keys, d_work, d_rotated, batch, stream);
}

extern "C" int dpfhe_rotate_hybrid_grouped(dpfhe_ctx* c, uint64_t* d_out2, const uint64_t* d_in2, const uint32_t* galois_elts, size_t n_elts, size_t group,
                                           const uint64_t* d_keys, uint64_t* d_work, uint64_t* d_rotated, void* stream) {
    return rotate_batch_impl(c, "dpfhe_rotate_hybrid_grouped", d_out2, d_in2, n_elts * group, galois_elts, n_elts, group, d_keys, d_work, d_rotated, n_elts * group, stream);
}

// ------------------------------------------------------------------------------------------------
// N3, round 3: baby-step / giant-step sums with the division by P DEFERRED (the rotated terms stay in the NTT domain over Q P)
// ------------------------------------------------------------------------------------------------
// (prepared = true: d_in_ntt, d_digits and item block 0 already hold what steps 1-3 write - a later slice of dpfhe_rotate_hybrid_hoisted at N >= 16384)
// Every ring degree: the stream kernels take log2 N at run time (32-bit segment arithmetic modulo 2N <= 2^17), the transforms are ntt_launch_items'.
static int rotate_hoisted_qp_impl(dpfhe_ctx* c, uint64_t* d_out_qp, const uint64_t* d_in2, size_t n_items, const uint32_t* galois_elts, const uint64_t* d_keys,
                                  uint64_t* d_in_ntt, uint64_t* d_digits, size_t batch, void* stream, bool prepared) {
    const char* what = "dpfhe_rotate_hoisted_qp";
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    if (int rc = check_extended(c, what)) return rc;
    if (n_items == 0) return DPFHE_SUCCESS;
    if (!d_out_qp || !d_in2 || (batch && (!galois_elts || !d_keys)) || !d_in_ntt || !d_digits || misaligned(d_out_qp) || misaligned(d_in2) || misaligned(d_keys) ||
        misaligned(d_in_ntt) || misaligned(d_digits))
        return fail(DPFHE_INVALID_ARGUMENT, what, "null or misaligned buffer");
    const size_t L = c->n_limbs, Ld = L - 1, T = n_items;
    const int n = 1 << c->log2n;
    if (int rc = check_galois_elts(c, galois_elts, batch, what)) return rc;
    const size_t in_words = T * 2 * Ld * (size_t)n, out_words = (batch + 1) * T * 2 * L * n, dig_words = T * Ld * L * (size_t)n;
    if (overlaps(d_out_qp, out_words, d_in2, in_words) || overlaps(d_out_qp, out_words, d_in_ntt, in_words) || overlaps(d_out_qp, out_words, d_digits, dig_words) ||
        overlaps(d_digits, dig_words, d_in2, in_words) || overlaps(d_digits, dig_words, d_in_ntt, in_words) || overlaps(d_in_ntt, in_words, d_in2, in_words))
        return fail(DPFHE_INVALID_ARGUMENT, what, "buffers must not overlap");
    const size_t key_words = Ld * 2 * L * (size_t)n;
    const int chunks = chunks_of(n);
    if ((batch + 1) * T * L * 8 > kMaxGrid || T * Ld * L * (size_t)chunks > kMaxGrid || T * 2 * L * (size_t)chunks > kMaxGrid || !ntt_grid_fits(c, T * Ld * L))
        return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    const u64 p_special = c->p_special;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DPFHE_ON_DEVICE(c, what);
    if (!prepared) {
        // 1. NTT of the inputs on the data limbs (the same tables, seen as an Ld-limb context)
        if (int e = ntt_launch_items(c, false, d_in_ntt, d_in2, T * 2, Ld, s)) return e;
        // 2. digits of every item's c1, lifted to every limb and transformed
        launch_lift_digits(c, T * Ld * L * (size_t)chunks, s, d_digits, d_in2 + Ld * (size_t)n, 2 * Ld * (size_t)n, chunks);
        if (int e = check_launch("lift_digits kernel launch")) return e;
        if (int e = ntt_launch_items(c, false, d_digits, d_digits, T * Ld, 0, s)) return e;   // (per limb class where the context has them)
        // 3. item block 0: the inputs themselves as P * ct over the extended basis
        const unsigned idg = (unsigned)(T * 2 * L * (size_t)chunks);
        with_ctx_arith(c, [&](auto arith) { hipLaunchKernelGGL((lift_qp_kernel<decltype(arith)>), dim3(idg), dim3(256), 0, s, d_out_qp, d_in_ntt, c->lc, p_special, (int)L, n, chunks); });
        if (int e = check_launch("lift_qp kernel launch")) return e;
    }
    // 4. the rotations: permuted digit segments x key segments as a stream (kernels_misc.h hoisted_qp_stream_kernel), 64 rotations per launch
    return for_slices(batch, kMaxGaloisBatch, [&](size_t first, size_t cnt) -> int {
        uint64_t* dst = d_out_qp + (1 + first) * T * 2 * L * n;
        {
            QpElts ge{};
            for (size_t i = 0; i < cnt; ++i) ge.v[i] = galois_elts[first + i];
            // (pairs per thread: 2 measured best at 8 tokens - 291 us against 300 with 1 and 329 with 4 -, 1 is 5 % ahead at one token: profiles/r04_ab_baby_steps.txt)
            if (c->fold && Ld >= 1 && Ld <= 6) {   // every segment of the workgroup requested up front (one pair of words per thread)
                const size_t grid1 = QpMap::grid((int)c->log2n, (int)L, cnt, T, 1);
                if (grid1 > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
#define QPU(LD) case LD: hipLaunchKernelGGL((hoisted_qp_upfront_kernel<LD>), dim3((unsigned)grid1), dim3(256), 0, s, dst, d_digits, d_in_ntt, d_keys + first * key_words, key_words, ge, \
                                            (unsigned)cnt, (unsigned)T, p_special, c->lc, (int)c->log2n); break
                switch (Ld) { QPU(1); QPU(2); QPU(3); QPU(4); QPU(5); QPU(6); }
#undef QPU
                return check_launch("hoisted_qp kernel launch");
            }
            const size_t grid = QpMap::grid((int)c->log2n, (int)L, cnt, T);
            if (grid > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
            with_ctx_arith(c, [&](auto arith) {
                hipLaunchKernelGGL((hoisted_qp_stream_kernel<decltype(arith), kQpPairs>), dim3((unsigned)grid), dim3(256), 0, s, dst, d_digits, d_in_ntt, d_keys + first * key_words, key_words, ge,
                                   (unsigned)cnt, (unsigned)T, p_special, c->lc, (int)L, (int)c->log2n);
            });
        }
        return check_launch("hoisted_qp kernel launch");
    });
}

extern "C" int dpfhe_rotate_hoisted_qp(dpfhe_ctx* c, uint64_t* d_out_qp, const uint64_t* d_in2, size_t n_items, const uint32_t* galois_elts, const uint64_t* d_keys,
                                       uint64_t* d_in_ntt, uint64_t* d_digits, size_t batch, void* stream) {
    return rotate_hoisted_qp_impl(c, d_out_qp, d_in2, n_items, galois_elts, d_keys, d_in_ntt, d_digits, batch, stream, false);
}

// N3, hoisted: `batch` rotations of ONE ciphertext; the digit decomposition of c1 and its Ld*L forward transforms are done once
// (d_digits), every rotation is a permutation of those words in the NTT domain + its key inner product + two inverse transforms
extern "C" int dpfhe_rotate_hybrid_hoisted(dpfhe_ctx* c, uint64_t* d_out2, const uint64_t* d_in2, size_t n_items, const uint32_t* galois_elts, const uint64_t* d_keys,
                                           uint64_t* d_work, uint64_t* d_rotated0, uint64_t* d_digits, size_t batch, void* stream) {
    const char* what = "dpfhe_rotate_hybrid_hoisted";
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    if (int rc = check_extended(c, what)) return rc;
    if (batch == 0 || n_items == 0) return DPFHE_SUCCESS;
    const bool composed = c->log2n > kMaxFusedLog2N;   // N >= 16384: the deferred-division pipeline below never touches d_work / d_rotated0 - they may be NULL
    if (!d_out2 || !d_in2 || !galois_elts || !d_keys || (!composed && (!d_work || !d_rotated0)) || !d_digits || misaligned(d_out2) || misaligned(d_in2) || misaligned(d_keys) ||
        misaligned(d_work) || misaligned(d_rotated0) || misaligned(d_digits))
        return fail(DPFHE_INVALID_ARGUMENT, what, "null or misaligned buffer");
    const size_t L = c->n_limbs, Ld = L - 1, T = n_items, total = batch * T;
    const int n = 1 << c->log2n;
    const unsigned two_n = 2u << c->log2n;
    if (int rc = check_galois_elts(c, galois_elts, batch, what)) return rc;
    const size_t in_words = T * 2 * Ld * (size_t)n, out_words = total * 2 * Ld * n, work_words = d_work ? total * 2 * L * n : 0, rot_words = d_rotated0 ? total * Ld * n : 0,
                 dig_words = T * Ld * L * (size_t)n;
    if (overlaps(d_out2, out_words, d_in2, in_words) || overlaps(d_out2, out_words, d_work, work_words) || overlaps(d_out2, out_words, d_rotated0, rot_words) ||
        overlaps(d_work, work_words, d_rotated0, rot_words) || overlaps(d_digits, dig_words, d_work, work_words) || overlaps(d_digits, dig_words, d_out2, out_words) ||
        overlaps(d_digits, dig_words, d_rotated0, rot_words) || overlaps(d_digits, dig_words, d_in2, in_words) || overlaps(d_rotated0, rot_words, d_in2, in_words))
        return fail(DPFHE_INVALID_ARGUMENT, what, "buffers must not overlap");
    const size_t key_words = Ld * 2 * L * (size_t)n;
    const int chunks = chunks_of(n);
    if (composed) {
        DPFHE_ON_DEVICE(c, what);
        // N >= 16384 (round 5; N = 32768, 65536 on the split transforms): no fused hoisted kernel - the deferred-division pipeline instead: dpfhe_rotate_hoisted_qp gives, per rotation and item,
        // P sigma_g(ct) + its key-switching term in the NTT domain over Q P; one inverse transform and the division by P per term finish it (the same words:
        // tests/test_rlwe_semantics.py).  Scratch (the Q P terms + the transformed inputs) from the stream's arena, rotations in slices under the scratch limit;
        // d_work / d_rotated0 are not used on this path.
        const size_t item_qp = T * 2 * L * (size_t)n, fit = c->scratch_limit_words.load(std::memory_order_relaxed) / item_qp;
        const size_t per = fit > 2 ? (fit - 2 < batch ? fit - 2 : batch) : 1;     // (+ block 0 and the transformed inputs)
        if (per * T * 2 * Ld * (size_t)chunks > kMaxGrid || !ntt_grid_fits(c, per * T * 2 * L)) return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch (lower the scratch limit)");
        StreamScratch ws(c, static_cast<hipStream_t>(stream));       // one arena for every slice: the transformed inputs and digits are prepared by the first slice only
        if (int rc = ws.alloc((per + 1) * item_qp + in_words, what)) return rc;
        u64* qp = ws.p;
        u64* in_ntt = qp + (per + 1) * item_qp;
        return for_slices(batch, per, [&](size_t r0, size_t m) -> int {
            if (int rc = rotate_hoisted_qp_impl(c, qp, d_in2, T, galois_elts + r0, d_keys + r0 * key_words, in_ntt, d_digits, m, stream, r0 != 0)) return rc;
            hipStream_t s = static_cast<hipStream_t>(stream);
            if (int rc = ntt_launch(c, true, qp + item_qp, qp + item_qp, m * T * 2 * L, s)) return rc;
            launch_rescale(c, m * T * 2 * Ld * (size_t)chunks, s, d_out2 + r0 * T * 2 * Ld * n, qp + item_qp, nullptr, 0, 0);
            return check_launch("hoisted rescale launch");
        });
    }
    // (the key-switch launch pads its (rotation, limb[, component]) tiles to a multiple of 8 per token: launch_impl.h launch_hoisted_ks)
    if (total * 2 * Ld * (size_t)chunks > kMaxGrid || (total * L * 2 + 8 * T) > kMaxGrid || T * Ld * L * (size_t)chunks > kMaxGrid)
        return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DPFHE_ON_DEVICE(c, what);
    // 1. digits of every item's c1, lifted to every limb, then transformed (T * Ld RNS polynomials on the extended context)
    launch_lift_digits(c, T * Ld * L * (size_t)chunks, s, d_digits, d_in2 + Ld * (size_t)n, 2 * Ld * (size_t)n, chunks);
    if (int e = check_launch("lift_digits kernel launch")) return e;
    if (int e = ntt_launch_items(c, false, d_digits, d_digits, T * Ld, 0, s)) return e;   // (per limb class where the context has them)
    // 2. sigma_g(c0) of every (rotation, item) for the final addition: [batch][T][Ld][N]; 64 output items per launch
    if (int e = for_slices(total, kMaxGaloisBatch, [&](size_t first, size_t cnt) {
        GaloisInvs inv{};
        for (size_t i = 0; i < cnt; ++i) inv.v[i] = galois_inverse(galois_elts[(first + i) / T], two_n);
        launch_galois_multi(s, (unsigned)(cnt * Ld), d_rotated0 + first * Ld * n, d_in2, 2 * Ld * (size_t)n, c->lc, (int)Ld, n, (int)Ld, inv, (unsigned)T, (unsigned)(first % T));
        return check_launch("galois kernel launch");
    })) return e;
    // 3. permuted digits (.) keys, one inverse transform per (rotation, limb, key component, item); 64 rotations per launch
    if (int e = for_slices(batch, kMaxGaloisBatch, [&](size_t first, size_t cnt) -> int {
        const int rc = with_policy_or_classes(c, [&](const auto& tb) {
            return launch_hoisted_ks((int)c->log2n, d_work + first * T * 2 * L * n, d_digits, d_keys + first * key_words, key_words, galois_elts + first, cnt, T, tb, s);
        });
        if (rc) return fail(DPFHE_INVALID_STATE, what, "no kernel geometry for this log2_n");
        return check_launch("hoisted key-switch kernel launch");
    })) return e;
    // 4. divide by P with rounding; component 0 gets sigma_g(c0) added ([total][1][Ld][N] addend)
    launch_rescale(c, total * 2 * Ld * (size_t)chunks, s, d_out2, d_work, d_rotated0, 1, 1);
    return check_launch("hoisted rescale launch");
}

extern "C" int dpfhe_ntt_inv_galois(dpfhe_ctx* c, uint64_t* d_out, const uint64_t* d_in, size_t rns_polys_per_elt, const uint32_t* galois_elts, size_t n_elts, void* stream) {
    const char* what = "dpfhe_ntt_inv_galois";
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    if (n_elts == 0 || rns_polys_per_elt == 0) return DPFHE_SUCCESS;
    if (!d_out || !d_in || !galois_elts || misaligned(d_out) || misaligned(d_in)) return fail(DPFHE_INVALID_ARGUMENT, what, "null or misaligned buffer");
    if (int rc = check_galois_elts(c, galois_elts, n_elts, what)) return rc;
    const size_t per_elt = rns_polys_per_elt * c->n_limbs, words = n_elts * per_elt << c->log2n;
    if (d_out != d_in && overlaps(d_out, words, d_in, words)) return fail(DPFHE_INVALID_ARGUMENT, what, "output must be the input buffer or disjoint from it");
    const bool split = split_log_n1((int)c->log2n) != 0;
    // N > 16384: the sub-transforms of block b read block b' (ntt_core.h galois_sub_block) - in place, their output is staged in the stream's arena, elements in
    // slices under the scratch limit (each slice: in -> scratch -> out, the same 4 N words of traffic per polynomial as the plain split inverse)
    const size_t group = split && d_out == d_in ? slice_items(c, n_elts < (size_t)kMaxGaloisBatch ? n_elts : (size_t)kMaxGaloisBatch, per_elt << c->log2n) : (size_t)kMaxGaloisBatch;
    if (!ntt_grid_fits(c, per_elt * (n_elts < group ? n_elts : group))) return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    DPFHE_ON_DEVICE(c, what);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (split) {
        StreamScratch ws(c, s);
        if (d_out == d_in) if (int rc = ws.alloc((n_elts < group ? n_elts : group) * per_elt << c->log2n, what)) return rc;
        return for_slices(n_elts, group, [&](size_t first, size_t cnt) -> int {
            const size_t off = first * per_elt << c->log2n;
            u64* mid = d_out == d_in ? ws.p : d_out + off;
            const int rc = c->fold ? launch_ntt_inv_galois_split((int)c->log2n, d_out + off, mid, d_in + off, galois_elts + first, cnt, per_elt, c->foldt, s)
                                   : launch_ntt_inv_galois_split((int)c->log2n, d_out + off, mid, d_in + off, galois_elts + first, cnt, per_elt, c->shoup, s);
            if (rc) return fail(DPFHE_INVALID_STATE, what, "no split transform for this context");
            return check_launch("ntt_inv_galois kernel launch");
        });
    }
    return for_slices(n_elts, kMaxGaloisBatch, [&](size_t first, size_t cnt) -> int {
        const size_t off = first * per_elt << c->log2n;
        const int rc = with_policy_or_classes(c, [&](const auto& tb) { return launch_ntt_inv_galois((int)c->log2n, d_out + off, d_in + off, galois_elts + first, cnt, per_elt, tb, s); });
        if (rc) return fail(DPFHE_INVALID_STATE, what, "no single-kernel transform for this log2_n");
        return check_launch("ntt_inv_galois kernel launch");
    });
}

extern "C" int dpfhe_switch_key_qp(dpfhe_ctx* c, uint64_t* d_out_qp, const uint64_t* d_in2, const uint64_t* d_keys, size_t n_keys, size_t group, void* stream) {
    const char* what = "dpfhe_switch_key_qp";
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    if (int rc = check_extended(c, what)) return rc;
    const size_t batch = n_keys * group;
    if (batch == 0) return DPFHE_SUCCESS;
    if (!d_out_qp || !d_in2 || !d_keys || misaligned(d_out_qp) || misaligned(d_in2) || misaligned(d_keys)) return fail(DPFHE_INVALID_ARGUMENT, what, "null or misaligned buffer");
    const size_t L = c->n_limbs, Ld = L - 1;
    const int n = 1 << c->log2n;
    if (overlaps(d_out_qp, batch * 2 * L * n, d_in2, batch * 2 * Ld * n)) return fail(DPFHE_INVALID_ARGUMENT, what, "output overlaps the input");
    const size_t blocks = batch * L;
    const size_t key_words = Ld * 2 * L * (size_t)n;
    if (blocks > kMaxGrid || RelinMap::plan(blocks, (unsigned)L, key_words, (unsigned)group).grid > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    DPFHE_ON_DEVICE(c, what);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (c->log2n > kMaxFusedLog2N)   // composed from the batched transform (round 5): the digits of c1, lifted and transformed, times the group's key
        return key_products_composed(c, d_out_qp, d_in2 + Ld * (size_t)n, 2 * Ld * (size_t)n, d_keys, key_words, (unsigned)group, batch, s, what);
    const int rc = relin_launch(c, 4, d_out_qp, d_in2, d_keys, key_words, (unsigned)group, blocks, s);
    if (rc) return fail(DPFHE_INVALID_STATE, what, "no kernel geometry for this log2_n");
    return check_launch("switch_key_qp kernel launch");
}

extern "C" int dpfhe_rescale_bsgs(dpfhe_ctx* c, uint64_t* d_out2, const uint64_t* d_in_qp, const uint64_t* d_addends, size_t n_add, size_t batch, void* stream) {
    const char* what = "dpfhe_rescale_bsgs";
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    if (c->n_limbs < 2) return fail(DPFHE_INVALID_STATE, what, "no limb left to drop");
    if (batch == 0) return DPFHE_SUCCESS;
    if (!d_out2 || !d_in_qp || (n_add && !d_addends) || misaligned(d_out2) || misaligned(d_in_qp) || misaligned(d_addends))
        return fail(DPFHE_INVALID_ARGUMENT, what, "null or misaligned buffer");
    const size_t L = c->n_limbs, Ld = L - 1;
    const int n = 1 << c->log2n;
    const int chunks = chunks_of(n);
    if (overlaps(d_out2, batch * 2 * Ld * n, d_in_qp, batch * 2 * L * n) || (n_add && overlaps(d_out2, batch * 2 * Ld * n, d_addends, n_add * batch * 2 * Ld * n)))
        return fail(DPFHE_INVALID_ARGUMENT, what, "output overlaps an input");
    const size_t blocks = batch * 2 * Ld * (size_t)chunks;
    if (blocks > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    DPFHE_ON_DEVICE(c, what);
    hipStream_t s = static_cast<hipStream_t>(stream);
    with_ctx_arith(c, [&](auto arith) {
        hipLaunchKernelGGL((rescale_bsgs_kernel<decltype(arith)>), dim3((unsigned)blocks), dim3(256), 0, s, d_out2, d_in_qp, d_addends, n_add, batch, c->lc, c->d_rescale, (int)L, n, chunks);
    });
    return check_launch("rescale_bsgs kernel launch");
}

extern "C" int dpfhe_apply_galois(dpfhe_ctx* c, uint64_t* d_out, const uint64_t* d_in, size_t n_rns_polys, uint32_t galois_elt, void* stream) {
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_apply_galois", "null context");
    const unsigned two_n = 2u << c->log2n;
    if (!(galois_elt & 1u) || galois_elt >= two_n) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_apply_galois", "galois_elt must be odd and < 2N");
    if (n_rns_polys == 0) return DPFHE_SUCCESS;
    if (!d_out || !d_in || misaligned(d_out) || misaligned(d_in) ||
        overlaps(d_out, n_rns_polys * ((size_t)c->n_limbs << c->log2n), d_in, n_rns_polys * ((size_t)c->n_limbs << c->log2n)))
        return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_apply_galois", "null, misaligned or aliased buffer");
    const size_t npolys = n_rns_polys * c->n_limbs;
    if (npolys > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_apply_galois", "batch too large for one launch");
    DPFHE_ON_DEVICE(c, "dpfhe_apply_galois");
    const unsigned inv = galois_inverse(galois_elt, two_n);
    hipLaunchKernelGGL(galois_kernel, dim3((unsigned)npolys), dim3(256), 0, static_cast<hipStream_t>(stream), d_out, d_in, c->lc, (int)c->n_limbs,
                       1 << c->log2n, inv);
    return check_launch("galois kernel launch");
}

// ------------------------------------------------------------------------------------------------
extern "C" int dpfhe_matvec_plain(dpfhe_ctx* c, uint64_t* d_y, const uint64_t* d_W, const uint64_t* d_x, size_t rows, size_t cols,
                                  void* stream) {
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_matvec_plain", "null context");
    if (rows == 0) return DPFHE_SUCCESS;
    if (cols == 0) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_matvec_plain", "cols must be > 0");
    if (!d_y || !d_W || !d_x || misaligned(d_y) || misaligned(d_W) || misaligned(d_x))
        return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_matvec_plain", "null or misaligned buffer");
    const int n = 1 << c->log2n;
    constexpr int RT = 4;
    DPFHE_ON_DEVICE(c, "dpfhe_matvec_plain");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (c->fold) {   // column accumulators split at bit 30 (kernels_misc.h matvec_fold_kernel): 4 multiply-adds per term
        constexpr int WPT = kMatvecWpt2;
        const int chunks = (n + 256 * WPT - 1) / (256 * WPT);
        const size_t slabs = c->n_limbs * (size_t)chunks, rtiles = (rows + RT - 1) / RT;
        const size_t blocks = MatvecMap::grid(c->n_limbs, chunks, rtiles, 1);
        if (blocks > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_matvec_plain", "too many rows for one launch");
        // a W beyond the 256 MiB Infinity Cache is a read-once stream (every tile goes to exactly one workgroup here): non-temporal loads
        const bool ntw = rows * cols * ((size_t)c->n_limbs << c->log2n) * sizeof(u64) > kInfinityCacheBytes;
        // (the branch-free FULL form of the kernel, which the multi-right-hand-side product takes, measured SLOWER here: 1412 against 1258 us on configs[2] -
        // this launch streams 6 GiB of W from HBM with two right-hand-side polynomials per workgroup and lives on memory-level parallelism, not on issue slots)
        if (ntw) hipLaunchKernelGGL((matvec_fold_kernel<RT, 2, WPT, true>), dim3((unsigned)blocks), dim3(256), 0, s, d_y, d_W, d_x, c->lc, (int)c->n_limbs, n, chunks, rows,
                                    cols, (size_t)2, 1u, (unsigned)(rtiles * slabs));
        else hipLaunchKernelGGL((matvec_fold_kernel<RT, 2, WPT>), dim3((unsigned)blocks), dim3(256), 0, s, d_y, d_W, d_x, c->lc, (int)c->n_limbs, n, chunks, rows, cols,
                                (size_t)2, 1u, (unsigned)(rtiles * slabs));
        return check_launch("matvec kernel launch");
    }
    const int chunks = chunks_of(n);
    const size_t blocks = MatvecMap::grid(c->n_limbs, chunks, (rows + RT - 1) / RT, 1);   // block ids laid out per XCD: kernels_misc.h matvec_kernel
    if (blocks > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_matvec_plain", "too many rows for one launch");
    hipLaunchKernelGGL((matvec_kernel<ShoupArith, RT>), dim3((unsigned)blocks), dim3(256), 0, s, d_y, d_W, d_x, c->lc, (int)c->n_limbs, n, chunks, rows, cols);
    return check_launch("matvec kernel launch");
}

// One launch of the multi-right-hand-side product: `groups` groups of C / 2 right-hand sides (x / y at xs / ys, the full [n_rhs][2] stride), RT rows and
// 256 WPT words per workgroup, block ids laid out per XCD (kernels_misc.h).  FOLD: matvec_fold_kernel's split-at-bit-30 column accumulators; otherwise
// the generic matvec_multi_kernel (2 words per thread).
template <bool FOLD, int RT, int C, int WPT = 2>
static int matvec_multi_launch(const dpfhe_ctx* c, const char* what, u64* ys, const u64* d_W, const u64* xs, size_t rows, size_t cols, size_t n_rhs, size_t groups,
                               hipStream_t s) {
    const int n = 1 << c->log2n, chunks = (n + 256 * WPT - 1) / (256 * WPT);
    const size_t slabs = c->n_limbs * (size_t)chunks, rtiles = (rows + RT - 1) / RT, tiles = rtiles * slabs;
    const size_t blocks = MatvecMap::grid(c->n_limbs, chunks, rtiles, groups);
    if (blocks > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, what, "too many rows for one launch");
    if constexpr (!FOLD)
        hipLaunchKernelGGL((matvec_multi_kernel<ShoupArith, RT, C>), dim3((unsigned)blocks), dim3(256), 0, s, ys, d_W, xs, c->lc, (int)c->n_limbs, n, chunks, rows, cols,
                           n_rhs * 2, (unsigned)groups, (unsigned)tiles);
    else if (rows % RT == 0 && cols % FoldArith::kDot30Period == 0)   // whole row tiles and whole periods (a packed layer's products): the branch-free form
        hipLaunchKernelGGL((matvec_fold_kernel<RT, C, WPT, false, kMatvecWd, true>), dim3((unsigned)blocks), dim3(256), 0, s, ys, d_W, xs, c->lc, (int)c->n_limbs, n, chunks,
                           rows, cols, n_rhs * 2, (unsigned)groups, (unsigned)tiles);
    else
        hipLaunchKernelGGL((matvec_fold_kernel<RT, C, WPT, false, kMatvecWd>), dim3((unsigned)blocks), dim3(256), 0, s, ys, d_W, xs, c->lc, (int)c->n_limbs, n, chunks,
                           rows, cols, n_rhs * 2, (unsigned)groups, (unsigned)tiles);
    return check_launch("matvec_multi kernel launch");
}

extern "C" int dpfhe_matvec_plain_multi(dpfhe_ctx* c, uint64_t* d_y, const uint64_t* d_W, const uint64_t* d_x, size_t rows, size_t cols, size_t n_rhs,
                                        void* stream) {
    const char* what = "dpfhe_matvec_plain_multi";
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    if (rows == 0 || n_rhs == 0) return DPFHE_SUCCESS;
    if (cols == 0) return fail(DPFHE_INVALID_ARGUMENT, what, "cols must be > 0");
    if (!d_y || !d_W || !d_x || misaligned(d_y) || misaligned(d_W) || misaligned(d_x)) return fail(DPFHE_INVALID_ARGUMENT, what, "null or misaligned buffer");
    if (n_rhs == 1) return dpfhe_matvec_plain(c, d_y, d_W, d_x, rows, cols, stream);
    const size_t poly = (size_t)c->n_limbs << c->log2n;
    hipStream_t s = static_cast<hipStream_t>(stream);
    DPFHE_ON_DEVICE(c, what);
    // 2 right-hand sides x 4 rows per workgroup (32 128-bit accumulators per thread); all groups of 2 in ONE launch whose block ids put
    // the groups of a W tile on the same XCD (kernels_misc.h), an odd last right-hand side in a second launch.  x / y are
    // [cols | rows][n_rhs][2][L][N]: a group is a strided slice, so the kernels take the full stride.  Measured on the 32 x 32 x
    // 1024-diagonal matvec of a packed GPT-2 layer, per token: 86 us single; 8 tokens: 75 us with one launch per group (W re-read from
    // HBM by every group), see MEASUREMENTS.md for the XCD-grouped launch.
    const size_t pairs = n_rhs / 2;
    const uint64_t* x_last = d_x + (n_rhs - 1) * 2 * poly;   // an odd last right-hand side
    uint64_t* y_last = d_y + (n_rhs - 1) * 2 * poly;
    int rc = DPFHE_SUCCESS;
    if (c->fold) {   // split-at-bit-30 column accumulators (kernels_misc.h matvec_fold_kernel), same grouping and block-id layout
        if (pairs) rc = matvec_multi_launch<true, kMatvecRt4, 4, kMatvecWpt4>(c, what, d_y, d_W, d_x, rows, cols, n_rhs, pairs, s);
        if (!rc && (n_rhs & 1)) rc = matvec_multi_launch<true, 4, 2, kMatvecWpt2>(c, what, y_last, d_W, x_last, rows, cols, n_rhs, 1, s);
    } else {
        if (pairs) rc = matvec_multi_launch<false, 4, 4>(c, what, d_y, d_W, d_x, rows, cols, n_rhs, pairs, s);
        if (!rc && (n_rhs & 1)) rc = matvec_multi_launch<false, 4, 2>(c, what, y_last, d_W, x_last, rows, cols, n_rhs, 1, s);
    }
    return rc;
}

extern "C" int dpfhe_matvec_scalar(dpfhe_ctx* c, uint64_t* d_y, const uint64_t* d_w, const uint64_t* d_x, size_t rows, size_t cols,
                                   void* stream) {
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_matvec_scalar", "null context");
    if (rows == 0) return DPFHE_SUCCESS;
    if (cols == 0) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_matvec_scalar", "cols must be > 0");
    if (!d_y || !d_w || !d_x || misaligned(d_y) || misaligned(d_x) || (reinterpret_cast<uintptr_t>(d_w) & 7))
        return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_matvec_scalar", "null or misaligned buffer");
    const int n = 1 << c->log2n;
    const int chunks = chunks_of(n);
    constexpr int RT = 8;
    const size_t blocks = ((rows + RT - 1) / RT) * c->n_limbs * (size_t)chunks;
    if (blocks > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_matvec_scalar", "too many rows for one launch");
    DPFHE_ON_DEVICE(c, "dpfhe_matvec_scalar");
    hipStream_t s = static_cast<hipStream_t>(stream);
    with_ctx_arith(c, [&](auto arith) {
        hipLaunchKernelGGL((matvec_scalar_kernel<decltype(arith), RT>), dim3((unsigned)blocks), dim3(256), 0, s, d_y, d_w, d_x, c->lc, (int)c->n_limbs, n, chunks, rows, cols);
    });
    return check_launch("matvec_scalar kernel launch");
}

extern "C" int dpfhe_reduce_sum(dpfhe_ctx* c, uint64_t* d_out, const uint64_t* d_in, size_t count, size_t components, void* stream) {
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_reduce_sum", "null context");
    if (components == 0 || count == 0) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_reduce_sum", "count and components must be > 0");
    if (!d_out || !d_in || misaligned(d_out) || misaligned(d_in)) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_reduce_sum", "null or misaligned buffer");
    const size_t blocks = components * c->n_limbs;
    if (blocks > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_reduce_sum", "too many components");
    DPFHE_ON_DEVICE(c, "dpfhe_reduce_sum");
    const int n = 1 << c->log2n;
    const int chunks = chunks_of(n);
    const size_t words_per_item = components * c->n_limbs * (size_t)n;
    // batch splits (their partial sums are combined with atomics): 15 for the large batches of the sharded multiply; a short batch (the
    // 32 rotated terms of a packed layer) keeps at least 8 items per split, so that every work item has 4 independent loads in flight
    const size_t want = count / 8 ? count / 8 : 1;
    const unsigned splits = (unsigned)(want < (size_t)kReduceSplits ? want : (size_t)kReduceSplits);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (blocks * (size_t)chunks * splits > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_reduce_sum", "too many components for one launch");
    HIP_TRY(hipMemsetAsync(d_out, 0, words_per_item * sizeof(u64), s));   // after every validation: a rejected call leaves d_out untouched
    const unsigned poly_chunks = (unsigned)(blocks * chunks);
    const unsigned items = poly_chunks * splits;
    // The ONE place that picks the partial-sum kernel.  The large batches of the sharded multiply on all-fold limbs: reduce_thin_kernel, one workgroup
    // per CU - the only placement that leaves both multiply workgroups of a CU resident while the reduce of the previous step runs beside them
    // (kernels_misc.h; a second thin workgroup on a CU would not fit the registers either).  Everything else - short batches (latency-bound: no cap),
    // the 32 rotated terms of a packed layer, limbs of another class: reduce_partial_kernel, as before.
    if (c->fold && count > 512) {
        const unsigned grid = items < (unsigned)c->n_cu ? items : (unsigned)c->n_cu;
        const unsigned threads = n / 2 < 256 ? (unsigned)n / 2 : 256u;   // N = 256: half a chunk
        unsigned log2_chunks = 0;
        while ((1 << log2_chunks) < chunks) ++log2_chunks;
        hipLaunchKernelGGL(reduce_thin_kernel, dim3(grid), dim3(threads), 0, s, d_out, d_in, c->lc, (unsigned)c->n_limbs, (unsigned)n, log2_chunks,
                           count / splits, (unsigned)(count % splits), words_per_item, poly_chunks, splits);
    } else {
        // two workgroups per CU walk the work items: as fast as an uncapped launch when alone (537 vs 551 us for 8192 x 3
        // components at N=4096) and 2 % faster for the multiply it overlaps with in bench.py
        unsigned grid = items;
        if (count > 512 && grid > 2u * (unsigned)c->n_cu) grid = 2u * (unsigned)c->n_cu;
        hipLaunchKernelGGL(reduce_partial_kernel, dim3(grid), dim3(256), 0, s, d_out, d_in, c->lc, (int)c->n_limbs, n, chunks, count, words_per_item,
                           poly_chunks, splits);
    }
    if (int e = check_launch("reduce_sum partial kernel launch")) return e;
    hipLaunchKernelGGL(reduce_final_kernel, dim3((unsigned)(blocks * chunks)), dim3(256), 0, s, d_out, c->lc, (int)c->n_limbs, n, chunks);
    return check_launch("reduce_sum kernel launch");
}

// words that are sums of at most 15 canonical residues (< 15 q < 2^64) -> canonical, in place: the one pass after an all-reduce of partial ciphertexts
extern "C" int dpfhe_canonicalize_sum(dpfhe_ctx* c, uint64_t* d_io, size_t n_rns_polys, void* stream) {
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_canonicalize_sum", "null context");
    if (n_rns_polys == 0) return DPFHE_SUCCESS;
    if (!d_io || misaligned(d_io)) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_canonicalize_sum", "null or misaligned buffer");
    const int n = 1 << c->log2n, chunks = chunks_of(n);
    const size_t blocks = n_rns_polys * c->n_limbs * (size_t)chunks;
    if (blocks > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_canonicalize_sum", "batch too large for one launch");
    DPFHE_ON_DEVICE(c, "dpfhe_canonicalize_sum");
    hipLaunchKernelGGL(reduce_final_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), d_io, c->lc, (int)c->n_limbs, n, chunks);
    return check_launch("canonicalize_sum kernel launch");
}

// ------------------------------------------------------------------------------------------------
// the fused rescales of the approximate family's activations (fused_rescale.h; kernels in kernels_misc.h)
// what a host twin has no context to take from: every limb's constants and the rescale constants of limbs [0, last) relative to limb `last`
static void host_limb_consts(const uint64_t* moduli, uint32_t n_limbs, std::vector<LimbConst>& lc, bool& fold) {
    lc.assign(n_limbs, LimbConst{});
    fold = true;
    for (uint32_t l = 0; l < n_limbs; ++l) {
        const u64 q = moduli[l];
        const unsigned __int128 ratio = (~(unsigned __int128)0) / q;
        lc[l].q = q;
        lc[l].d = fold_eligible(q) ? (1ull << 60) - q : 0;
        lc[l].br_hi = (u64)(ratio >> 64); lc[l].br_lo = (u64)ratio;
        lc[l].two64 = (u64)((((unsigned __int128)1) << 64) % q);
        fold = fold && fold_eligible(q);
    }
}
static int host_rescale_consts(const char* what, const uint64_t* moduli, size_t last, std::vector<RescaleConst>& rc) {
    rc.assign(last, RescaleConst{});
    bool coprime = true;
    fill_rescale_consts(rc.data(), moduli, last, [&](u64 a, u64 q) { uint64_t inv = 0; coprime = inverse_mod(a, q, inv) && coprime; return inv; });
    return coprime ? (int)DPFHE_SUCCESS : fail(DPFHE_INVALID_ARGUMENT, what, "moduli must be pairwise coprime");
}

extern "C" int dpfhe_relinearize_rescale_pass_host(const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n, uint64_t* out, const uint64_t* work_qp,
                                                   const uint64_t* in3, size_t batch) {
    static const char* what = "dpfhe_relinearize_rescale_pass_host";
    if (!moduli || !out || !work_qp || !in3) return fail(DPFHE_INVALID_ARGUMENT, what, "null argument");
    if (int rc = check_host_ring(what, moduli, n_limbs, log2_n)) return rc;
    if (n_limbs < 3) return fail(DPFHE_INVALID_STATE, what, "no data limb left to drop (Ld < 2)");
    const size_t n = (size_t)1 << log2_n, L = n_limbs, Ld = L - 1;
    if (overlaps(out, batch * 2 * (Ld - 1) * n, work_qp, batch * 2 * L * n) || overlaps(out, batch * 2 * (Ld - 1) * n, in3, batch * 3 * Ld * n))
        return fail(DPFHE_INVALID_ARGUMENT, what, "output overlaps an input");
    for (size_t p = 0; p < 2 * batch; ++p)
        for (size_t l = 0; l < L; ++l)
            for (size_t k = 0; k < n; ++k) {
                if (work_qp[(p * L + l) * n + k] >= moduli[l]) return fail(DPFHE_INVALID_ARGUMENT, what, "words must be canonical residues");
                if (l < Ld && in3[(((p >> 1) * 3 + (p & 1)) * Ld + l) * n + k] >= moduli[l]) return fail(DPFHE_INVALID_ARGUMENT, what, "words must be canonical residues");
            }
    std::vector<LimbConst> lc;
    std::vector<RescaleConst> rcp, rcq;
    bool fold;
    host_limb_consts(moduli, n_limbs, lc, fold);
    if (int rc = host_rescale_consts(what, moduli, L - 1, rcp)) return rc;
    if (int rc = host_rescale_consts(what, moduli, L - 2, rcq)) return rc;
    if (fold) relin_rescale_pass_host<FoldArith>(n, L, lc.data(), rcp.data(), rcq.data(), out, work_qp, in3, batch);
    else relin_rescale_pass_host<ShoupArith>(n, L, lc.data(), rcp.data(), rcq.data(), out, work_qp, in3, batch);
    return DPFHE_SUCCESS;
}

// the shape checks the device entry and the host twin of the linear combination share
static int lincomb_args(const char* what, const uint64_t* out, const uint64_t* x, const uint64_t* w, size_t n_terms, size_t batch, uint32_t limbs, uint32_t log2n) {
    if (!out || !x || !w) return fail(DPFHE_INVALID_ARGUMENT, what, "null buffer");
    if (limbs < 2) return fail(DPFHE_INVALID_STATE, what, "no limb left to drop");
    if (n_terms == 0 || n_terms > kLincombMaxTerms) return fail(DPFHE_INVALID_ARGUMENT, what, "1 to 16 terms");
    if (batch == 0) return fail(DPFHE_INVALID_ARGUMENT, what, "batch must be positive");
    const size_t n = (size_t)1 << log2n;
    if (batch > kMaxGrid / (2 * (size_t)(limbs - 1) * (size_t)chunks_of(n))) return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    const size_t out_words = batch * 2 * (limbs - 1) * n;
    if (overlaps(out, out_words, x, n_terms * batch * 2 * limbs * n) || overlaps(out, out_words, w, (n_terms + 1) * limbs))
        return fail(DPFHE_INVALID_ARGUMENT, what, "output overlaps an input");
    return DPFHE_SUCCESS;
}

extern "C" int dpfhe_lincomb_rescale(dpfhe_ctx* c, uint64_t* d_out, const uint64_t* d_x, const uint64_t* d_w, size_t n_terms, size_t batch, void* stream) {
    static const char* what = "dpfhe_lincomb_rescale";
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    if (int rc = lincomb_args(what, d_out, d_x, d_w, n_terms, batch, c->n_limbs, c->log2n)) return rc;
    if (misaligned(d_out) || misaligned(d_x) || misaligned(d_w)) return fail(DPFHE_INVALID_ARGUMENT, what, "misaligned buffer");
    DPFHE_ON_DEVICE(c, what);
    const int n = 1 << c->log2n, chunks = chunks_of(n);
    const size_t blocks = batch * 2 * (c->n_limbs - 1) * (size_t)chunks;
    with_ctx_arith(c, [&](auto arith) {
        hipLaunchKernelGGL((lincomb_rescale_kernel<decltype(arith)>), dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), d_out, d_x, d_w, c->lc,
                           c->d_rescale, (int)c->n_limbs, n, chunks, (int)n_terms, batch);
    });
    return check_launch("lincomb_rescale kernel launch");
}

extern "C" int dpfhe_lincomb_rescale_host(const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n, uint64_t* out, const uint64_t* x, const uint64_t* w,
                                          size_t n_terms, size_t batch) {
    static const char* what = "dpfhe_lincomb_rescale_host";
    if (!moduli) return fail(DPFHE_INVALID_ARGUMENT, what, "null moduli");
    if (int rc = check_host_ring(what, moduli, n_limbs, log2_n)) return rc;
    if (int rc = lincomb_args(what, out, x, w, n_terms, batch, n_limbs, log2_n)) return rc;
    const size_t n = (size_t)1 << log2_n, L = n_limbs;
    for (size_t i = 0; i < n_terms * batch * 2 * L; ++i)
        for (size_t k = 0; k < n; ++k)
            if (x[i * n + k] >= moduli[i % L]) return fail(DPFHE_INVALID_ARGUMENT, what, "words must be canonical residues");
    for (size_t i = 0; i < (n_terms + 1) * L; ++i)
        if (w[i] >= moduli[i % L]) return fail(DPFHE_INVALID_ARGUMENT, what, "weights must be canonical residues");
    std::vector<LimbConst> lc;
    std::vector<RescaleConst> rc;
    bool fold;
    host_limb_consts(moduli, n_limbs, lc, fold);
    if (int e = host_rescale_consts(what, moduli, L - 1, rc)) return e;
    if (fold) lincomb_rescale_host<FoldArith>(n, L, lc.data(), rc.data(), out, x, w, n_terms, batch);
    else lincomb_rescale_host<ShoupArith>(n, L, lc.data(), rc.data(), out, x, w, n_terms, batch);
    return DPFHE_SUCCESS;
}
