// cabi_keyswitch.hip - the C ABI's key switching: RNS-digit and hybrid keys on the fused relin_kernel of kernels.h (launch.h), composed above
// N = 8192 over kernels_keyswitch.h; the rescales, which are first of all key switching's division by P; the host twins of the fused rescales.
// The rotations (cabi_rotate.hip) borrow launch_rescale, launch_lift_digits, key_switch_hybrid and its first pass key_products_hybrid from here (cabi.h).
#include "cabi.h"
#include "fused_rescale.h"
#include "kernels_keyswitch.h"
#include "rotate_add.h"

// relin_kernel launches (`blocks` = items x L): on the context's policy, or - a MIXTURE of classes - one launch per class present, each over its own limbs
// (relin_kernel maps its workgroups through DevTables::active_map: the digits of every limb still enter every limb's transforms)
static int relin_launch(const dpfhe_ctx* c, int mode, u64* out, const u64* in, const u64* evk, size_t key_stride, unsigned key_group, size_t blocks, hipStream_t s) {
    if (class_mixture(c)) {
        const size_t items = blocks / c->n_limbs;
        return for_each_class(c, c->n_limbs, [&](const auto& tb) { return launch_relin((int)c->log2n, mode, out, in, evk, key_stride, key_group, items * (size_t)tb.n_active, tb, s); });
    }
    return with_policy(c, [&](const auto& tb) { return launch_relin((int)c->log2n, mode, out, in, evk, key_stride, key_group, blocks, tb, s); });
}

// ---- ring degrees above 8192: the fused kernels stop there (kernels_keyswitch.h); the same operations composed from the batched transforms
// and one-pass streaming kernels.  Their scratch comes from per-stream arenas (cabi.h StreamScratch).

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

static int key_switch_composed(dpfhe_ctx* c, uint64_t* d_out2, const uint64_t* d_in, int in_comps, int add_mask, const uint64_t* d_evk, size_t batch,
                               hipStream_t s, const char* what) {
    const size_t poly = (size_t)c->n_limbs << c->log2n, per = slice_items(c, batch, c->n_limbs * poly);
    return for_slices(batch, per, [&](size_t i, size_t m) {
        return key_switch_composed_slice(c, d_out2 + i * 2 * poly, d_in + i * (size_t)in_comps * poly, in_comps, add_mask, d_evk, m, s, what);
    });
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
void launch_rescale(const dpfhe_ctx* c, size_t blocks, hipStream_t s, u64* out, const u64* in, const u64* add, int add_comps, int add_mask) {
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
void launch_lift_digits(const dpfhe_ctx* c, size_t grid, hipStream_t s, u64* digits, const u64* comp, size_t item_stride, int chunks) {
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
int key_switch_hybrid(dpfhe_ctx* c, const char* what, int in_comps, uint64_t* d_out2, const uint64_t* d_in, const uint64_t* d_key,
                      uint64_t* d_work, size_t batch, void* stream, size_t key_stride, unsigned key_group, bool drop_last) {
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
    if (!key_products_fit(c, batch, key_stride, key_group)) return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    DPFHE_ON_DEVICE(c, "hybrid key switch");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = key_products_hybrid(c, what, in_comps, d_work, d_in, d_key, batch, s, key_stride, key_group)) return rc;
    // divide by P with rounding and add c0 (and c1 for relinearisation): one pass over the 2*batch polynomials of `work`
    const int chunks = chunks_of(n);
    const size_t rblocks = batch * 2 * Ld * (size_t)chunks;
    if (rblocks > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    if (drop_last) {   // ... and by the last data prime in the same pass
        with_ctx_arith(c, [&](auto arith) {
            hipLaunchKernelGGL((relin_rescale_kernel<decltype(arith)>), dim3((unsigned)relin_rescale_grid(batch, Ld, (size_t)n)), dim3(256), 0, s, d_out2, d_work, d_in, c->lc,
                               c->d_rescale, c->d_rescale2, (int)L, n, chunks);
        });
        return check_launch("hybrid rescale-twice launch");
    }
    launch_rescale(c, rblocks, s, d_out2, d_work, d_in, in_comps, in_comps == 3 ? 3 : 1);
    return check_launch("hybrid rescale launch");
}

// the fused key-switch launch of `batch` items fits one grid (the grouped and key-major launches pad the grid to whole XCD rounds: the launcher's own
// plan; a launch per limb class is no larger)
bool key_products_fit(const dpfhe_ctx* c, size_t batch, size_t key_stride, unsigned key_group) {
    const size_t blocks = batch * c->n_limbs;
    return blocks <= kMaxGrid && RelinMap::plan(blocks, c->n_limbs, key_stride, key_group).grid <= kMaxGrid;
}

// The first pass of hybrid key switching alone: d_work [batch][2][L][N] (coefficient domain over Q P) = sum_j [last component of item]_{q_j} key_j, nothing
// added, nothing divided.  d_in: [batch][in_comps][Ld][N].  Arguments validated (key_products_fit included), device selected by the caller.
int key_products_hybrid(dpfhe_ctx* c, const char* what, int in_comps, uint64_t* d_work, const uint64_t* d_in, const uint64_t* d_key, size_t batch, hipStream_t s,
                        size_t key_stride, unsigned key_group) {
    const size_t L = c->n_limbs, Ld = L - 1, blocks = batch * L, kg = key_group ? key_group : 1;
    const int n = 1 << c->log2n;
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
        return check_launch("hybrid key-switch kernel launch");
    }
    return DPFHE_SUCCESS;
}

extern "C" int dpfhe_relinearize_hybrid(dpfhe_ctx* c, uint64_t* d_out2, const uint64_t* d_in3, const uint64_t* d_key, uint64_t* d_work, size_t batch,
                                        void* stream) {
    return key_switch_hybrid(c, "dpfhe_relinearize_hybrid", 3, d_out2, d_in3, d_key, d_work, batch, stream);
}
extern "C" int dpfhe_switch_key_hybrid(dpfhe_ctx* c, uint64_t* d_out2, const uint64_t* d_in2, const uint64_t* d_key, uint64_t* d_work, size_t batch,
                                       void* stream) {
    return key_switch_hybrid(c, "dpfhe_switch_key_hybrid", 2, d_out2, d_in2, d_key, d_work, batch, stream);
}
extern "C" int dpfhe_relinearize_rescale_hybrid(dpfhe_ctx* c, uint64_t* d_out2, const uint64_t* d_in3, const uint64_t* d_key, uint64_t* d_work, size_t batch,
                                                void* stream) {
    return key_switch_hybrid(c, "dpfhe_relinearize_rescale_hybrid", 3, d_out2, d_in3, d_key, d_work, batch, stream, 0, 1, true);
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

// ------------------------------------------------------------------------------------------------
// the fused rescales of the approximate family's activations (fused_rescale.h; kernels in kernels_keyswitch.h)
// what a host twin has no context to take from: every limb's constants, which arithmetic they allow, and the rescale constants of the limbs below the
// last one relative to it (rc_last) and - two_levels - of those below the one before it relative to that (rc_prev)
struct HostRing {
    std::vector<LimbConst> lc;
    std::vector<RescaleConst> rc_last, rc_prev;
    bool fold = true;
    int build(const char* what, const uint64_t* moduli, uint32_t n_limbs, bool two_levels) {
        lc.assign(n_limbs, LimbConst{});
        for (uint32_t l = 0; l < n_limbs; ++l) {
            lc[l] = limb_const_of_modulus(moduli[l]);
            fold = fold && fold_eligible(moduli[l]);
        }
        bool coprime = true;
        auto inv = [&](u64 a, u64 q) { uint64_t r = 0; coprime = inverse_mod(a, q, r) && coprime; return r; };
        rc_last.assign(n_limbs - 1, RescaleConst{});
        fill_rescale_consts(rc_last.data(), moduli, n_limbs - 1, inv);
        if (coprime && two_levels) {
            rc_prev.assign(n_limbs - 2, RescaleConst{});
            fill_rescale_consts(rc_prev.data(), moduli, n_limbs - 2, inv);
        }
        return coprime ? (int)DPFHE_SUCCESS : fail(DPFHE_INVALID_ARGUMENT, what, "moduli must be pairwise coprime");
    }
};
// f(FoldArith{} or ShoupArith{}): the twin runs in the arithmetic a context on these moduli would launch with (cabi.h with_ctx_arith)
template <class Fn>
static void with_host_arith(bool fold, Fn f) { fold ? f(FoldArith{}) : f(ShoupArith{}); }

// p: [rows][row_limbs][n], of which the first read_limbs limbs of every row are read: each word below its limb's modulus
static int canonical_rows(const char* what, const uint64_t* p, size_t rows, size_t row_limbs, size_t read_limbs, const uint64_t* moduli, size_t n,
                          const char* detail = "words must be canonical residues") {
    for (size_t r = 0; r < rows; ++r)
        for (size_t l = 0; l < read_limbs; ++l)
            for (size_t k = 0; k < n; ++k)
                if (p[(r * row_limbs + l) * n + k] >= moduli[l]) return fail(DPFHE_INVALID_ARGUMENT, what, detail);
    return DPFHE_SUCCESS;
}
// ... of the product's components 0 and 1 (in3: [batch][3][Ld][n])
static int canonical_c0_c1(const char* what, const uint64_t* in3, size_t batch, size_t Ld, const uint64_t* moduli, size_t n) {
    for (size_t b = 0; b < batch; ++b)
        if (int rc = canonical_rows(what, in3 + b * 3 * Ld * n, 2, Ld, Ld, moduli, n)) return rc;
    return DPFHE_SUCCESS;
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
    if (int rc = canonical_rows(what, work_qp, 2 * batch, L, L, moduli, n)) return rc;
    if (int rc = canonical_c0_c1(what, in3, batch, Ld, moduli, n)) return rc;
    HostRing r;
    if (int rc = r.build(what, moduli, n_limbs, true)) return rc;
    with_host_arith(r.fold, [&](auto arith) {
        relin_rescale_pass_host<decltype(arith)>(n, L, r.lc.data(), r.rc_last.data(), r.rc_prev.data(), out, work_qp, in3, batch);
    });
    return DPFHE_SUCCESS;
}

// host twin of the last pass of a rotate-and-add step (rotate_add.h; the device pass is cabi_rotate.hip's): a division by P like the one above
extern "C" int dpfhe_rotate_add_pass_host(const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n, uint64_t* out, const uint64_t* work_qp, const uint64_t* in2,
                                          uint32_t galois_elt, size_t batch) {
    static const char* what = "dpfhe_rotate_add_pass_host";
    if (!moduli || !out || !work_qp || !in2) return fail(DPFHE_INVALID_ARGUMENT, what, "null argument");
    if (int rc = check_host_ring(what, moduli, n_limbs, log2_n)) return rc;
    if (n_limbs < 2) return fail(DPFHE_INVALID_STATE, what, "the extended basis needs at least one data limb and the special prime");
    const size_t n = (size_t)1 << log2_n, L = n_limbs, Ld = L - 1;
    if (!(galois_elt & 1u) || galois_elt >= 2 * n) return fail(DPFHE_INVALID_ARGUMENT, what, "galois_elt must be odd and < 2N");
    if (overlaps(out, batch * 2 * Ld * n, work_qp, batch * 2 * L * n) || overlaps(out, batch * 2 * Ld * n, in2, batch * 2 * Ld * n))
        return fail(DPFHE_INVALID_ARGUMENT, what, "output overlaps an input");
    if (int rc = canonical_rows(what, work_qp, 2 * batch, L, L, moduli, n)) return rc;
    if (int rc = canonical_rows(what, in2, 2 * batch, Ld, Ld, moduli, n)) return rc;
    HostRing r;
    if (int rc = r.build(what, moduli, n_limbs, false)) return rc;
    const unsigned g_inv = galois_inverse(galois_elt, 2u * (unsigned)n);
    with_host_arith(r.fold, [&](auto arith) { rotate_add_pass_host<decltype(arith)>(n, L, r.lc.data(), r.rc_last.data(), out, work_qp, in2, g_inv, batch); });
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
    if (int rc = canonical_rows(what, x, n_terms * batch * 2, L, L, moduli, n)) return rc;
    if (int rc = canonical_rows(what, w, n_terms + 1, L, L, moduli, 1, "weights must be canonical residues")) return rc;
    HostRing r;
    if (int rc = r.build(what, moduli, n_limbs, false)) return rc;
    with_host_arith(r.fold, [&](auto arith) { lincomb_rescale_host<decltype(arith)>(n, L, r.lc.data(), r.rc_last.data(), out, x, w, n_terms, batch); });
    return DPFHE_SUCCESS;
}

// ---- a relinearised product + scalar linear combination + rescale in one last pass (fused_rescale.h (c)) ----------------------------------------------------
// what the device entry and the host twin check alike: the counts, the terms' heights, and that the output overlaps no input
static int relin_lincomb_args(const char* what, const uint64_t* out, const uint64_t* in3, const uint64_t* const* terms, const uint32_t* term_limbs, size_t n_terms,
                              const uint64_t* w, size_t batch, size_t Ld, size_t n) {
    if (n_terms > kRelinLincombMaxTerms) return fail(DPFHE_INVALID_ARGUMENT, what, "0 to 15 terms");
    if (!out || !in3 || !w || (n_terms && (!terms || !term_limbs))) return fail(DPFHE_INVALID_ARGUMENT, what, "null or misaligned buffer");
    const size_t out_words = batch * 2 * (Ld - 1) * n;
    if (overlaps(out, out_words, in3, batch * 3 * Ld * n) || overlaps(out, out_words, w, (n_terms + 2) * Ld)) return fail(DPFHE_INVALID_ARGUMENT, what, "output overlaps an input");
    for (size_t k = 0; k < n_terms; ++k) {
        if (!terms[k]) return fail(DPFHE_INVALID_ARGUMENT, what, "null or misaligned buffer");
        if (term_limbs[k] < Ld) return fail(DPFHE_INVALID_ARGUMENT, what, "a term has fewer limbs than the data context");
        if (overlaps(out, out_words, terms[k], batch * 2 * term_limbs[k] * n)) return fail(DPFHE_INVALID_ARGUMENT, what, "output overlaps an input");
    }
    return DPFHE_SUCCESS;
}

extern "C" int dpfhe_relinearize_lincomb_rescale_hybrid(dpfhe_ctx* c, uint64_t* d_out2, const uint64_t* d_in3, const uint64_t* d_key, uint64_t* d_work,
                                                        const uint64_t* const* d_terms, const uint32_t* term_limbs, size_t n_terms, const uint64_t* d_w,
                                                        size_t batch, void* stream) {
    static const char* what = "dpfhe_relinearize_lincomb_rescale_hybrid";
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    if (int rc = check_extended(c, what)) return rc;
    if (c->n_limbs < 3) return fail(DPFHE_INVALID_STATE, what, "no data limb left to drop (Ld < 2)");
    if (batch == 0) return DPFHE_SUCCESS;
    const size_t L = c->n_limbs, Ld = L - 1, n = (size_t)1 << c->log2n;
    if (!d_key || !d_work) return fail(DPFHE_INVALID_ARGUMENT, what, "null or misaligned buffer");
    if (int rc = relin_lincomb_args(what, d_out2, d_in3, d_terms, term_limbs, n_terms, d_w, batch, Ld, n)) return rc;
    bool skew = misaligned(d_out2) || misaligned(d_in3) || misaligned(d_key) || misaligned(d_work) || misaligned(d_w);
    for (size_t k = 0; k < n_terms; ++k) skew = skew || misaligned(d_terms[k]);
    if (skew) return fail(DPFHE_INVALID_ARGUMENT, what, "null or misaligned buffer");
    {   // pass 1 writes the work buffer while it reads the input and the key; the last pass reads everything else while it writes the output
        const size_t out_words = batch * 2 * (Ld - 1) * n, work_words = batch * 2 * L * n, key_words = Ld * 2 * L * n;
        bool hit = overlaps(d_work, work_words, d_out2, out_words) || overlaps(d_work, work_words, d_in3, batch * 3 * Ld * n) || overlaps(d_work, work_words, d_key, key_words) ||
                   overlaps(d_work, work_words, d_w, (n_terms + 2) * Ld) || overlaps(d_out2, out_words, d_key, key_words);
        for (size_t k = 0; k < n_terms; ++k) hit = hit || overlaps(d_work, work_words, d_terms[k], batch * 2 * term_limbs[k] * n);
        if (hit) return fail(DPFHE_INVALID_ARGUMENT, what, "the output and the work buffer must not overlap each other or any input");
    }
    if (!key_products_fit(c, batch, 0, 1) || relin_rescale_grid(batch, Ld, n) > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    DPFHE_ON_DEVICE(c, what);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = key_products_hybrid(c, what, 3, d_work, d_in3, d_key, batch, s, 0, 1)) return rc;
    LincombTerms terms{};
    for (size_t k = 0; k < n_terms; ++k) { terms.z[k] = d_terms[k]; terms.limbs[k] = term_limbs[k]; }
    with_ctx_arith(c, [&](auto arith) {
        hipLaunchKernelGGL((relin_lincomb_rescale_kernel<decltype(arith)>), dim3((unsigned)relin_rescale_grid(batch, Ld, n)), dim3(256), 0, s, d_out2, d_work, d_in3, terms,
                           d_w, c->lc, c->d_rescale, c->d_rescale2, (int)L, (int)n, chunks_of(n), (int)n_terms);
    });
    return check_launch("hybrid relinearise-combine-rescale launch");
}

extern "C" int dpfhe_relinearize_lincomb_rescale_pass_host(const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n, uint64_t* out, const uint64_t* work_qp,
                                                           const uint64_t* in3, const uint64_t* const* terms, const uint32_t* term_limbs, size_t n_terms,
                                                           const uint64_t* w, size_t batch) {
    static const char* what = "dpfhe_relinearize_lincomb_rescale_pass_host";
    if (!moduli || !work_qp) return fail(DPFHE_INVALID_ARGUMENT, what, "null argument");
    if (int rc = check_host_ring(what, moduli, n_limbs, log2_n)) return rc;
    if (n_limbs < 3) return fail(DPFHE_INVALID_STATE, what, "no data limb left to drop (Ld < 2)");
    const size_t n = (size_t)1 << log2_n, L = n_limbs, Ld = L - 1;
    if (int rc = relin_lincomb_args(what, out, in3, terms, term_limbs, n_terms, w, batch, Ld, n)) return rc;
    if (overlaps(out, batch * 2 * (Ld - 1) * n, work_qp, batch * 2 * L * n)) return fail(DPFHE_INVALID_ARGUMENT, what, "output overlaps an input");
    if (int rc = canonical_rows(what, work_qp, 2 * batch, L, L, moduli, n)) return rc;
    if (int rc = canonical_c0_c1(what, in3, batch, Ld, moduli, n)) return rc;
    for (size_t t = 0; t < n_terms; ++t)   // of a term, as of the device entry, only the first Ld limbs are read
        if (int rc = canonical_rows(what, terms[t], 2 * batch, term_limbs[t], Ld, moduli, n)) return rc;
    if (int rc = canonical_rows(what, w, n_terms + 2, Ld, Ld, moduli, 1, "weights must be canonical residues")) return rc;
    HostRing r;
    if (int rc = r.build(what, moduli, n_limbs, true)) return rc;
    with_host_arith(r.fold, [&](auto arith) {
        relin_lincomb_rescale_pass_host<decltype(arith)>(n, L, r.lc.data(), r.rc_last.data(), r.rc_prev.data(), out, work_qp, in3, terms, term_limbs, n_terms, w, batch);
    });
    return DPFHE_SUCCESS;
}
