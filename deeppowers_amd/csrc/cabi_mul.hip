// cabi_mul.hip - the C ABI's ciphertext multiply: dpfhe_ct_mul on the fused kernels of kernels.h (launch.h), composed above N = 8192 over
// kernels_mul.h, its traced diagnostic form, dpfhe_ct_mul_sum (sums of products), dpfhe_ct_mul_complement (products with a shared complement factor) and
// dpfhe_ct_mul_outer (all pairs of two operand lists), all three composed at every ring degree.  cabi.h lists the other units and states the ABI's conventions.
#include "cabi.h"
#include "kernels_mul.h"

// ---- ring degrees above 8192: the fused kernels stop there (kernels_mul.h); the same operation composed from the batched transforms
// and a one-pass streaming kernel.  Its scratch comes from per-stream arenas (cabi.h StreamScratch).

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

static int ct_mul_composed(dpfhe_ctx* c, uint64_t* d_out3, const uint64_t* d_a2, const uint64_t* d_b2, size_t batch, uint32_t flags, hipStream_t s) {
    const size_t poly = (size_t)c->n_limbs << c->log2n, per = slice_items(c, batch, 4 * poly);
    return for_slices(batch, per, [&](size_t i, size_t m) { return ct_mul_composed_slice(c, d_out3 + i * 3 * poly, d_a2 + i * 2 * poly, d_b2 + i * 2 * poly, m, flags, s); });
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

// ---- a sum of tensor products (include/dpfhe.h dpfhe_ct_mul_sum): always composed, at every ring degree - batched forward transforms into the stream's arena,
// tensor3_sum_kernel (kernels_mul.h), three inverse transforms per group.

struct MulSumCall {
    dpfhe_ctx* c;
    uint32_t flags;
    hipStream_t s;
    size_t terms_total;   // the terms of a group as the CALLER laid them out (strides of d_a2 / d_b2)
    bool shared, square;
};

static int mul_sum_kernel_launch(const MulSumCall& k, uint64_t* d_out3, const u64* pa, const u64* pb, size_t groups, size_t terms, bool b_shared, bool accumulate) {
    dpfhe_ctx* c = k.c;
    const size_t L = c->n_limbs, n = (size_t)1 << c->log2n;
    const size_t grid = mul_sum_grid(groups, L, n);
    with_ctx_arith(c, [&](auto arith) {
        hipLaunchKernelGGL((tensor3_sum_kernel<decltype(arith)>), dim3((unsigned)grid), dim3(256), 0, k.s, d_out3, pa, pb, c->lc, (int)L, (int)n, chunks_of(n), (int)terms,
                           (int)b_shared, (int)accumulate);
    });
    return check_launch("tensor product sum kernel launch");
}

static int ct_mul_sum_composed(const MulSumCall& k, uint64_t* d_out3, const uint64_t* d_a2, const uint64_t* d_b2, size_t groups) {
    dpfhe_ctx* c = k.c;
    const size_t L = c->n_limbs, poly = L << c->log2n, terms = k.terms_total, item = terms * 2 * poly;   // item: one group's operand
    const bool out_ntt = (k.flags & DPFHE_OUT_NTT) != 0;
    if (k.flags & DPFHE_IN_NTT) {   // no scratch: one launch over everything
        if (int rc = mul_sum_kernel_launch(k, d_out3, d_a2, d_b2, groups, terms, k.shared, false)) return rc;
        return out_ntt ? DPFHE_SUCCESS : ntt_launch(c, true, d_out3, d_out3, groups * 3 * L, k.s);
    }
    // Scratch for the transformed operands: [b, when shared | slice of a | that slice of b, when it has its own and is not a itself]
    const size_t limit = c->scratch_limit_words.load(std::memory_order_relaxed);
    const size_t fixed = k.shared ? item : 0, per_group = (k.shared || k.square ? 1 : 2) * item;
    StreamScratch ws(c, k.s);
    if (fixed + per_group <= limit) {   // whole groups fit: slices of groups
        const size_t fit = (limit - fixed) / per_group, per = fit < groups ? fit : groups;
        if (int rc = ws.alloc(fixed + per * per_group, "dpfhe_ct_mul_sum (scratch for the transformed operands)")) return rc;
        if (k.shared) if (int rc = ntt_launch(c, false, ws.p, d_b2, terms * 2 * L, k.s)) return rc;   // once for all slices
        return for_slices(groups, per, [&](size_t g0, size_t m) {
            u64* ta = ws.p + fixed;
            u64* tb = k.shared ? ws.p : k.square ? ta : ta + m * item;
            if (int rc = ntt_launch(c, false, ta, d_a2 + g0 * item, m * terms * 2 * L, k.s)) return rc;
            if (!k.shared && !k.square) if (int rc = ntt_launch(c, false, tb, d_b2 + g0 * item, m * terms * 2 * L, k.s)) return rc;
            if (int rc = mul_sum_kernel_launch(k, d_out3 + g0 * 3 * poly, ta, tb, m, terms, k.shared, false)) return rc;
            return out_ntt ? (int)DPFHE_SUCCESS : ntt_launch(c, true, d_out3 + g0 * 3 * poly, d_out3 + g0 * 3 * poly, m * 3 * L, k.s);
        });
    }
    // one group does not fit: group by group, each cut into ranges of terms that accumulate into its NTT-domain output; the inverse transforms come last
    const size_t per_term = (k.square ? 2 : 4) * poly, fit = limit / per_term, per = fit == 0 ? 1 : (fit < terms ? fit : terms);
    if (int rc = ws.alloc(per * per_term, "dpfhe_ct_mul_sum (scratch for a range of transformed terms)")) return rc;
    for (size_t g = 0; g < groups; ++g) {
        const u64 *ga = d_a2 + g * item, *gb = d_b2 + (k.shared ? 0 : g * item);
        u64* go = d_out3 + g * 3 * poly;
        if (int rc = for_slices(terms, per, [&](size_t t0, size_t m) {
                u64 *ta = ws.p, *tb = k.square ? ta : ta + m * 2 * poly;
                if (int rc = ntt_launch(c, false, ta, ga + t0 * 2 * poly, m * 2 * L, k.s)) return rc;
                if (!k.square) if (int rc = ntt_launch(c, false, tb, gb + t0 * 2 * poly, m * 2 * L, k.s)) return rc;
                return mul_sum_kernel_launch(k, go, ta, tb, 1, m, false, t0 != 0);
            })) return rc;
        if (!out_ntt) if (int rc = ntt_launch(c, true, go, go, 3 * L, k.s)) return rc;
    }
    return DPFHE_SUCCESS;
}

extern "C" int dpfhe_ct_mul_sum(dpfhe_ctx* c, uint64_t* d_out3, const uint64_t* d_a2, const uint64_t* d_b2, size_t groups, size_t terms, size_t b_groups,
                                uint32_t flags, void* stream) {
    static const char* what = "dpfhe_ct_mul_sum";
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    if (flags & ~(DPFHE_IN_NTT | DPFHE_OUT_NTT)) return fail(DPFHE_INVALID_ARGUMENT, what, "unknown flag");
    if (terms == 0) return fail(DPFHE_INVALID_ARGUMENT, what, "terms must be at least 1");
    if (groups == 0) return DPFHE_SUCCESS;
    if (b_groups != 1 && b_groups != groups) return fail(DPFHE_INVALID_ARGUMENT, what, "b_groups must be 1 (shared) or groups");
    if (!d_out3 || !d_a2 || !d_b2 || misaligned(d_out3) || misaligned(d_a2) || misaligned(d_b2)) return fail(DPFHE_INVALID_ARGUMENT, what, "null or misaligned buffer");
    const size_t L = c->n_limbs, n = (size_t)1 << c->log2n, poly = L * n;
    // sizes first (a product that wraps size_t would pass the overlap test): every count below stays under 2^31 residue polynomials
    if (groups > kMaxGrid || terms > kMaxGrid || groups * terms > kMaxGrid / (2 * L) || mul_sum_grid(groups, L, n) > kMaxGrid || !ntt_grid_fits(c, groups * 3 * L) ||
        !ntt_grid_fits(c, groups * terms * 2 * L))
        return fail(DPFHE_INVALID_ARGUMENT, what, "groups * terms too large for one launch");
    if (overlaps(d_out3, groups * 3 * poly, d_a2, groups * terms * 2 * poly) || overlaps(d_out3, groups * 3 * poly, d_b2, b_groups * terms * 2 * poly))
        return fail(DPFHE_INVALID_ARGUMENT, what, "output overlaps an operand");
    DPFHE_ON_DEVICE(c, what);
    MulSumCall k{c, flags, static_cast<hipStream_t>(stream), terms, b_groups == 1 && groups > 1, d_a2 == d_b2 && b_groups == groups};
    return ct_mul_sum_composed(k, d_out3, d_a2, d_b2, groups);
}

// ---- products with a shared complement factor (include/dpfhe.h dpfhe_ct_mul_complement): always composed, at every ring degree - batched forward transforms of
// b and a into the stream's arena, tensor3_complement_kernel (kernels_mul.h), three inverse transforms per output item.  At N <= 8192 a fused form would have
// to hold the factor's transform in the workgroup across terms + 1 products; the composed form reuses the batched transforms as they are.

struct MulComplementCall {
    dpfhe_ctx* c;
    uint32_t flags;
    hipStream_t s;
    const u64* d_kappa;
};

// `groups` groups of `terms` items: a and out3 are the first group's; out_self null for no self product
static int mul_complement_kernel_launch(const MulComplementCall& k, u64* d_out3, u64* d_out_self, const u64* pa, const u64* pb, size_t groups, size_t terms) {
    dpfhe_ctx* c = k.c;
    const size_t L = c->n_limbs, n = (size_t)1 << c->log2n;
    const size_t grid = mul_complement_grid(groups, L, n);
    with_ctx_arith(c, [&](auto arith) {
        hipLaunchKernelGGL((tensor3_complement_kernel<decltype(arith)>), dim3((unsigned)grid), dim3(256), 0, k.s, d_out3, d_out_self, terms ? pa : pb, pb, k.d_kappa, c->lc, (int)L, (int)n,
                           chunks_of(n), (int)terms);
    });
    return check_launch("complement product kernel launch");
}

static int ct_mul_complement_composed(const MulComplementCall& k, uint64_t* d_out3, const uint64_t* d_a2, const uint64_t* d_b2, size_t groups, size_t terms, bool with_self) {
    dpfhe_ctx* c = k.c;
    const size_t L = c->n_limbs, poly = L << c->log2n;
    const bool out_ntt = (k.flags & DPFHE_OUT_NTT) != 0;
    u64* d_self = with_self ? d_out3 + groups * terms * 3 * poly : nullptr;
    auto inverse = [&](u64* p, size_t items) { return out_ntt || items == 0 ? (int)DPFHE_SUCCESS : ntt_launch(c, true, p, p, items * 3 * L, k.s); };
    if (k.flags & DPFHE_IN_NTT) {   // no scratch: one launch over everything
        if (int rc = mul_complement_kernel_launch(k, d_out3, d_self, d_a2, d_b2, groups, terms)) return rc;
        return inverse(d_out3, groups * (terms + (with_self ? 1 : 0)));
    }
    // Scratch for the transformed operands: [slice of b | that slice's a]
    const size_t limit = c->scratch_limit_words.load(std::memory_order_relaxed), item = 2 * poly, per_group = (terms + 1) * item;
    StreamScratch ws(c, k.s);
    if (per_group <= limit) {   // whole groups fit: slices of groups
        const size_t fit = limit / per_group, per = fit < groups ? fit : groups;
        if (int rc = ws.alloc(per * per_group, "dpfhe_ct_mul_complement (scratch for the transformed operands)")) return rc;
        return for_slices(groups, per, [&](size_t g0, size_t m) {
            u64 *tb = ws.p, *ta = ws.p + m * item;
            u64* go = d_out3 + g0 * terms * 3 * poly;
            if (int rc = ntt_launch(c, false, tb, d_b2 + g0 * item, m * 2 * L, k.s)) return rc;
            if (terms) if (int rc = ntt_launch(c, false, ta, d_a2 + g0 * terms * item, m * terms * 2 * L, k.s)) return rc;
            if (int rc = mul_complement_kernel_launch(k, go, with_self ? d_self + g0 * 3 * poly : nullptr, ta, tb, m, terms)) return rc;
            if (int rc = inverse(go, m * terms)) return rc;
            return with_self ? inverse(d_self + g0 * 3 * poly, m) : (int)DPFHE_SUCCESS;
        });
    }
    // one group does not fit: group by group, b[g]'s transform kept across ranges of that group's numerators; the self product goes with the first range
    const size_t fit = limit > item ? (limit - item) / item : 0, per = fit == 0 ? 1 : (fit < terms ? fit : terms);
    if (int rc = ws.alloc((1 + per) * item, "dpfhe_ct_mul_complement (scratch for a range of transformed items)")) return rc;
    for (size_t g = 0; g < groups; ++g) {
        u64 *tb = ws.p, *ta = ws.p + item;
        if (int rc = ntt_launch(c, false, tb, d_b2 + g * item, 2 * L, k.s)) return rc;
        if (terms == 0) if (int rc = mul_complement_kernel_launch(k, d_out3, d_self + g * 3 * poly, tb, tb, 1, 0)) return rc;   // (with_self: the entry checked)
        if (int rc = for_slices(terms, per, [&](size_t t0, size_t m) {
                u64* go = d_out3 + (g * terms + t0) * 3 * poly;
                if (int rc = ntt_launch(c, false, ta, d_a2 + (g * terms + t0) * item, m * 2 * L, k.s)) return rc;
                if (int rc = mul_complement_kernel_launch(k, go, with_self && t0 == 0 ? d_self + g * 3 * poly : nullptr, ta, tb, 1, m)) return rc;
                return inverse(go, m);
            })) return rc;
        if (with_self) if (int rc = inverse(d_self + g * 3 * poly, 1)) return rc;
    }
    return DPFHE_SUCCESS;
}

extern "C" int dpfhe_ct_mul_complement(dpfhe_ctx* c, uint64_t* d_out3, const uint64_t* d_a2, const uint64_t* d_b2, const uint64_t* d_kappa, size_t groups, size_t terms,
                                       int with_self, uint32_t flags, void* stream) {
    static const char* what = "dpfhe_ct_mul_complement";
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    if (flags & ~(DPFHE_IN_NTT | DPFHE_OUT_NTT)) return fail(DPFHE_INVALID_ARGUMENT, what, "unknown flag");
    if (terms == 0 && !with_self) return fail(DPFHE_INVALID_ARGUMENT, what, "terms must be at least 1 when there is no self product");
    if (groups == 0) return DPFHE_SUCCESS;
    if (!d_out3 || !d_b2 || !d_kappa || (terms && !d_a2) || misaligned(d_out3) || misaligned(d_a2) || misaligned(d_b2) || misaligned(d_kappa))
        return fail(DPFHE_INVALID_ARGUMENT, what, "null or misaligned buffer");
    const size_t L = c->n_limbs, n = (size_t)1 << c->log2n, poly = L * n;
    // sizes first (a product that wraps size_t would pass the overlap test): every count below stays under 2^31 residue polynomials
    if (groups > kMaxGrid || terms > kMaxGrid || groups * (terms + 1) > kMaxGrid / (3 * L) || mul_complement_grid(groups, L, n) > kMaxGrid ||
        !ntt_grid_fits(c, groups * (terms + 1) * 3 * L))
        return fail(DPFHE_INVALID_ARGUMENT, what, "groups * (terms + 1) too large for one launch");
    const size_t out_words = groups * (terms + (with_self ? 1 : 0)) * 3 * poly;
    if ((terms && overlaps(d_out3, out_words, d_a2, groups * terms * 2 * poly)) || overlaps(d_out3, out_words, d_b2, groups * 2 * poly) || overlaps(d_out3, out_words, d_kappa, L))
        return fail(DPFHE_INVALID_ARGUMENT, what, "output overlaps an operand");
    DPFHE_ON_DEVICE(c, what);
    MulComplementCall k{c, flags, static_cast<hipStream_t>(stream), d_kappa};
    return ct_mul_complement_composed(k, d_out3, d_a2, d_b2, groups, terms, with_self != 0);
}

// ---- all pairs of two operand lists (include/dpfhe.h dpfhe_ct_mul_outer): always composed, at every ring degree - batched forward transforms of a and of b into
// the stream's arena (each operand transformed ONCE, not once per pair), tensor3_outer_kernel (kernels_mul.h), three inverse transforms per pair in place.

struct MulOuterCall {
    dpfhe_ctx* c;
    uint32_t flags;
    hipStream_t s;
    size_t b_total;   // the keys of the whole call: the row length of the full form's output
    bool causal;
};

// the scratch plan, in ITEMS of 2 L N words (the header states it): the operands' ranges per launch
struct MulOuterPlan { size_t a_per, b_per; bool shared; };   // shared: one transform serves both operands (a squaring that fits whole)
static MulOuterPlan mul_outer_plan(size_t fit, size_t A, size_t B, bool square) {
    if ((square ? A : A + B) <= fit) return MulOuterPlan{A, B, square};
    if (A + 1 <= fit) return MulOuterPlan{A, fit - A < B ? fit - A : B, false};   // a whole, b in ranges
    // a in ranges of whole tiles on half of what fits (one tile at least), b in ranges on the rest (half a tile of keys at least)
    const size_t tile = (size_t)kMulOuterTile;
    size_t a_per = fit / 2 / tile * tile;
    if (a_per < tile) a_per = tile;
    size_t b_per = fit > a_per ? fit - a_per : 0;
    if (b_per < tile / 2) b_per = tile / 2;
    return MulOuterPlan{a_per < A ? a_per : A, b_per < B ? b_per : B, false};
}

// pa, pb: the transformed rows of the ranges [a_off, a_off + a_count) and [b_off, b_off + b_count); d_out3: the whole output
static int mul_outer_kernel_launch(const MulOuterCall& k, u64* d_out3, const u64* pa, const u64* pb, size_t a_count, size_t b_count, size_t a_off, size_t b_off) {
    dpfhe_ctx* c = k.c;
    const size_t L = c->n_limbs, n = (size_t)1 << c->log2n;
    const size_t grid = MulOuterMap::grid(a_count, L, n);   // (<= the whole call's, which the entry checked)
    with_ctx_arith(c, [&](auto arith) {
        hipLaunchKernelGGL((tensor3_outer_kernel<decltype(arith)>), dim3((unsigned)grid), dim3(256), 0, k.s, d_out3, pa, pb, c->lc, (int)L, (int)n, chunks_of(n),
                           (unsigned)MulOuterMap::tiles(a_count), a_count, b_count, a_off, b_off, k.b_total, (int)k.causal);
    });
    return check_launch("outer tensor product kernel launch");
}

static int ct_mul_outer_composed(const MulOuterCall& k, uint64_t* d_out3, const uint64_t* d_a2, const uint64_t* d_b2, size_t A, size_t B) {
    dpfhe_ctx* c = k.c;
    const size_t L = c->n_limbs, poly = L << c->log2n, item = 2 * poly;
    const size_t pairs = k.causal ? A * (A + 1) / 2 : A * B;
    auto inverse = [&]() { return (k.flags & DPFHE_OUT_NTT) ? (int)DPFHE_SUCCESS : ntt_launch(c, true, d_out3, d_out3, pairs * 3 * L, k.s); };
    if (k.flags & DPFHE_IN_NTT) {   // no scratch: one launch over everything
        if (int rc = mul_outer_kernel_launch(k, d_out3, d_a2, d_b2, A, B, 0, 0)) return rc;
        return inverse();
    }
    // Scratch for the transformed operands: [range of a | range of b]; the products of different ranges are independent - nothing accumulates
    const MulOuterPlan pl = mul_outer_plan(c->scratch_limit_words.load(std::memory_order_relaxed) / item, A, B, d_a2 == d_b2 && A == B);
    StreamScratch ws(c, k.s);
    if (int rc = ws.alloc((pl.a_per + (pl.shared ? 0 : pl.b_per)) * item, "dpfhe_ct_mul_outer (scratch for the transformed operands)")) return rc;
    u64 *ta = ws.p, *tb = pl.shared ? ws.p : ws.p + pl.a_per * item;
    if (int rc = for_slices(A, pl.a_per, [&](size_t a0, size_t am) {
            if (int rc = ntt_launch(c, false, ta, d_a2 + a0 * item, am * 2 * L, k.s)) return rc;
            // under the causal flag the blocks wholly above the diagonal are empty: the keys past the range's last query are neither transformed nor walked
            const size_t b_end = k.causal && a0 + am < B ? a0 + am : B;
            return for_slices(b_end, pl.b_per, [&](size_t b0, size_t bm) {
                if (!pl.shared) if (int rc = ntt_launch(c, false, tb, d_b2 + b0 * item, bm * 2 * L, k.s)) return rc;
                return mul_outer_kernel_launch(k, d_out3, ta, tb, am, bm, a0, b0);
            });
        })) return rc;
    return inverse();
}

extern "C" int dpfhe_ct_mul_outer(dpfhe_ctx* c, uint64_t* d_out3, const uint64_t* d_a2, const uint64_t* d_b2, size_t a_items, size_t b_items, uint32_t flags, void* stream) {
    static const char* what = "dpfhe_ct_mul_outer";
    // what the arguments alone decide comes before the context is looked at: a caller without a device learns of it too (tests/test_mul_outer_cabi_cpu.py)
    if (flags & ~(DPFHE_IN_NTT | DPFHE_OUT_NTT | DPFHE_OUTER_CAUSAL)) return fail(DPFHE_INVALID_ARGUMENT, what, "unknown flag");
    const bool causal = (flags & DPFHE_OUTER_CAUSAL) != 0;
    if (causal && a_items != b_items) return fail(DPFHE_INVALID_ARGUMENT, what, "the causal form needs a_items == b_items");
    if (a_items > kMaxGrid || b_items > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, what, "a_items * b_items too large for one launch");
    const bool nothing = a_items == 0 || b_items == 0;
    if (!nothing && (!d_out3 || !d_a2 || !d_b2 || misaligned(d_out3) || misaligned(d_a2) || misaligned(d_b2)))
        return fail(DPFHE_INVALID_ARGUMENT, what, "null or misaligned buffer");
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    if (nothing) return DPFHE_SUCCESS;
    const size_t L = c->n_limbs, n = (size_t)1 << c->log2n, poly = L * n;
    // sizes first (a product that wraps size_t would pass the overlap test): every count below stays under 2^31 residue polynomials
    if (a_items * b_items > kMaxGrid / (3 * L) || MulOuterMap::grid(a_items, L, n) > kMaxGrid ||
        !ntt_grid_fits(c, a_items * b_items * 3 * L) || !ntt_grid_fits(c, a_items * 2 * L) || !ntt_grid_fits(c, b_items * 2 * L))
        return fail(DPFHE_INVALID_ARGUMENT, what, "a_items * b_items too large for one launch");
    const size_t out_words = (causal ? a_items * (a_items + 1) / 2 : a_items * b_items) * 3 * poly;
    if (overlaps(d_out3, out_words, d_a2, a_items * 2 * poly) || overlaps(d_out3, out_words, d_b2, b_items * 2 * poly))
        return fail(DPFHE_INVALID_ARGUMENT, what, "output overlaps an operand");
    DPFHE_ON_DEVICE(c, what);
    MulOuterCall k{c, flags, static_cast<hipStream_t>(stream), b_items, causal};
    return ct_mul_outer_composed(k, d_out3, d_a2, d_b2, a_items, b_items);
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
