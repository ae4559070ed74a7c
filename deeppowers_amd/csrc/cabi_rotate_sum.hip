// cabi_rotate_sum.hip - the C ABI's hoisted slot sums: the sum of R rotations of every item under ONE digit lift (kernels_rotate_sum.h), on one-prime keys and
// on grouped-digit keys.  The digit lifts, the transforms and the divisions by P are borrowed from their own units (cabi.h), which also lists the other units and
// states the ABI's conventions.
#include "cabi.h"
#include "kernels_rotate_sum.h"

// out_t = ct_t + round(INTT(S_t) / P),  S_t = the sum of blocks 1 .. R of dpfhe_rotate_hoisted_qp.  Four stages:
//   1. the input transform, digit lift and digit transforms of dpfhe_rotate_hoisted_qp (its steps 1 and 2; block 0 = P ct is an exact multiple of P and
//      enters as the addend of stage 4 instead, never passing through Q P);
//   2. hoisted_qp_sum_kernel: every item's R rotated key products summed in registers, ONE Q P block per item;
//   3. one batched inverse transform of n_items * 2 * L rows, in place;
//   4. the division by P with the input as the addend of both components (rescale_kernel: the words of dpfhe_rescale_bsgs with one addend).
extern "C" int dpfhe_rotate_sum_hoisted(dpfhe_ctx* c, uint64_t* d_out2, const uint64_t* d_in2, size_t n_items, const uint32_t* galois_elts, const uint64_t* d_keys,
                                        size_t n_rot, uint64_t* d_in_ntt, uint64_t* d_digits, uint64_t* d_sum_qp, void* stream) {
    const char* what = "dpfhe_rotate_sum_hoisted";
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    if (int rc = check_extended(c, what)) return rc;
    // (a sum cannot be sliced across launches without re-reading its accumulators: one launch's worth of elements)
    if (n_rot == 0 || n_rot > (size_t)kMaxGaloisBatch) return fail(DPFHE_INVALID_ARGUMENT, what, "n_rot must be in [1, 64]");
    if (n_items == 0) return DPFHE_SUCCESS;
    if (!d_out2 || !d_in2 || !galois_elts || !d_keys || !d_in_ntt || !d_digits || !d_sum_qp || misaligned(d_out2) || misaligned(d_in2) || misaligned(d_keys) ||
        misaligned(d_in_ntt) || misaligned(d_digits) || misaligned(d_sum_qp))
        return fail(DPFHE_INVALID_ARGUMENT, what, "null or misaligned buffer");
    if (int rc = check_galois_elts(c, galois_elts, n_rot, what)) return rc;
    const size_t L = c->n_limbs, Ld = L - 1, T = n_items;
    const int n = 1 << c->log2n;
    const size_t ct_words = T * 2 * Ld * (size_t)n, qp_words = T * 2 * L * (size_t)n, dig_words = T * Ld * L * (size_t)n, key_words = Ld * 2 * L * (size_t)n;
    const uint64_t* bufs[] = {d_out2, d_in2, d_in_ntt, d_digits, d_sum_qp, d_keys};
    const size_t sizes[] = {ct_words, ct_words, ct_words, dig_words, qp_words, n_rot * key_words};
    for (int a = 0; a < 6; ++a)
        for (int b = a + 1; b < 6; ++b)
            if ((a != 1 || b != 5) && overlaps(bufs[a], sizes[a], bufs[b], sizes[b]))   // (the input and the keys are only read)
                return fail(DPFHE_INVALID_ARGUMENT, what, "buffers must not overlap");
    const int chunks = chunks_of(n);
    const QpSumPlan plan = QpSumMap::plan((int)c->log2n, L, T);
    if (T > 0xffffffffu || plan.grid > kMaxGrid || T * Ld * L * (size_t)chunks > kMaxGrid || T * 2 * Ld * (size_t)chunks > kMaxGrid || !ntt_grid_fits(c, T * Ld * L) ||
        !ntt_grid_fits(c, T * 2 * L))
        return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DPFHE_ON_DEVICE(c, what);
    // 1. NTT of the inputs on the data limbs, and the digits of every item's c1, lifted to every limb and transformed.  Only c0's transform is read: the batched
    //    transform takes contiguous items and c0, c1 alternate in d_in2, so c0 alone would be one launch per item; c1 rides along in the one launch (Ld of the
    //    stage's Ld (L + 2) forward transforms), and d_in_ntt keeps dpfhe_rotate_hoisted_qp's layout.
    if (int e = ntt_launch_items(c, false, d_in_ntt, d_in2, T * 2, Ld, s)) return e;
    launch_lift_digits(c, T * Ld * L * (size_t)chunks, s, d_digits, d_in2 + Ld * (size_t)n, 2 * Ld * (size_t)n, chunks);
    if (int e = check_launch("lift_digits kernel launch")) return e;
    if (int e = ntt_launch_items(c, false, d_digits, d_digits, T * Ld, 0, s)) return e;   // (per limb class where the context has them)
    // 2. the sum of the rotated key products, one Q P block per item
    QpSumElts ge{};
    for (size_t i = 0; i < n_rot; ++i) ge.v[i] = galois_elts[i];
    with_ctx_arith(c, [&](auto arith) {
        hipLaunchKernelGGL((hoisted_qp_sum_kernel<decltype(arith)>), dim3((unsigned)plan.grid), dim3(256), 0, s, d_sum_qp, d_digits, d_in_ntt, d_keys, key_words, ge, (unsigned)n_rot,
                           (unsigned)T, plan.tiles, c->p_special, c->lc, (int)L, (int)c->log2n);
    });
    if (int e = check_launch("hoisted_qp_sum kernel launch")) return e;
    // 3. back to the coefficient domain, in place
    if (int e = ntt_launch(c, true, d_sum_qp, d_sum_qp, T * 2 * L, s)) return e;
    // 4. / P, + the input
    launch_rescale(c, T * 2 * Ld * (size_t)chunks, s, d_out2, d_sum_qp, d_in2, 2, 3);
    return check_launch("rescale kernel launch");
}

// The same sum on GROUPED-digit keys (alpha special primes, beta = ceil(Ld / alpha) digit groups): out_t = ct_t + round(INTT(S_t) / P).  Five stages:
//   1. the input transform on the data limbs (as above: c0's is read, c1's rides along);
//   2. digit_group_lift_kernel on every item's c1 (component 1 of 2), one launch for all items and groups, and the digits' transforms: n_items beta items of L rows;
//   3. hoisted_qp_sum_grouped_kernel: R (beta + 1) terms per output word of a data limb, R beta on a special limb, ONE Q P block per item;
//   4. one batched inverse transform of n_items * 2 * L rows, in place;
//   5. grouped_moddown_kernel with both components of the input as the addend.
// The table of (context, alpha) is dpfhe_switch_key_grouped's (grouped_table): whichever entry comes first makes it, n_items == 0 being the warm-up here.
extern "C" int dpfhe_rotate_sum_hoisted_grouped(dpfhe_ctx* c, uint64_t* d_out2, const uint64_t* d_in2, size_t n_items, uint32_t n_special, const uint32_t* galois_elts,
                                                const uint64_t* d_keys, size_t n_rot, uint64_t* d_in_ntt, uint64_t* d_digits, uint64_t* d_sum_qp, void* stream) {
    const char* what = "dpfhe_rotate_sum_hoisted_grouped";
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    const uint32_t L32 = c->n_limbs, alpha = n_special;
    if (alpha == 0 || alpha > (uint32_t)kBxMaxSrc || alpha >= L32) return fail(DPFHE_INVALID_ARGUMENT, what, "n_special must be in [1, 10] and leave a data limb");
    if (L32 > (uint32_t)kBxMaxDst) return fail(DPFHE_INVALID_ARGUMENT, what, "at most 20 limbs (the limit of dpfhe_base_extend)");
    if (n_rot == 0 || n_rot > (size_t)kMaxGaloisBatch) return fail(DPFHE_INVALID_ARGUMENT, what, "n_rot must be in [1, 64]");
    const size_t L = L32, Ld = L - alpha, beta = (Ld + alpha - 1) / alpha, T = n_items;
    const bool made = c->grouped_tabs[alpha].load(std::memory_order_acquire) != nullptr;
    if (T == 0) return made ? (int)DPFHE_SUCCESS : grouped_table(c, alpha, (unsigned)beta, what);   // (the warm-up)
    if (!d_out2 || !d_in2 || !galois_elts || !d_keys || !d_in_ntt || !d_digits || !d_sum_qp || misaligned(d_out2) || misaligned(d_in2) || misaligned(d_keys) ||
        misaligned(d_in_ntt) || misaligned(d_digits) || misaligned(d_sum_qp))
        return fail(DPFHE_INVALID_ARGUMENT, what, "null or misaligned buffer");
    if (int rc = check_galois_elts(c, galois_elts, n_rot, what)) return rc;
    const size_t n = (size_t)1 << c->log2n;
    const int chunks = chunks_of(n);
    const QpSumPlan plan = QpSumMap::plan((int)c->log2n, L, T <= 0xffffffffu ? T : 0xffffffffu);
    const GroupedKsPlan gplan = GroupedKsMap::plan(T, (unsigned)L, alpha, n);
    if (T > 0xffffffffu || plan.grid > kMaxGrid || !gplan.ok || !ntt_grid_fits(c, T * beta * L) || !ntt_grid_fits(c, T * 2 * L))
        return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    const size_t ct_words = T * 2 * Ld * n, qp_words = T * 2 * L * n, dig_words = T * beta * L * n, key_words = beta * 2 * L * n;
    {
        const uint64_t* bufs[] = {d_out2, d_in2, d_in_ntt, d_digits, d_sum_qp, d_keys};
        const size_t sizes[] = {ct_words, ct_words, ct_words, dig_words, qp_words, n_rot * key_words};
        for (int a = 0; a < 6; ++a)
            for (int b = a + 1; b < 6; ++b)
                if ((a != 1 || b != 5) && overlaps(bufs[a], sizes[a], bufs[b], sizes[b]))   // (the input and the keys are only read)
                    return fail(DPFHE_INVALID_ARGUMENT, what, "buffers must not overlap");
    }
    if (!made)
        if (int rc = grouped_table(c, alpha, (unsigned)beta, what)) return rc;
    const BaseExtArgs* tabs = static_cast<const BaseExtArgs*>(c->grouped_tabs[alpha].load(std::memory_order_acquire));
    hipStream_t s = static_cast<hipStream_t>(stream);
    DPFHE_ON_DEVICE(c, what);
    // 1. NTT of the inputs on the data limbs;  2. the centred digit of every group of every item's c1 on every limb of Q P, transformed
    if (int e = ntt_launch_items(c, false, d_in_ntt, d_in2, T * 2, Ld, s)) return e;
    launch_grouped(alpha, true, gplan, s, d_digits, d_in2, nullptr, 2, 0, tabs, c, (int)Ld, chunks);
    if (int e = check_launch("digit group lift kernel launch")) return e;
    if (int e = ntt_launch_items(c, false, d_digits, d_digits, T * beta, 0, s)) return e;
    // 3. the sum of the rotated key products, one Q P block per item
    QpSumElts ge{};
    for (size_t i = 0; i < n_rot; ++i) ge.v[i] = galois_elts[i];
    with_ctx_arith(c, [&](auto arith) {
        hipLaunchKernelGGL((hoisted_qp_sum_grouped_kernel<decltype(arith)>), dim3((unsigned)plan.grid), dim3(256), 0, s, d_sum_qp, d_digits, d_in_ntt, d_keys, key_words, ge,
                           (unsigned)n_rot, (unsigned)T, plan.tiles, tabs + beta, c->lc, (int)L, (int)beta, (int)Ld, (int)c->log2n);
    });
    if (int e = check_launch("hoisted_qp_sum_grouped kernel launch")) return e;
    // 4. back to the coefficient domain, in place;  5. / P, + the input
    if (int e = ntt_launch(c, true, d_sum_qp, d_sum_qp, T * 2 * L, s)) return e;
    launch_grouped(alpha, false, gplan, s, d_out2, d_sum_qp, d_in2, 2, 3, tabs, c, (int)Ld, chunks);
    return check_launch("grouped division launch");
}
