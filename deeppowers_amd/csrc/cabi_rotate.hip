// cabi_rotate.hip - the C ABI's rotations: Galois automorphisms, batched and hoisted rotations and the rotate-and-add ladder under hybrid keys (kernels_rotate.h; the fused
// hoisted key switch and the inverse transform with a built-in automorphism are kernels.h's, through launch.h).  The key switch behind a rotation,
// its digit lift and its division by P are cabi_keyswitch.hip's (cabi.h).  cabi.h lists the other units and states the ABI's conventions.
#include "cabi.h"
#include "kernels_rotate.h"

// automorphism launch: polynomials up to 64 KiB are staged through LDS, larger ones gathered from global memory
static void launch_galois_multi(hipStream_t s, unsigned grid, u64* out, const u64* in, size_t in_item_stride, const LimbConst* lc, int n_limbs, int n,
                                int polys_per_item, const GaloisInvs& inv, unsigned in_mod, unsigned item0, size_t out_item_stride = 0) {
    if (!out_item_stride) out_item_stride = (size_t)polys_per_item * n;   // output items back to back
    if (n <= 8192)
        hipLaunchKernelGGL(galois_multi_kernel<true>, dim3(grid), dim3(256), (size_t)n * 8, s, out, in, in_item_stride, lc, n_limbs, n, polys_per_item, inv, in_mod, item0, out_item_stride);
    else
        hipLaunchKernelGGL(galois_multi_kernel<false>, dim3(grid), dim3(256), 0, s, out, in, in_item_stride, lc, n_limbs, n, polys_per_item, inv, in_mod, item0, out_item_stride);
}

// the inverses of `cnt` output items' elements from `first` on, `div` consecutive items sharing an element: what galois_multi_kernel takes
static GaloisInvs galois_inverses(const uint32_t* galois_elts, size_t first, size_t cnt, size_t div, unsigned two_n) {
    GaloisInvs inv{};
    for (size_t i = 0; i < cnt; ++i) inv.v[i] = galois_inverse(galois_elts[(first + i) / div], two_n);
    return inv;
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
        const GaloisInvs inv = galois_inverses(galois_elts, first, cnt, group, two_n);
        const uint64_t* src = d_in2 + (n_in == 1 ? 0 : first * ct_words);
        launch_galois_multi(s, (unsigned)(cnt * 2 * Ld), d_rotated + first * ct_words, src, n_in == 1 ? (size_t)0 : ct_words, c->lc, (int)Ld, n, (int)(2 * Ld), inv, 0u, 0u);
        return check_launch("galois kernel launch");
    });
    if (rc) return rc;
    return key_switch_hybrid(c, what, 2, d_out2, d_rotated, d_keys, d_work, batch, stream, key_words, (unsigned)group);
}

extern "C" int dpfhe_rotate_hybrid_batch(dpfhe_ctx* c, uint64_t* d_out2, const uint64_t* d_in2, size_t n_in, const uint32_t* galois_elts,
                                         const uint64_t* d_keys, uint64_t* d_work, uint64_t* d_rotated, size_t batch, void* stream) {
    return rotate_batch_impl(c, "dpfhe_rotate_hybrid_batch", d_out2, d_in2, n_in, galois_elts, batch, 1, d_keys, d_work, d_rotated, batch, stream);
}

extern "C" int dpfhe_rotate_hybrid_grouped(dpfhe_ctx* c, uint64_t* d_out2, const uint64_t* d_in2, const uint32_t* galois_elts, size_t n_elts, size_t group,
                                           const uint64_t* d_keys, uint64_t* d_work, uint64_t* d_rotated, void* stream) {
    return rotate_batch_impl(c, "dpfhe_rotate_hybrid_grouped", d_out2, d_in2, n_elts * group, galois_elts, n_elts, group, d_keys, d_work, d_rotated, n_elts * group, stream);
}

// The rotate-and-add ladder: acc <- acc + rotate(acc, g_e) for e < n_steps, every item of a step under that step's element and key.  Three launches per step:
//   1. sigma_g(c1) of every item - into the c1 slots of the step's OUTPUT buffer, which nothing reads until pass 3 overwrites it: there the fused key switch
//      finds its digits at the two-component item stride it reads (kernels.h relin_kernel MODE 3), and no buffer of its own is needed;
//   2. the key products of those words over Q P (cabi_keyswitch.hip key_products_hybrid: fused up to N = 8192, composed above);
//   3. rotate_add_pass_kernel: / P, + the step's input, + sigma_g(c0) gathered in the pass.
// The steps ping-pong between d_out2 and d_acc so that the last one lands in d_out2; step 0 reads d_in2.
extern "C" int dpfhe_rotate_add_hybrid(dpfhe_ctx* c, uint64_t* d_out2, const uint64_t* d_in2, const uint32_t* galois_elts, const uint64_t* d_keys, uint64_t* d_work,
                                       uint64_t* d_acc, size_t n_steps, size_t batch, void* stream) {
    const char* what = "dpfhe_rotate_add_hybrid";
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    if (int rc = check_extended(c, what)) return rc;
    if (n_steps == 0) return fail(DPFHE_INVALID_ARGUMENT, what, "n_steps must be positive");
    if (batch == 0) return DPFHE_SUCCESS;
    if (n_steps == 1) d_acc = nullptr;   // not used
    if (!d_out2 || !d_in2 || !galois_elts || !d_keys || !d_work || (n_steps > 1 && !d_acc) || misaligned(d_out2) || misaligned(d_in2) || misaligned(d_keys) ||
        misaligned(d_work) || misaligned(d_acc))
        return fail(DPFHE_INVALID_ARGUMENT, what, "null or misaligned buffer");
    if (int rc = check_galois_elts(c, galois_elts, n_steps, what)) return rc;
    const size_t L = c->n_limbs, Ld = L - 1;
    const int n = 1 << c->log2n;
    const unsigned two_n = 2u << c->log2n;
    const size_t ct_words = 2 * Ld * (size_t)n, key_words = Ld * 2 * L * (size_t)n, io_words = batch * ct_words, work_words = batch * 2 * L * n,
                 acc_words = d_acc ? io_words : 0;
    if (overlaps(d_out2, io_words, d_in2, io_words) || overlaps(d_work, work_words, d_in2, io_words) || overlaps(d_work, work_words, d_out2, io_words) ||
        overlaps(d_acc, acc_words, d_in2, io_words) || overlaps(d_acc, acc_words, d_out2, io_words) || overlaps(d_acc, acc_words, d_work, work_words))
        return fail(DPFHE_INVALID_ARGUMENT, what, "buffers must not overlap");
    const unsigned slices = RotateAddMap::slices((size_t)n);
    const size_t pass_grid = RotateAddMap::grid(batch * Ld, slices);
    if (batch * Ld > kMaxGrid || pass_grid > kMaxGrid || !key_products_fit(c, batch, key_words, (unsigned)batch) || batch > 0xffffffffu)
        return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DPFHE_ON_DEVICE(c, what);
    const uint64_t* cur = d_in2;
    for (size_t e = 0; e < n_steps; ++e) {
        uint64_t* dst = ((n_steps - 1 - e) & 1) ? d_acc : d_out2;
        if (int rc = for_slices(batch, kMaxGaloisBatch, [&](size_t first, size_t cnt) {   // the elements travel as kernel arguments, 64 at a time
                const GaloisInvs inv = galois_inverses(galois_elts + e, first, cnt, batch, two_n);
                launch_galois_multi(s, (unsigned)(cnt * Ld), dst + first * ct_words + Ld * (size_t)n, cur + first * ct_words + Ld * (size_t)n, ct_words, c->lc, (int)Ld, n, (int)Ld,
                                    inv, 0u, 0u, ct_words);
                return check_launch("galois kernel launch");
            }))
            return rc;
        if (int rc = key_products_hybrid(c, what, 2, d_work, dst, d_keys + e * key_words, batch, s, key_words, (unsigned)batch)) return rc;
        const unsigned g_inv = galois_inverse(galois_elts[e], two_n);
        with_ctx_arith(c, [&](auto arith) {
            if (RotateAddMap::staged((size_t)n))
                hipLaunchKernelGGL((rotate_add_pass_kernel<decltype(arith), true>), dim3((unsigned)pass_grid), dim3(256), (size_t)n * 8, s, dst, d_work, cur, c->lc, c->d_rescale,
                                   (int)L, n, slices, batch * Ld, g_inv);
            else
                hipLaunchKernelGGL((rotate_add_pass_kernel<decltype(arith), false>), dim3((unsigned)pass_grid), dim3(256), 0, s, dst, d_work, cur, c->lc, c->d_rescale, (int)L, n,
                                   slices, batch * Ld, g_inv);
        });
        if (int rc = check_launch("rotate-add pass launch")) return rc;
        cur = dst;
    }
    return DPFHE_SUCCESS;
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
    // 4. the rotations: permuted digit segments x key segments as a stream (kernels_rotate.h hoisted_qp_stream_kernel), 64 rotations per launch
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
        const GaloisInvs inv = galois_inverses(galois_elts, first, cnt, T, two_n);
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
            const int rc = with_ctx_arith(c, [&](auto arith) {
                return launch_ntt_inv_galois_split((int)c->log2n, d_out + off, mid, d_in + off, galois_elts + first, cnt, per_elt, tables_of<decltype(arith)>(c), s);
            });
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
