// cabi_rotate_matvec.hip - the C ABI's fused first two stages of a packed layer: the hoisted baby steps multiplied by their pre-rotated diagonals and summed,
// no Q P block per rotation in between (rotate_matvec.h).  The digit lift and the transforms are borrowed from their own units (cabi.h), which also lists the
// other units and states the ABI's conventions.
#include "cabi.h"
#include "rotate_matvec.h"

// y = dpfhe_matvec_plain_multi(W, dpfhe_rotate_hoisted_qp(in)), word for word.  Two stages:
//   1. the input transform, digit lift and digit transforms of dpfhe_rotate_hoisted_qp (its steps 1 and 2; its step 3, block 0 = P ct, is formed in stage 2);
//   2. hoisted_qp_matvec_kernel: every rotated key product formed in registers and multiplied into a tile of rows.
extern "C" int dpfhe_rotate_matvec_hoisted_qp(dpfhe_ctx* c, uint64_t* d_y_qp, const uint64_t* d_W, const uint64_t* d_in2, size_t n_items, const uint32_t* galois_elts,
                                              const uint64_t* d_keys, size_t batch, size_t rows, uint64_t* d_in_ntt, uint64_t* d_digits, void* stream) {
    const char* what = "dpfhe_rotate_matvec_hoisted_qp";
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    if (int rc = check_extended(c, what)) return rc;
    // (the accumulators of a row are never re-read: one launch's worth of elements)
    if (batch == 0 || batch > (size_t)kMaxGaloisBatch) return fail(DPFHE_INVALID_ARGUMENT, what, "batch must be in [1, 64]");
    if (rows == 0 || rows > kRotMatvecMaxRows) return fail(DPFHE_INVALID_ARGUMENT, what, "rows must be in [1, 65536]");
    if (n_items == 0) return DPFHE_SUCCESS;
    if (!d_y_qp || !d_W || !d_in2 || !galois_elts || !d_keys || !d_in_ntt || !d_digits || misaligned(d_y_qp) || misaligned(d_W) || misaligned(d_in2) ||
        misaligned(d_keys) || misaligned(d_in_ntt) || misaligned(d_digits))
        return fail(DPFHE_INVALID_ARGUMENT, what, "null or misaligned buffer");
    if (int rc = check_galois_elts(c, galois_elts, batch, what)) return rc;
    const size_t L = c->n_limbs, Ld = L - 1, T = n_items;
    const int n = 1 << c->log2n;
    const size_t ct_words = T * 2 * Ld * (size_t)n, y_words = rows * T * 2 * L * (size_t)n, dig_words = T * Ld * L * (size_t)n, key_words = Ld * 2 * L * (size_t)n,
                 w_words = rows * (batch + 1) * L * (size_t)n;
    const uint64_t* bufs[] = {d_y_qp, d_in_ntt, d_digits, d_in2, d_W, d_keys};   // the first three are written
    const size_t sizes[] = {y_words, ct_words, dig_words, ct_words, w_words, batch * key_words};
    for (int a = 0; a < 3; ++a)
        for (int b = a + 1; b < 6; ++b)
            if (overlaps(bufs[a], sizes[a], bufs[b], sizes[b])) return fail(DPFHE_INVALID_ARGUMENT, what, "buffers must not overlap");
    const int chunks = chunks_of(n);
    const RotMatvecPlan plan = RotMatvecMap::plan((int)c->log2n, L, T, rows);
    if (T > 0xffffffffu || plan.grid > kMaxGrid || T * Ld * L * (size_t)chunks > kMaxGrid || T * 2 * Ld * (size_t)chunks > kMaxGrid || !ntt_grid_fits(c, T * Ld * L) ||
        !ntt_grid_fits(c, T * 2 * L))
        return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    hipStream_t s = static_cast<hipStream_t>(stream);
    DPFHE_ON_DEVICE(c, what);
    // 1. NTT of the inputs on the data limbs, and the digits of every item's c1, lifted to every limb and transformed
    if (int e = ntt_launch_items(c, false, d_in_ntt, d_in2, T * 2, Ld, s)) return e;
    launch_lift_digits(c, T * Ld * L * (size_t)chunks, s, d_digits, d_in2 + Ld * (size_t)n, 2 * Ld * (size_t)n, chunks);
    if (int e = check_launch("lift_digits kernel launch")) return e;
    if (int e = ntt_launch_items(c, false, d_digits, d_digits, T * Ld, 0, s)) return e;   // (per limb class where the context has them)
    // 2. the weighted sums of block 0 and the rotated key products, rows x items x 2 polynomials over Q P
    RotMatvecElts ge{};
    for (size_t i = 0; i < batch; ++i) ge.v[i] = galois_elts[i];
    with_ctx_arith(c, [&](auto arith) {
        hipLaunchKernelGGL((hoisted_qp_matvec_kernel<decltype(arith)>), dim3((unsigned)plan.grid), dim3(256), 0, s, d_y_qp, d_W, d_digits, d_in_ntt, d_keys, key_words, ge,
                           (unsigned)batch, (unsigned)T, (unsigned)rows, plan.row_tiles, c->p_special, c->lc, (int)L, (int)c->log2n);
    });
    return check_launch("hoisted_qp_matvec kernel launch");
}
