// cabi_linalg.hip - the C ABI's linear algebra: ciphertext x plaintext matrix-vector products and shard-local sums (kernels_linalg.h).
// cabi.h lists the other units and states the ABI's conventions.
#include "cabi.h"
#include "kernels_linalg.h"

// words per thread of the FoldArith matvec kernels: 2 right-hand-side polynomials per workgroup / 4 (kernels_linalg.h matvec_fold_kernel)
constexpr int kMatvecWpt2 = 2, kMatvecWpt4 = 1;
constexpr int kMatvecWd = 1;     // columns of W lookahead in the multi-right-hand-side product (2 measured no faster: profiles/r04_ab_matvec_full.txt)
constexpr int kMatvecRt4 = 4;    // rows per workgroup of the 4-polynomial (2-token) kernel (8 measured slower)

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
    if (c->fold) {   // column accumulators split at bit 30 (kernels_linalg.h matvec_fold_kernel): 4 multiply-adds per term
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
    const size_t blocks = MatvecMap::grid(c->n_limbs, chunks, (rows + RT - 1) / RT, 1);   // block ids laid out per XCD: kernels_linalg.h matvec_kernel
    if (blocks > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_matvec_plain", "too many rows for one launch");
    hipLaunchKernelGGL((matvec_kernel<ShoupArith, RT>), dim3((unsigned)blocks), dim3(256), 0, s, d_y, d_W, d_x, c->lc, (int)c->n_limbs, n, chunks, rows, cols);
    return check_launch("matvec kernel launch");
}

// One launch of the multi-right-hand-side product: `groups` groups of C / 2 right-hand sides (x / y at xs / ys, the full [n_rhs][2] stride), RT rows and
// 256 WPT words per workgroup, block ids laid out per XCD (kernels_linalg.h).  FOLD: matvec_fold_kernel's split-at-bit-30 column accumulators; otherwise
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
    // the groups of a W tile on the same XCD (kernels_linalg.h), an odd last right-hand side in a second launch.  x / y are
    // [cols | rows][n_rhs][2][L][N]: a group is a strided slice, so the kernels take the full stride.  Measured on the 32 x 32 x
    // 1024-diagonal matvec of a packed GPT-2 layer, per token: 86 us single; 8 tokens: 75 us with one launch per group (W re-read from
    // HBM by every group), see MEASUREMENTS.md for the XCD-grouped launch.
    const size_t pairs = n_rhs / 2;
    const uint64_t* x_last = d_x + (n_rhs - 1) * 2 * poly;   // an odd last right-hand side
    uint64_t* y_last = d_y + (n_rhs - 1) * 2 * poly;
    int rc = DPFHE_SUCCESS;
    if (c->fold) {   // split-at-bit-30 column accumulators (kernels_linalg.h matvec_fold_kernel), same grouping and block-id layout
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
    // (kernels_linalg.h; a second thin workgroup on a CU would not fit the registers either).  Everything else - short batches (latency-bound: no cap),
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
