// cabi_poly.hip - polynomial arithmetic entries of include/dpfhe.h: the batched transforms, the coefficient-wise operations, the copy.
#include "cabi.h"
#include "kernels_poly.h"

// batched transform of `items` RNS polynomials over the first `limbs_used` limbs (limbs_used = 0: all); arguments validated, device selected by the caller
int ntt_launch_items(dpfhe_ctx* c, bool inverse, uint64_t* out, const uint64_t* in, size_t items, size_t limbs_used, hipStream_t s) {
    const size_t Lu = limbs_used ? limbs_used : c->n_limbs;
    int rc;
    if (c->classes) {
        // several classes among these limbs: one launch, the class branch inside the kernel.  One class only: that class's own kernel (the merged
        // kernel carries the register budget of its widest arm: measured 62 against 69 % of HBM peak on an all-f64 context)
        bool several = false;
        for (size_t l = 1; l < Lu; ++l) several = several || c->limb_cls[l] != c->limb_cls[0];
        rc = 1;
        if (several) {
            MixedTables mt = c->mixed;
            mt.n_limbs = (int)Lu;
            rc = launch_ntt_classes((int)c->log2n, inverse, out, in, items * Lu, mt, s);
        }
        if (rc == 1)                                                                   // (one class, or a geometry without the merged kernel)
            rc = for_each_class(c, Lu, [&](const auto& tb) { return launch_ntt((int)c->log2n, inverse, out, in, items * (size_t)tb.n_active, tb, s); });
    } else {
        rc = with_ctx_arith(c, [&](auto arith) {
            DevTables<decltype(arith)> td = tables_of<decltype(arith)>(c); td.n_limbs = (int)Lu;
            return launch_ntt((int)c->log2n, inverse, out, in, items * Lu, td, s);
        });
    }
    if (rc) return fail(DPFHE_INVALID_STATE, "ntt", "no kernel geometry for this log2_n");
    return check_launch("ntt kernel launch");
}

static int ntt_entry(dpfhe_ctx* c, bool inverse, uint64_t* out, const uint64_t* in, size_t n_rns_polys, void* stream) {
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, "ntt", "null context");
    if (n_rns_polys == 0) return DPFHE_SUCCESS;
    if (!out || !in || misaligned(out) || misaligned(in)) return fail(DPFHE_INVALID_ARGUMENT, "ntt", "null or misaligned buffer");
    const size_t npolys = n_rns_polys * c->n_limbs;
    if (!ntt_grid_fits(c, npolys)) return fail(DPFHE_INVALID_ARGUMENT, "ntt", "batch too large for one launch");
    DPFHE_ON_DEVICE(c, "ntt");
    return ntt_launch(c, inverse, out, in, npolys, static_cast<hipStream_t>(stream));
}

extern "C" int dpfhe_ntt_fwd(dpfhe_ctx* c, uint64_t* d_io, size_t n, void* s) { return ntt_entry(c, false, d_io, d_io, n, s); }
extern "C" int dpfhe_ntt_inv(dpfhe_ctx* c, uint64_t* d_io, size_t n, void* s) { return ntt_entry(c, true, d_io, d_io, n, s); }
extern "C" int dpfhe_ntt_fwd_oop(dpfhe_ctx* c, uint64_t* o, const uint64_t* i, size_t n, void* s) { return ntt_entry(c, false, o, i, n, s); }
extern "C" int dpfhe_ntt_inv_oop(dpfhe_ctx* c, uint64_t* o, const uint64_t* i, size_t n, void* s) { return ntt_entry(c, true, o, i, n, s); }

// ------------------------------------------------------------------------------------------------
template <int OP>
static void launch_dy(const dpfhe_ctx* c, u64* out, const u64* a, const u64* b, size_t npolys, hipStream_t s, int b_period) {
    // distinct streams of the launch: a, b (unless broadcast or the same buffer), the result (unless in place; read as well by mul_add)
    const int streams = 1 + ((OP != DY_NEG && !b_period && b != a) ? 1 : 0) + ((out != a && out != b) ? 1 : 0);
    const bool nt = (npolys << c->log2n) * sizeof(u64) * (size_t)streams > kInfinityCacheBytes;   // cannot stay in the Infinity Cache
    with_ctx_arith(c, [&](auto arith) {
        typedef decltype(arith) Arith;
        if (nt) hipLaunchKernelGGL((dyadic_kernel<Arith, OP, true>), dim3((unsigned)npolys), dim3(256), 0, s, out, a, b, c->lc, (int)c->n_limbs, 1 << c->log2n, b_period);
        else hipLaunchKernelGGL((dyadic_kernel<Arith, OP, false>), dim3((unsigned)npolys), dim3(256), 0, s, out, a, b, c->lc, (int)c->n_limbs, 1 << c->log2n, b_period);
    });
}

int launch_dyadic(const dpfhe_ctx* c, int op, u64* out, const u64* a, const u64* b, size_t npolys, hipStream_t s, int b_period) {
    switch (op) {
        case DY_MUL: launch_dy<DY_MUL>(c, out, a, b, npolys, s, b_period); return 0;
        case DY_MUL_ADD: launch_dy<DY_MUL_ADD>(c, out, a, b, npolys, s, b_period); return 0;
        case DY_ADD: launch_dy<DY_ADD>(c, out, a, b, npolys, s, b_period); return 0;
        case DY_SUB: launch_dy<DY_SUB>(c, out, a, b, npolys, s, b_period); return 0;
        case DY_NEG: launch_dy<DY_NEG>(c, out, a, b, npolys, s, b_period); return 0;
        default: return -1;
    }
}

static int dyadic_entry(dpfhe_ctx* c, int op, uint64_t* out, const uint64_t* a, const uint64_t* b, size_t n_rns_polys, void* stream, bool broadcast_b = false) {
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, "dyadic", "null context");
    if (n_rns_polys == 0) return DPFHE_SUCCESS;
    if (!out || !a || (op != DY_NEG && !b) || misaligned(out) || misaligned(a) || misaligned(b))
        return fail(DPFHE_INVALID_ARGUMENT, "dyadic", "null or misaligned buffer");
    const size_t npolys = n_rns_polys * c->n_limbs;
    if (npolys > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, "dyadic", "batch too large for one launch");
    DPFHE_ON_DEVICE(c, "dyadic");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (op == DY_NEG) b = a;
    const int b_period = broadcast_b ? (int)c->n_limbs : 0;
    if (launch_dyadic(c, op, out, a, b, npolys, s, b_period)) return fail(DPFHE_INVALID_ARGUMENT, "dyadic", "bad op");
    return check_launch("dyadic kernel launch");
}

extern "C" int dpfhe_dyadic_mul(dpfhe_ctx* c, uint64_t* o, const uint64_t* a, const uint64_t* b, size_t n, void* s) { return dyadic_entry(c, DY_MUL, o, a, b, n, s); }
extern "C" int dpfhe_dyadic_mul_add(dpfhe_ctx* c, uint64_t* acc, const uint64_t* a, const uint64_t* b, size_t n, void* s) { return dyadic_entry(c, DY_MUL_ADD, acc, a, b, n, s); }
extern "C" int dpfhe_add(dpfhe_ctx* c, uint64_t* o, const uint64_t* a, const uint64_t* b, size_t n, void* s) { return dyadic_entry(c, DY_ADD, o, a, b, n, s); }
extern "C" int dpfhe_sub(dpfhe_ctx* c, uint64_t* o, const uint64_t* a, const uint64_t* b, size_t n, void* s) { return dyadic_entry(c, DY_SUB, o, a, b, n, s); }
extern "C" int dpfhe_negate(dpfhe_ctx* c, uint64_t* o, const uint64_t* a, size_t n, void* s) { return dyadic_entry(c, DY_NEG, o, a, nullptr, n, s); }
// A7: every residue polynomial of a times ONE plaintext (an RNS polynomial of L limbs), one launch for the whole batch
extern "C" int dpfhe_multiply_plain(dpfhe_ctx* c, uint64_t* o, const uint64_t* a, const uint64_t* pt, size_t n, void* s) { return dyadic_entry(c, DY_MUL, o, a, pt, n, s, true); }

extern "C" int dpfhe_copy(dpfhe_ctx* c, uint64_t* d_dst, const uint64_t* d_src, size_t n_words, void* stream) {
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_copy", "null context");
    if (n_words == 0) return DPFHE_SUCCESS;
    if (!d_dst || !d_src || misaligned(d_dst) || misaligned(d_src) || (n_words & 1)) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_copy", "null or misaligned buffer, or an odd word count");
    if (overlaps(d_dst, n_words, d_src, n_words)) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_copy", "buffers overlap");
    const size_t n_vec = n_words / 2, blocks = (n_vec + 2047) / 2048;
    if (blocks > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_copy", "too many words for one launch");
    DPFHE_ON_DEVICE(c, "dpfhe_copy");
    // streams that cannot live in the 256 MiB Infinity Cache (source + destination) go around it
    if (n_words * 16 > kInfinityCacheBytes)
        hipLaunchKernelGGL(copy_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), reinterpret_cast<U64x2*>(d_dst),
                           reinterpret_cast<const U64x2*>(d_src), n_vec);
    else
        hipLaunchKernelGGL(copy_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), reinterpret_cast<U64x2*>(d_dst),
                           reinterpret_cast<const U64x2*>(d_src), n_vec);
    return check_launch("copy kernel launch");
}
