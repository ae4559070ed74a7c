// k_cencode.hip - complex slot encoding (cencode.h): the device kernels, their launcher, the host twin, the host decoder and the entries of include/dpfhe.h.
//
// N <= 16384: one workgroup of up to 512 lanes per slot vector.  It gathers the n = N / 2 complex slots in transform order (the slot -> position table
// and the conjugation fused into the load) and keeps them in LDS (16 n = 8 N bytes: dynamic up to 64 KiB, a static 128 KiB array at N = 16384), runs the
// levels three at a time (each lane takes groups of 8 complex words through 3 levels in registers, one barrier per pass; the first pass works on the
// gathered words before they reach LDS; Delta / n rides on the last level), then every lane rounds and lifts its pairs of coefficients and writes the
// L limb rows with 16-byte stores.  FP64 vector arithmetic only.
// N = 32768, 65536: the first 12 levels run per 4096-word chunk as above and park their words in row 0 of the item's own output (real parts in the
// low half of the row, imaginary parts in the high half: exactly N doubles); a second kernel takes, per lane, the 4 or 8 complex words 4096 apart of a
// pair of columns through the remaining levels in registers and writes all rows of exactly the positions it read - no scratch and no hazard.
#include <cstring>
#include <new>

#include "cabi.h"
#include "cencode.h"

namespace dpfhe {

constexpr u32 kCencThreads = 256;       // lanes per workgroup of the second kernel
constexpr u32 kCencLdsThreads = 512;    // lanes per slot vector (or chunk) of the LDS kernel
constexpr u32 kCencDynLdsLog = 12;      // complex words in 64 KiB of dynamic LDS
constexpr u32 kCencMaxLdsLog = 13;      // complex words in the static 128 KiB array
constexpr u32 kCencChunkLog = 12;       // chunk of the two-kernel form
// the second kernel's blocks: one lane per pair of columns of a chunk (spelled with % and / in the kernel, as in k_encode.hip)
constexpr ItemChunkPlan cenc_tail_plan(size_t items) { return ItemChunkMap::plan(items, 1u << (kCencChunkLog - 1), kCencThreads); }

// A workgroup per chunk of 2^log2c complex words (workmap.h ItemChunkMap, n >> log2c chunks per item).  WHOLE (log2c == log2 n): the full transform and the
// output; otherwise the first log2c levels of the chunk, parked in row 0 of the item's output.  STATIC: complex words of a static LDS array (0: dynamic).
// The steps between the barriers are cencode.h's cenc_lane_*.
template <bool WHOLE, u32 STATIC>
__global__ __launch_bounds__(kCencLdsThreads) void cencode_lds_kernel(u64* __restrict__ out, const double* __restrict__ slots, const CencodeTables tb, u32 log2c,
                                                                      double scale, u32 real, u32 plain) {
    extern __shared__ __attribute__((aligned(16))) cenc_f64x2 dyn_lds[];
    __shared__ __attribute__((aligned(16))) cenc_f64x2 static_lds[STATIC ? STATIC : 1];
    cenc_f64x2* a = STATIC ? static_lds : dyn_lds;
    const u32 tid = threadIdx.x, T = blockDim.x, log2h = tb.log2n - 1;
    const u32 C = 1u << log2c, chunk = ItemChunkMap::chunk(blockIdx.x, log2h - log2c), base = chunk << log2c;
    const size_t item = ItemChunkMap::outer(blockIdx.x, log2h - log2c);
    cenc_lane_first_pass(a, slots + (item << (real ? log2h : tb.log2n)), real != 0, tid, T, base, C, tb);
    __syncthreads();
    u32 lg0 = kCencRadixLog;
    for (; log2c - lg0 > kCencRadixLog; lg0 += kCencRadixLog) {
        cenc_lane_mid_pass(a, tid, T, base, C, lg0, tb);
        __syncthreads();
    }
    cenc_lane_last_pass<WHOLE>(a, tid, T, base, log2c, lg0, scale, tb);
    __syncthreads();
    cenc_lane_store<WHOLE>(out + item * ((plain ? (size_t)1 : (size_t)tb.n_limbs) << tb.log2n), a, tid, T, base, C, plain != 0, tb);
}

// the last R = log2 n - 12 levels: lane j of an item owns columns 2 j, 2 j + 1 of each of the 2^R chunks
template <int R>
__global__ __launch_bounds__(kCencThreads) void cencode_tail_kernel(u64* __restrict__ out, const CencodeTables tb, double scale, u32 plain) {
    constexpr u32 kBlocksPerItem = 1u << cenc_tail_plan(1).log2_chunks;
    const u32 k = 2 * ItemChunkMap::lane(blockIdx.x % kBlocksPerItem, kCencThreads, threadIdx.x);
    const size_t item = blockIdx.x / kBlocksPerItem;
    cenc_lane_tail<R>(out + item * ((plain ? (size_t)1 : (size_t)tb.n_limbs) << tb.log2n), k, kCencChunkLog, scale, plain != 0, tb);
}

// device: out = the encoding of d_slots ([items][n] (re, im) pairs, or [items][n] doubles when real) at scale Delta = scale_over_n n; plain: [items][N]
// two's-complement words, else [items][L][N] residues.  0, or -1 if the grid is too large.
static int launch_encode_complex(u64* out, const double* slots, size_t items, double scale, bool real, bool plain, const CencodeTables& tb, hipStream_t s) {
    const u32 log2h = tb.log2n - 1;
    const bool whole = log2h <= kCencMaxLdsLog;
    const u32 log2c = whole ? log2h : kCencChunkLog;
    const u32 C = 1u << log2c, threads = (C >> kCencRadixLog) < kCencLdsThreads ? (C >> kCencRadixLog) : kCencLdsThreads;
    const ItemChunkPlan lds = ItemChunkMap::fixed(items, threads, log2h - log2c), tail = cenc_tail_plan(items);
    if (!lds.ok || (!whole && !tail.ok)) return -1;
    const u32 r = real ? 1u : 0u, p = plain ? 1u : 0u;
    if (whole && log2c > kCencDynLdsLog) {
        hipLaunchKernelGGL((cencode_lds_kernel<true, 1u << kCencMaxLdsLog>), dim3((unsigned)lds.grid), dim3(threads), 0, s, out, slots, tb, log2c, scale, r, p);
        return 0;
    }
    if (whole) {
        hipLaunchKernelGGL((cencode_lds_kernel<true, 0>), dim3((unsigned)lds.grid), dim3(threads), C * sizeof(cenc_f64x2), s, out, slots, tb, log2c, scale, r, p);
        return 0;
    }
    hipLaunchKernelGGL((cencode_lds_kernel<false, 0>), dim3((unsigned)lds.grid), dim3(threads), C * sizeof(cenc_f64x2), s, out, slots, tb, log2c, 0.0, r, p);
    if (log2h - kCencChunkLog == 2)
        hipLaunchKernelGGL(cencode_tail_kernel<2>, dim3((unsigned)tail.grid), dim3(kCencThreads), 0, s, out, tb, scale, p);
    else
        hipLaunchKernelGGL(cencode_tail_kernel<3>, dim3((unsigned)tail.grid), dim3(kCencThreads), 0, s, out, tb, scale, p);
    return 0;
}

template <int R>
static void cenc_pass_host(cenc_f64x2* a, u32 lg0, u32 log2h, bool last, const cenc_f64x2* tw, double scale) {
    for (u32 g = 0; g < (1u << (log2h - R)); ++g) {
        if (last) cenc_group_mem<R, true>(a, g, 0, lg0, log2h, tw, scale);
        else cenc_group_mem<R, false>(a, g, 0, lg0, log2h, tw, scale);
    }
}

void encode_complex_host(u64* out, const double* slots, size_t items, double scale, bool real, bool plain, const CencodeTables& tb) {
    const u32 log2h = tb.log2n - 1;
    const size_t n = (size_t)1 << tb.log2n, h = n >> 1;
    std::vector<cenc_f64x2> buf(h);
    cenc_f64x2* a = buf.data();
    for (size_t item = 0; item < items; ++item) {
        const double* v = slots + item * (real ? h : n);
        for (size_t p = 0; p < h; ++p) a[p] = cenc_slot(v, tb.src[p], real);
        u32 lg0 = 0;
        for (; log2h - lg0 > kCencRadixLog; lg0 += kCencRadixLog) cenc_pass_host<3>(a, lg0, log2h, false, tb.tw, scale);
        switch (log2h - lg0) {
        case 1: cenc_pass_host<1>(a, lg0, log2h, true, tb.tw, scale); break;
        case 2: cenc_pass_host<2>(a, lg0, log2h, true, tb.tw, scale); break;
        default: cenc_pass_host<3>(a, lg0, log2h, true, tb.tw, scale); break;
        }
        u64* item_out = out + item * (plain ? 1 : tb.n_limbs) * n;
        for (size_t j = 0; j < h; j += 2) cenc_store_pair(item_out, j, a[j], a[j + 1], plain, tb);
    }
}

// the forward transform: Cooley-Tukey butterflies (u, v) -> (u + s v, u - s v) with s = conj(w), levels log2 n - 1 ... 0, then the slot of each position
void decode_complex_host(double* slots_out, const int64_t* coeffs, size_t items, double scale, bool real, u32 log2_n) {
    CencodeHostTables t;
    cenc_host_tables(log2_n, nullptr, 0, t);
    const u32 log2h = log2_n - 1;
    const size_t n = (size_t)1 << log2_n, h = n >> 1;
    std::vector<cenc_f64x2> a(h);
    for (size_t item = 0; item < items; ++item) {
        const int64_t* c = coeffs + item * n;
        for (size_t j = 0; j < h; ++j) a[j] = cenc_f64x2{(double)c[j], (double)c[j + h]};
        for (u32 lg = log2h; lg-- > 0;) {
            const size_t d = (size_t)1 << lg;
            for (size_t j = 0; j < h; ++j) {
                if (j & d) continue;
                const cenc_f64x2 w = t.tw[((size_t)1 << (log2h - 1 - lg)) + (j >> (lg + 1))];
                const cenc_f64x2 u = a[j], v = cenc_mul(a[j + d], cenc_f64x2{w.x, -w.y});
                a[j] = cenc_add(u, v);
                a[j + d] = cenc_sub(u, v);
            }
        }
        double* o = slots_out + item * (real ? h : n);
        for (size_t p = 0; p < h; ++p) {
            const u32 s = t.src[p], i = s & ~kCencConj;
            if (real) o[i] = a[p].x / scale;
            else {
                o[2 * (size_t)i] = a[p].x / scale;
                o[2 * (size_t)i + 1] = ((s & kCencConj) ? -a[p].y : a[p].y) / scale;
            }
        }
    }
}

}  // namespace dpfhe

// ------------------------------------------------------------------------------------------------
// complex slot encoding (cencode.h, k_cencode.hip): vectors of n = N / 2 complex (or real) slots -> round(Delta m), plain or as residues on every limb
struct dpfhe_cencoder {
    dpfhe_ctx* ctx = nullptr;
    void* d_blob = nullptr;   // one allocation: cenc_f64x2 tw[n] | CencLimb[L] | u32 src[n]
    CencodeTables tb{};
};

static const uint32_t kCencodeFlags = DPFHE_ENCODE_PLAIN | DPFHE_ENCODE_NTT | DPFHE_ENCODE_REAL;

// Delta / n, the factor the last level carries (n a power of two: exact unless it underflows); false unless Delta is finite and positive
static bool cencode_scale(double scale, uint32_t log2_n, double& scale_over_n) {
    if (!(scale > 0.0) || !std::isfinite(scale)) return false;
    scale_over_n = std::ldexp(scale, -(int)(log2_n - 1));
    return true;
}

extern "C" int dpfhe_cencoder_create(dpfhe_cencoder** out, dpfhe_ctx* c) {
    static const char* what = "dpfhe_cencoder_create";
    if (!out || !c) return fail(DPFHE_INVALID_ARGUMENT, what, "null argument");
    CencodeHostTables h;
    cenc_host_tables(c->log2n, c->moduli.data(), c->n_limbs, h);
    const size_t half = (size_t)1 << (c->log2n - 1);
    const size_t tw_bytes = half * sizeof(cenc_f64x2), limb_bytes = c->n_limbs * sizeof(CencLimb), src_bytes = half * sizeof(u32);
    std::vector<unsigned char> blob(tw_bytes + limb_bytes + src_bytes);
    std::memcpy(blob.data(), h.tw.data(), tw_bytes);
    std::memcpy(blob.data() + tw_bytes, h.limb.data(), limb_bytes);
    std::memcpy(blob.data() + tw_bytes + limb_bytes, h.src.data(), src_bytes);
    DPFHE_ON_DEVICE(c, what);
    dpfhe_cencoder* e = new (std::nothrow) dpfhe_cencoder;
    if (!e) return fail(DPFHE_OUT_OF_MEMORY, what, "host allocation");
    if (int rc = upload_blob(&e->d_blob, blob, what)) {
        delete e;
        return rc;
    }
    const unsigned char* d = static_cast<const unsigned char*>(e->d_blob);
    e->ctx = c;
    e->tb.tw = reinterpret_cast<const cenc_f64x2*>(d);
    e->tb.limb = reinterpret_cast<const CencLimb*>(d + tw_bytes);
    e->tb.src = reinterpret_cast<const u32*>(d + tw_bytes + limb_bytes);
    e->tb.log2n = c->log2n;
    e->tb.n_limbs = c->n_limbs;
    *out = e;
    return DPFHE_SUCCESS;
}

extern "C" int dpfhe_cencoder_destroy(dpfhe_cencoder* e) {
    if (!e) return DPFHE_SUCCESS;
    if (e->d_blob) (void)hipFree(e->d_blob);
    delete e;
    return DPFHE_SUCCESS;
}

extern "C" int dpfhe_encode_complex(dpfhe_cencoder* e, uint64_t* d_out, const double* d_slots, size_t items, double scale, uint32_t flags, void* stream) {
    static const char* what = "dpfhe_encode_complex";
    if (!e || !d_out || !d_slots || items == 0) return fail(DPFHE_INVALID_ARGUMENT, what, "null argument or items 0");
    if ((flags & ~kCencodeFlags) || (flags & (DPFHE_ENCODE_PLAIN | DPFHE_ENCODE_NTT)) == (DPFHE_ENCODE_PLAIN | DPFHE_ENCODE_NTT))
        return fail(DPFHE_INVALID_ARGUMENT, what, "unknown flag, or PLAIN together with NTT");
    if (misaligned(d_out) || misaligned(d_slots)) return fail(DPFHE_INVALID_ARGUMENT, what, "misaligned buffer");
    dpfhe_ctx* c = e->ctx;
    double scale_over_n = 0.0;
    if (!cencode_scale(scale, c->log2n, scale_over_n)) return fail(DPFHE_INVALID_ARGUMENT, what, "scale must be finite and positive");
    const bool plain = (flags & DPFHE_ENCODE_PLAIN) != 0, real = (flags & DPFHE_ENCODE_REAL) != 0;
    const size_t n = (size_t)1 << c->log2n;
    if (items > kMaxGrid / n) return fail(DPFHE_INVALID_ARGUMENT, what, "too many items for one launch");   // (tighter than the launcher's ItemChunkPlan: kept, it keeps every size below in range)
    if (overlaps_bytes(d_out, items * (plain ? 1 : c->n_limbs) * n * 8, d_slots, items * (real ? n / 2 : n) * 8))
        return fail(DPFHE_INVALID_ARGUMENT, what, "out and slots overlap");
    if ((flags & DPFHE_ENCODE_NTT) && !ntt_grid_fits(c, items * c->n_limbs)) return fail(DPFHE_INVALID_ARGUMENT, what, "too many items for one launch");
    DPFHE_ON_DEVICE(c, what);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (launch_encode_complex(d_out, d_slots, items, scale_over_n, real, plain, e->tb, s)) return fail(DPFHE_INVALID_ARGUMENT, what, "too many items for one launch");
    if (int rc = check_launch("encode_complex kernel launch")) return rc;
    if (flags & DPFHE_ENCODE_NTT) return ntt_launch_items(c, false, d_out, d_out, items, 0, s);
    return DPFHE_SUCCESS;
}

extern "C" int dpfhe_encode_complex_host(const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n, uint64_t* out, const double* slots, size_t items, double scale,
                                         uint32_t flags) {
    static const char* what = "dpfhe_encode_complex_host";
    if (!moduli || !out || !slots || items == 0) return fail(DPFHE_INVALID_ARGUMENT, what, "null argument or items 0");
    if (flags & ~(uint32_t)(DPFHE_ENCODE_PLAIN | DPFHE_ENCODE_REAL)) return fail(DPFHE_INVALID_ARGUMENT, what, "unknown flag (the host twin has no transform over the q_l)");
    if (int rc = check_host_ring(what, moduli, n_limbs, log2_n)) return rc;
    if (misaligned(out) || misaligned(slots)) return fail(DPFHE_INVALID_ARGUMENT, what, "misaligned buffer");
    double scale_over_n = 0.0;
    if (!cencode_scale(scale, log2_n, scale_over_n)) return fail(DPFHE_INVALID_ARGUMENT, what, "scale must be finite and positive");
    const size_t n = (size_t)1 << log2_n;
    const bool plain = (flags & DPFHE_ENCODE_PLAIN) != 0, real = (flags & DPFHE_ENCODE_REAL) != 0;
    if (items > ~(size_t)0 / (8 * n * n_limbs)) return fail(DPFHE_INVALID_ARGUMENT, what, "too many items");
    if (overlaps_bytes(out, items * (plain ? 1 : n_limbs) * n * 8, slots, items * (real ? n / 2 : n) * 8)) return fail(DPFHE_INVALID_ARGUMENT, what, "out and slots overlap");
    CencodeHostTables h;
    cenc_host_tables(log2_n, moduli, n_limbs, h);
    encode_complex_host(out, slots, items, scale_over_n, real, plain, h.view(log2_n));
    return DPFHE_SUCCESS;
}

extern "C" int dpfhe_decode_complex_host(uint32_t log2_n, double* slots_out, const int64_t* coeffs, size_t items, double scale, uint32_t flags) {
    static const char* what = "dpfhe_decode_complex_host";
    if (!slots_out || !coeffs || items == 0) return fail(DPFHE_INVALID_ARGUMENT, what, "null argument or items 0");
    if (flags & ~(uint32_t)DPFHE_ENCODE_REAL) return fail(DPFHE_INVALID_ARGUMENT, what, "unknown flag");
    if (log2_n < 8 || log2_n > 16) return fail(DPFHE_INVALID_ARGUMENT, what, "log2_n must lie in [8, 16]");
    if (!(scale > 0.0) || !std::isfinite(scale)) return fail(DPFHE_INVALID_ARGUMENT, what, "scale must be finite and positive");
    const size_t n = (size_t)1 << log2_n;
    if (items > ~(size_t)0 / (8 * n)) return fail(DPFHE_INVALID_ARGUMENT, what, "too many items");
    if (overlaps_bytes(slots_out, items * ((flags & DPFHE_ENCODE_REAL) ? n / 2 : n) * 8, coeffs, items * n * 8)) return fail(DPFHE_INVALID_ARGUMENT, what, "slots and coefficients overlap");
    decode_complex_host(slots_out, coeffs, items, scale, (flags & DPFHE_ENCODE_REAL) != 0, log2_n);
    return DPFHE_SUCCESS;
}
