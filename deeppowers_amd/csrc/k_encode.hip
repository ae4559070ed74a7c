// k_encode.hip - slot encoding over Z_t (encode.h): the device kernels, their launcher, the host twin and the entries of include/dpfhe.h.
//
// N <= 16384: one workgroup of 512 lanes per slot vector.  It gathers the vector in transform order (the slot -> position table fused into the
// load) and keeps it in LDS (4 N bytes), runs the levels three at a time (each lane takes groups of 8 words through 3 levels in registers, one
// barrier per pass; the first pass works on the gathered words before they reach LDS; N^-1 rides on the last level), then every lane centres
// and lifts its pairs of coefficients and writes the L limb rows with 16-byte stores, each row contiguous across the wave.  4 bytes read and
// 8 L written per coefficient: a write stream (MEASUREMENTS.md "Slot encoding on the device": 256 and 1024 lanes measured slower at N = 8192).
// N = 32768, 65536 (the vector does not fit the 64 KiB a workgroup takes here): the first 13 levels run per 8192-word chunk as above and park their
// words in row 0 of the item's own output (low half of each 64-bit word); a second kernel takes, per lane, the 4 or 8 words 8192 apart of a pair of
// columns through the remaining levels in registers and writes all rows of exactly the positions it read - no scratch and no hazard.
#include <cstring>
#include <new>

#include "cabi.h"
#include "encode.h"

namespace dpfhe {

constexpr u32 kEncThreads = 256;      // lanes per workgroup of the second kernel
constexpr u32 kEncLdsThreads = 512;   // lanes per slot vector (or chunk) of the LDS kernel
constexpr u32 kEncMaxLdsLog = 14;     // 64 KiB of LDS
constexpr u32 kEncChunkLog = 13;      // chunk of the two-kernel form
// the second kernel's blocks: a lane per pair of columns of a chunk (in the kernel with % and /: as mask and shift its butterflies change, profiles/r21_item_chunk_map.txt)
constexpr ItemChunkPlan enc_tail_plan(size_t items) { return ItemChunkMap::plan(items, 1u << (kEncChunkLog - 1), kEncThreads); }

// A workgroup per chunk of 2^log2c words (workmap.h ItemChunkMap, N >> log2c chunks per item).  WHOLE (log2c == log2 N): the full transform and the output;
// otherwise the first log2c levels of the chunk, parked in row 0 of the item's output.  The steps between the barriers are encode.h's enc_lane_*.
template <bool WHOLE>
__global__ __launch_bounds__(kEncLdsThreads) void encode_lds_kernel(u64* __restrict__ out, const u32* __restrict__ slots, const EncodeTables tb, u32 log2c,
                                                                    u32 plain) {
    extern __shared__ __attribute__((aligned(16))) u32 a[];
    const u32 tid = threadIdx.x, T = blockDim.x, log2n = tb.log2n;
    const u32 C = 1u << log2c, chunk = ItemChunkMap::chunk(blockIdx.x, log2n - log2c), base = chunk << log2c;
    const size_t item = ItemChunkMap::outer(blockIdx.x, log2n - log2c);
    enc_lane_first_pass(a, slots + (item << log2n), tid, T, base, C, tb);
    __syncthreads();
    u32 lg0 = kEncRadixLog;
    for (; log2c - lg0 > kEncRadixLog; lg0 += kEncRadixLog) {
        enc_lane_mid_pass(a, tid, T, base, C, lg0, tb);
        __syncthreads();
    }
    enc_lane_last_pass<WHOLE>(a, tid, T, base, log2c, lg0, tb);
    __syncthreads();
    enc_lane_store<WHOLE>(out + item * ((plain ? (size_t)1 : (size_t)tb.n_limbs) << log2n), a, tid, T, base, C, plain != 0, tb);
}

// the last R = log2 N - 13 levels: lane j of an item owns coefficients 2 j, 2 j + 1 of each of the 2^R chunks
template <int R>
__global__ __launch_bounds__(kEncThreads) void encode_tail_kernel(u64* __restrict__ out, const EncodeTables tb, u32 plain) {
    constexpr u32 kBlocksPerItem = 1u << enc_tail_plan(1).log2_chunks;
    const u32 k = 2 * ItemChunkMap::lane(blockIdx.x % kBlocksPerItem, kEncThreads, threadIdx.x);
    const size_t item = blockIdx.x / kBlocksPerItem;
    enc_lane_tail<R>(out + item * ((plain ? (size_t)1 : (size_t)tb.n_limbs) << tb.log2n), k, kEncChunkLog, plain != 0, tb);
}

// device: out = the encoding of d_slots [items][N]; plain: [items][N] words in [0, t), else [items][L][N] residues.  0, or -1 if the grid is too large.
static int launch_encode_slots(u64* out, const u32* slots, size_t items, bool plain, const EncodeTables& tb, hipStream_t s) {
    const u32 log2n = tb.log2n;
    const bool whole = log2n <= kEncMaxLdsLog;
    const u32 log2c = whole ? log2n : kEncChunkLog;
    const u32 C = 1u << log2c, threads = (C >> kEncRadixLog) < kEncLdsThreads ? (C >> kEncRadixLog) : kEncLdsThreads;
    const ItemChunkPlan p = ItemChunkMap::fixed(items, threads, log2n - log2c), tail = enc_tail_plan(items);
    if (!p.ok || (!whole && !tail.ok)) return -1;
    if (whole) {
        hipLaunchKernelGGL(encode_lds_kernel<true>, dim3((unsigned)p.grid), dim3(threads), C * sizeof(u32), s, out, slots, tb, log2c, plain ? 1u : 0u);
        return 0;
    }
    hipLaunchKernelGGL(encode_lds_kernel<false>, dim3((unsigned)p.grid), dim3(threads), C * sizeof(u32), s, out, slots, tb, log2c, plain ? 1u : 0u);
    if (log2n - kEncChunkLog == 2)
        hipLaunchKernelGGL(encode_tail_kernel<2>, dim3((unsigned)tail.grid), dim3(kEncThreads), 0, s, out, tb, plain ? 1u : 0u);
    else
        hipLaunchKernelGGL(encode_tail_kernel<3>, dim3((unsigned)tail.grid), dim3(kEncThreads), 0, s, out, tb, plain ? 1u : 0u);
    return 0;
}

template <int R>
static void enc_pass_host(u32* a, u32 lg0, u32 log2n, bool last, const EncTw* tw, u32 t) {
    for (u32 g = 0; g < (1u << (log2n - R)); ++g) {
        if (last) enc_group_mem<R, true>(a, g, 0, lg0, log2n, tw, t);
        else enc_group_mem<R, false>(a, g, 0, lg0, log2n, tw, t);
    }
}

void encode_slots_host(u64* out, const u32* slots, size_t items, bool plain, const EncodeTables& tb) {
    const u32 log2n = tb.log2n;
    const size_t n = (size_t)1 << log2n;
    u32* a = new u32[n];
    for (size_t item = 0; item < items; ++item) {
        for (size_t p = 0; p < n; ++p) a[p] = enc_slot(slots[item * n + tb.src[p]], tb.t);
        u32 lg0 = 0;
        for (; log2n - lg0 > kEncRadixLog; lg0 += kEncRadixLog) enc_pass_host<3>(a, lg0, log2n, false, tb.tw, tb.t);
        switch (log2n - lg0) {
        case 1: enc_pass_host<1>(a, lg0, log2n, true, tb.tw, tb.t); break;
        case 2: enc_pass_host<2>(a, lg0, log2n, true, tb.tw, tb.t); break;
        default: enc_pass_host<3>(a, lg0, log2n, true, tb.tw, tb.t); break;
        }
        u64* item_out = out + item * (plain ? 1 : tb.n_limbs) * n;
        for (size_t k = 0; k < n; ++k) {
            if (plain) item_out[k] = a[k];
            else
                for (u32 l = 0; l < tb.n_limbs; ++l) item_out[l * n + k] = enc_lift(a[k], tb.t, tb.half, tb.limb[l]);
        }
    }
    delete[] a;
}

}  // namespace dpfhe

// ------------------------------------------------------------------------------------------------
// slot encoding over Z_t (encode.h, k_encode.hip): slot vectors -> message polynomials, plain or as residues on every limb of the context
// validates (log2_n, t) and builds the tables of the definition in include/dpfhe.h
static int encode_tables(const char* what, uint32_t log2_n, uint64_t t, const uint64_t* moduli, uint32_t n_limbs, EncodeHostTables& h) {
    const uint64_t n = (uint64_t)1 << log2_n;
    if (t < 3 || (t >> 32) || (t - 1) % (2 * n) != 0 || !h_is_prime(t)) return fail(DPFHE_INVALID_ARGUMENT, what, "t must be a prime = 1 mod 2N below 2^32");
    if (!enc_host_tables(log2_n, t, moduli, n_limbs, h)) return fail(DPFHE_INVALID_ARGUMENT, what, "no primitive 2N-th root of unity mod t");
    return DPFHE_SUCCESS;
}

struct dpfhe_encoder {
    dpfhe_ctx* ctx = nullptr;
    uint64_t zeta = 0;
    void* d_blob = nullptr;   // one allocation: EncTw[N + 1] | EncLimb[L] | u32 src[N]
    EncodeTables tb{};
};

static const uint32_t kEncodeFlags = DPFHE_ENCODE_PLAIN | DPFHE_ENCODE_NTT;

extern "C" int dpfhe_encoder_create(dpfhe_encoder** out, dpfhe_ctx* c, uint64_t t) {
    static const char* what = "dpfhe_encoder_create";
    if (!out || !c) return fail(DPFHE_INVALID_ARGUMENT, what, "null argument");
    EncodeHostTables h;
    if (int rc = encode_tables(what, c->log2n, t, c->moduli.data(), c->n_limbs, h)) return rc;
    const size_t n = (size_t)1 << c->log2n;
    const size_t tw_bytes = ((n + 1) * sizeof(EncTw) + 15) & ~(size_t)15, limb_bytes = c->n_limbs * sizeof(EncLimb), src_bytes = n * sizeof(u32);
    std::vector<unsigned char> blob(tw_bytes + limb_bytes + src_bytes);
    std::memcpy(blob.data(), h.tw.data(), (n + 1) * sizeof(EncTw));
    std::memcpy(blob.data() + tw_bytes, h.limb.data(), limb_bytes);
    std::memcpy(blob.data() + tw_bytes + limb_bytes, h.src.data(), src_bytes);
    DPFHE_ON_DEVICE(c, what);
    dpfhe_encoder* e = new (std::nothrow) dpfhe_encoder;
    if (!e) return fail(DPFHE_OUT_OF_MEMORY, what, "host allocation");
    if (int rc = upload_blob(&e->d_blob, blob, what)) {
        delete e;
        return rc;
    }
    const unsigned char* d = static_cast<const unsigned char*>(e->d_blob);
    e->ctx = c;
    e->zeta = h.zeta;
    e->tb.tw = reinterpret_cast<const EncTw*>(d);
    e->tb.limb = reinterpret_cast<const EncLimb*>(d + tw_bytes);
    e->tb.src = reinterpret_cast<const u32*>(d + tw_bytes + limb_bytes);
    e->tb.t = (u32)t;
    e->tb.half = (u32)((t - 1) / 2);
    e->tb.log2n = c->log2n;
    e->tb.n_limbs = c->n_limbs;
    *out = e;
    return DPFHE_SUCCESS;
}

extern "C" int dpfhe_encoder_destroy(dpfhe_encoder* e) {
    if (!e) return DPFHE_SUCCESS;
    if (e->d_blob) (void)hipFree(e->d_blob);
    delete e;
    return DPFHE_SUCCESS;
}

extern "C" uint64_t dpfhe_encoder_root(const dpfhe_encoder* e) { return e ? e->zeta : 0; }

extern "C" int dpfhe_encode_slots(dpfhe_encoder* e, uint64_t* d_out, const uint32_t* d_slots, size_t items, uint32_t flags, void* stream) {
    static const char* what = "dpfhe_encode_slots";
    if (!e || !d_out || !d_slots || items == 0) return fail(DPFHE_INVALID_ARGUMENT, what, "null argument or items 0");
    if ((flags & ~kEncodeFlags) || flags == kEncodeFlags) return fail(DPFHE_INVALID_ARGUMENT, what, "unknown flag, or PLAIN together with NTT");
    if (misaligned(d_out) || misaligned(d_slots)) return fail(DPFHE_INVALID_ARGUMENT, what, "misaligned buffer");
    dpfhe_ctx* c = e->ctx;
    const bool plain = (flags & DPFHE_ENCODE_PLAIN) != 0;
    const size_t n = (size_t)1 << c->log2n;
    if (items > kMaxGrid / n) return fail(DPFHE_INVALID_ARGUMENT, what, "too many items for one launch");   // (tighter than the launcher's ItemChunkPlan: kept, it keeps every size below in range)
    if (overlaps_bytes(d_out, items * (plain ? 1 : c->n_limbs) * n * 8, d_slots, items * n * 4)) return fail(DPFHE_INVALID_ARGUMENT, what, "out and slots overlap");
    if ((flags & DPFHE_ENCODE_NTT) && !ntt_grid_fits(c, items * c->n_limbs)) return fail(DPFHE_INVALID_ARGUMENT, what, "too many items for one launch");
    DPFHE_ON_DEVICE(c, what);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (launch_encode_slots(d_out, d_slots, items, plain, e->tb, s)) return fail(DPFHE_INVALID_ARGUMENT, what, "too many items for one launch");
    if (int rc = check_launch("encode_slots kernel launch")) return rc;
    if (flags & DPFHE_ENCODE_NTT) return ntt_launch_items(c, false, d_out, d_out, items, 0, s);
    return DPFHE_SUCCESS;
}

extern "C" int dpfhe_encode_slots_host(const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n, uint64_t t, uint64_t* out, const uint32_t* slots, size_t items,
                                       uint32_t flags) {
    static const char* what = "dpfhe_encode_slots_host";
    if (!moduli || !out || !slots || items == 0) return fail(DPFHE_INVALID_ARGUMENT, what, "null argument or items 0");
    if (flags & ~(uint32_t)DPFHE_ENCODE_PLAIN) return fail(DPFHE_INVALID_ARGUMENT, what, "unknown flag (the host twin has no transform over the q_l)");
    if (int rc = check_host_ring(what, moduli, n_limbs, log2_n)) return rc;
    EncodeHostTables h;
    if (int rc = encode_tables(what, log2_n, t, moduli, n_limbs, h)) return rc;
    const size_t n = (size_t)1 << log2_n;
    const bool plain = (flags & DPFHE_ENCODE_PLAIN) != 0;
    if (items > ~(size_t)0 / (8 * n * n_limbs)) return fail(DPFHE_INVALID_ARGUMENT, what, "too many items");
    if (overlaps_bytes(out, items * (plain ? 1 : n_limbs) * n * 8, slots, items * n * 4)) return fail(DPFHE_INVALID_ARGUMENT, what, "out and slots overlap");
    for (size_t i = 0; i < items * n; ++i)
        if (slots[i] >= t) return fail(DPFHE_INVALID_ARGUMENT, what, "slot value >= t");
    encode_slots_host(out, slots, items, plain, h.view(log2_n, t));
    return DPFHE_SUCCESS;
}
