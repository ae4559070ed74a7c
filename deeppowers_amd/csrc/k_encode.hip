// k_encode.hip - slot encoding over Z_t (encode.h): the device kernels, their launcher and the host twin.
//
// N <= 16384: one workgroup of 512 lanes per slot vector.  It gathers the vector in transform order (the slot -> position table fused into the
// load) and keeps it in LDS (4 N bytes), runs the levels three at a time (each lane takes groups of 8 words through 3 levels in registers, one
// barrier per pass; the first pass works on the gathered words before they reach LDS; N^-1 rides on the last level), then every lane centres
// and lifts its pairs of coefficients and writes the L limb rows with 16-byte stores, each row contiguous across the wave.  4 bytes read and
// 8 L written per coefficient: a write stream (MEASUREMENTS.md "Slot encoding on the device": 256 and 1024 lanes measured slower at N = 8192).
// N = 32768, 65536 (the vector does not fit the 64 KiB a workgroup takes here): the first 13 levels run per 8192-word chunk as above and park their
// words in row 0 of the item's own output (low half of each 64-bit word); a second kernel takes, per lane, the 4 or 8 words 8192 apart of a pair of
// columns through the remaining levels in registers and writes all rows of exactly the positions it read - no scratch and no hazard.
#include "encode.h"

namespace dpfhe {

constexpr u32 kEncThreads = 256;      // lanes per workgroup of the second kernel
constexpr u32 kEncLdsThreads = 512;   // lanes per slot vector (or chunk) of the LDS kernel
constexpr u32 kEncMaxLdsLog = 14;     // 64 KiB of LDS
constexpr u32 kEncChunkLog = 13;      // chunk of the two-kernel form

// block b = item * chunks + chunk, chunks = N >> log2c.  WHOLE (log2c == log2 N): the full transform and the output; otherwise the first log2c levels
// of the chunk, parked in row 0 of the item's output.  The steps between the barriers are encode.h's enc_lane_*.
template <bool WHOLE>
__global__ __launch_bounds__(kEncLdsThreads) void encode_lds_kernel(u64* __restrict__ out, const u32* __restrict__ slots, const EncodeTables tb, u32 log2c,
                                                                    u32 plain) {
    extern __shared__ __attribute__((aligned(16))) u32 a[];
    const u32 tid = threadIdx.x, T = blockDim.x, log2n = tb.log2n;
    const u32 C = 1u << log2c, chunk = blockIdx.x & ((1u << (log2n - log2c)) - 1u), base = chunk << log2c;
    const size_t item = blockIdx.x >> (log2n - log2c);
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
    constexpr u32 kBlocksPerItem = (1u << (kEncChunkLog - 1)) / kEncThreads;
    const u32 k = 2 * ((blockIdx.x % kBlocksPerItem) * kEncThreads + threadIdx.x);
    const size_t item = blockIdx.x / kBlocksPerItem;
    enc_lane_tail<R>(out + item * ((plain ? (size_t)1 : (size_t)tb.n_limbs) << tb.log2n), k, kEncChunkLog, plain != 0, tb);
}

int launch_encode_slots(u64* out, const u32* slots, size_t items, bool plain, const EncodeTables& tb, hipStream_t s) {
    const u32 log2n = tb.log2n;
    const bool whole = log2n <= kEncMaxLdsLog;
    const u32 log2c = whole ? log2n : kEncChunkLog;
    const u32 C = 1u << log2c, threads = (C >> kEncRadixLog) < kEncLdsThreads ? (C >> kEncRadixLog) : kEncLdsThreads;
    const size_t grid = items << (log2n - log2c);
    if (grid == 0 || grid > 0x7fffffffu || (grid >> (log2n - log2c)) != items) return -1;
    if (whole) {
        hipLaunchKernelGGL(encode_lds_kernel<true>, dim3((unsigned)grid), dim3(threads), C * sizeof(u32), s, out, slots, tb, log2c, plain ? 1u : 0u);
        return 0;
    }
    hipLaunchKernelGGL(encode_lds_kernel<false>, dim3((unsigned)grid), dim3(threads), C * sizeof(u32), s, out, slots, tb, log2c, plain ? 1u : 0u);
    const size_t tail_grid = items * ((1u << (kEncChunkLog - 1)) / kEncThreads);
    if (log2n - kEncChunkLog == 2)
        hipLaunchKernelGGL(encode_tail_kernel<2>, dim3((unsigned)tail_grid), dim3(kEncThreads), 0, s, out, tb, plain ? 1u : 0u);
    else
        hipLaunchKernelGGL(encode_tail_kernel<3>, dim3((unsigned)tail_grid), dim3(kEncThreads), 0, s, out, tb, plain ? 1u : 0u);
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
