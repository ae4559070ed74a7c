// k_compact.hip - compact result ciphertexts (compact.h): the device kernel, its launcher, the host twin and the entries of include/dpfhe.h.
//
// One lane per pair of coefficients: for each component it reads its pair of every limb row (16-byte loads, each row contiguous across the wave),
// computes the two switched values in registers and parks them in LDS.  After one barrier the block's bit strings are gathered from LDS into
// 16-byte chunks: the block's 2 T values of component c are 2 T k_c bits = T k_c / 64 chunks (T >= 128 lanes, so every chunk is whole and
// starts on a 32-byte boundary of the record), and every global store is one full 16-byte contiguous store.  Blocks and lanes: workmap.h ItemChunkMap.
#include "cabi.h"
#include "compact.h"

namespace dpfhe {

constexpr u32 kCompactThreads = 256;

// lane `tid`'s two values of component C, parked in LDS
template <int NL, int C>
__device__ __forceinline__ void compact_pair(u64* vals, const u64* __restrict__ in, const CompactArgs& a, size_t item, size_t poly, size_t k, u32 tid) {
    const u64* src = in + (item * 2 + C) * NL * poly + k;
    u64 x0[NL], x1[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const u64x2_t w = *reinterpret_cast<const u64x2_t*>(src + l * poly);
        x0[l] = w.x;
        x1[l] = w.y;
    }
    vals[2 * tid] = compact_value<NL>(x0, C, a);
    vals[2 * tid + 1] = compact_value<NL>(x1, C, a);
}

// lane j of an item owns coefficients 2 j, 2 j + 1
template <int NL>
__global__ __launch_bounds__(kCompactThreads) void compact_kernel(uint8_t* __restrict__ out, const u64* __restrict__ in, const CompactArgs a, u32 log2n,
                                                                  u32 log2_chunks) {
    __shared__ u64 vals[2][2 * kCompactThreads];
    const u32 tid = threadIdx.x, T = blockDim.x;
    const ItemChunkWork w = ItemChunkMap::decode(blockIdx.x, log2_chunks);
    const size_t item = w.outer;
    const size_t poly = (size_t)1 << log2n;
    const size_t k = 2 * ItemChunkMap::lane<size_t>(w.chunk, T, tid);
    compact_pair<NL, 0>(vals[0], in, a, item, poly, k, tid);
    compact_pair<NL, 1>(vals[1], in, a, item, poly, k, tid);
    __syncthreads();
    const u32 ch0 = T * a.bits[0] / 64, ch1 = T * a.bits[1] / 64;   // 16-byte chunks of the block's bit string per component
    uint8_t* rec = out + item * compact_record_bytes(log2n, a);
    for (u32 m = tid; m < ch0 + ch1; m += T) {
        const u32 c = m >= ch0 ? 1u : 0u, mm = c ? m - ch0 : m, kb = a.bits[c];
        const u32 b0 = 128 * mm;                                          // chunk mm holds bits [b0, b0 + 128) of the block's string
        u64 lo = 0, hi = 0;
        for (u32 j = b0 / kb; j <= (b0 + 127) / kb; ++j) {               // the <= 17 values that overlap it
            const u64 v = vals[c][j];
            const int p = (int)(j * kb) - (int)b0;
            if (p < 0) lo |= v >> -p;
            else if (p == 0) lo |= v;
            else if (p < 64) { lo |= v << p; hi |= v >> (64 - p); }
            else hi |= v << (p - 64);
        }
        const size_t off = (c ? ((size_t)a.bits[0] << log2n) / 8 : 0) + (size_t)w.chunk * T * kb / 4 + 16 * (size_t)mm;
        *reinterpret_cast<u64x2_t*>(rec + off) = u64x2_t{lo, hi};
    }
}

// device: out = the records of in [batch][2][L][N] (log2n >= 8; out and in 16-byte aligned).  0, or -1 if the grid is too large for one launch.
static int launch_compact(int log2n, uint8_t* out, const u64* in, size_t batch, const CompactArgs& a, hipStream_t s) {
    const ItemChunkPlan p = ItemChunkMap::plan(batch, 1u << (log2n - 1), kCompactThreads);   // (the kernel's LDS array holds kCompactThreads pairs)
    if (!p.ok) return -1;
    const bool ok = compact_with_limbs(a.n_limbs, [&](auto nl) {
        hipLaunchKernelGGL(compact_kernel<decltype(nl)::value>, dim3((unsigned)p.grid), dim3(p.threads), 0, s, out, in, a, (u32)log2n, p.log2_chunks);
    });
    return ok ? 0 : -1;
}

void compact_host(int log2n, uint8_t* out, const u64* in, size_t batch, const CompactArgs& a) {
    const size_t n = (size_t)1 << log2n, rec = compact_record_bytes(log2n, a);
    compact_with_limbs(a.n_limbs, [&](auto nl) {
        constexpr int NL = decltype(nl)::value;
        for (size_t i = 0; i < batch; ++i) {
            uint8_t* dst = out + i * rec;
            for (int c = 0; c < 2; ++c) {
                const u64* src = in + (i * 2 + c) * NL * n;
                const u32 kb = a.bits[c];
                for (size_t b = 0; b < (n * kb) / 8; ++b) dst[b] = 0;
                for (size_t j = 0; j < n; ++j) {
                    u64 x[NL];
                    for (int l = 0; l < NL; ++l) x[l] = src[l * n + j];
                    const u64 v = compact_value<NL>(x, c, a);
                    for (u32 b = 0; b < kb; ++b) {
                        const size_t bit = j * kb + b;
                        dst[bit / 8] |= (uint8_t)(((v >> b) & 1u) << (bit % 8));
                    }
                }
                dst += (n * kb) / 8;
            }
        }
    });
}

}  // namespace dpfhe

// ------------------------------------------------------------------------------------------------
// compact result ciphertexts (compact.h, k_compact.hip): round(2^k X / Q) mod 2^k per component, bit-packed
// validates the widths and limb count, then fills every constant; the moduli must be pairwise coprime (their inverses exist)
static int compact_args(const char* what, uint32_t bits0, uint32_t bits1, const uint64_t* moduli, uint32_t n_limbs, CompactArgs& a) {
    if (bits0 < kCompactMinBits || bits0 > kCompactMaxBits || bits1 < kCompactMinBits || bits1 > kCompactMaxBits)
        return fail(DPFHE_INVALID_ARGUMENT, what, "widths must lie in [8, 60]");
    if (n_limbs == 0 || n_limbs > kCompactMaxLimbs) return fail(DPFHE_INVALID_ARGUMENT, what, "1 to 10 limbs (rescale first)");
    a = CompactArgs{};
    a.n_limbs = n_limbs;
    a.bits[0] = bits0; a.bits[1] = bits1;
    a.q64 = 1;
    for (uint32_t k = 0; k < n_limbs; ++k) {
        const uint64_t q = moduli[k];
        a.q[k] = q;
        a.lift[k] = q * ((((uint64_t)1 << 60) + q - 1) / q);   // < 2^60 + q
        for (uint32_t i = 0; i < k; ++i) {
            if (!inverse_mod(moduli[i], q, a.inv[k][i])) return fail(DPFHE_INVALID_ARGUMENT, what, "moduli must be pairwise coprime");
            a.inv_sh[k][i] = (uint64_t)(((unsigned __int128)a.inv[k][i] << 64) / q);
        }
        for (int c = 0; c < 2; ++c) {
            a.pow2[c][k] = (uint64_t)(((unsigned __int128)1 << a.bits[c]) % q);
            a.pow2_sh[c][k] = (uint64_t)(((unsigned __int128)a.pow2[c][k] << 64) / q);
        }
        a.q64 *= q;
    }
    uint64_t inv = a.q64;   // Q odd: Q Q = 1 mod 8, and each Newton step doubles the correct low bits
    for (int s = 0; s < 5; ++s) inv *= 2 - a.q64 * inv;
    a.qinv64 = inv;
    // floor(Q / 2) = (Q - 1) / 2 has the residues (q_i - 1) / 2 (Q = 0 and 2^-1 = (q_i + 1) / 2 mod q_i); its digits as the kernel computes them
    for (uint32_t i = 0; i < n_limbs; ++i) a.half[i] = (moduli[i] - 1) / 2;
    compact_with_limbs(n_limbs, [&](auto nl) {
        constexpr int NL = decltype(nl)::value;
        u64 v[NL];
        for (int i = 0; i < NL; ++i) v[i] = a.half[i];
        compact_digits<NL>(v, a);
        for (int i = 0; i < NL; ++i) a.half[i] = v[i];
    });
    return DPFHE_SUCCESS;
}

extern "C" int dpfhe_compact(dpfhe_ctx* c, uint8_t* d_out, const uint64_t* d_in, size_t batch, uint32_t bits0, uint32_t bits1, void* stream) {
    static const char* what = "dpfhe_compact";
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    if (!d_out || !d_in || batch == 0) return fail(DPFHE_INVALID_ARGUMENT, what, "null buffer or batch 0");
    CompactArgs a;
    if (int rc = compact_args(what, bits0, bits1, c->moduli.data(), c->n_limbs, a)) return rc;
    if (misaligned(d_out) || misaligned(d_in)) return fail(DPFHE_INVALID_ARGUMENT, what, "misaligned buffer");
    const size_t words = batch * 2 * ((size_t)c->n_limbs << c->log2n), bytes = batch * compact_record_bytes(c->log2n, a);
    if (overlaps_bytes(d_out, bytes, d_in, words * 8)) return fail(DPFHE_INVALID_ARGUMENT, what, "out and in overlap");
    DPFHE_ON_DEVICE(c, what);
    if (launch_compact((int)c->log2n, d_out, d_in, batch, a, static_cast<hipStream_t>(stream)))
        return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    return check_launch("compact kernel launch");
}

extern "C" int dpfhe_compact_host(const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n, uint8_t* out, const uint64_t* in, size_t batch, uint32_t bits0,
                                  uint32_t bits1) {
    static const char* what = "dpfhe_compact_host";
    if (!moduli || !out || !in || batch == 0) return fail(DPFHE_INVALID_ARGUMENT, what, "null buffer or batch 0");
    if (log2_n < 8 || log2_n > (uint32_t)kMaxLog2N) return fail(DPFHE_INVALID_ARGUMENT, what, "log2_n in [8, 16]");
    if (n_limbs == 0 || n_limbs > kCompactMaxLimbs) return fail(DPFHE_INVALID_ARGUMENT, what, "1 to 10 limbs (rescale first)");
    if (int rc = check_host_ring(what, moduli, n_limbs, log2_n)) return rc;   // (after this twin's own shape messages: only the moduli can fail here)
    CompactArgs a;
    if (int rc = compact_args(what, bits0, bits1, moduli, n_limbs, a)) return rc;
    const size_t words = batch * 2 * ((size_t)n_limbs << log2_n), bytes = batch * compact_record_bytes(log2_n, a);
    if (overlaps_bytes(out, bytes, in, words * 8)) return fail(DPFHE_INVALID_ARGUMENT, what, "out and in overlap");
    compact_host((int)log2_n, out, in, batch, a);
    return DPFHE_SUCCESS;
}
