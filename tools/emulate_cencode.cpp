// emulate_cencode.cpp - CPU emulation of the complex slot-encoding kernels (TEST INFRASTRUCTURE).
//
// Runs the per-lane code of deeppowers_amd/csrc/cencode.h (cenc_lane_*: exactly what k_cencode.hip's kernels call between their barriers) for every
// lane id of every workgroup, step by step, with LDS as a plain array that starts poisoned.  tests/test_emulated_cencode.py compares the words with the
// host twin, so the group / chunk / twiddle indexing of both kernel forms - also the parking of the two-kernel form in row 0 - is proven on the CPU.
// Built by the test (g++ -ffp-contract=off), never shipped, never on the product path.
#include <cmath>
#include <vector>

#include "../deeppowers_amd/csrc/cencode.h"

using namespace dpfhe;

template <bool WHOLE>
static void lds_kernel(u64* out, const double* slots, const CencodeTables& tb, u32 log2c, double scale, bool real, bool plain, u32 block, u32 T) {
    const u32 log2h = tb.log2n - 1, C = 1u << log2c, chunk = block & ((1u << (log2h - log2c)) - 1u), base = chunk << log2c;
    const size_t item = block >> (log2h - log2c);
    std::vector<cenc_f64x2> lds(C, cenc_f64x2{std::nan(""), std::nan("")});
    cenc_f64x2* a = lds.data();
    for (u32 tid = 0; tid < T; ++tid) cenc_lane_first_pass(a, slots + (item << (real ? log2h : tb.log2n)), real, tid, T, base, C, tb);
    u32 lg0 = kCencRadixLog;
    for (; log2c - lg0 > kCencRadixLog; lg0 += kCencRadixLog)
        for (u32 tid = 0; tid < T; ++tid) cenc_lane_mid_pass(a, tid, T, base, C, lg0, tb);
    for (u32 tid = 0; tid < T; ++tid) cenc_lane_last_pass<WHOLE>(a, tid, T, base, log2c, lg0, scale, tb);
    u64* item_out = out + item * ((plain ? (size_t)1 : (size_t)tb.n_limbs) << tb.log2n);
    for (u32 tid = 0; tid < T; ++tid) cenc_lane_store<WHOLE>(item_out, a, tid, T, base, C, plain, tb);
}

// out: [items][N] (plain) or [items][L][N], 16-byte aligned like slots.  log2c == log2n - 1: the one-kernel form with `threads` lanes; log2c below that
// (by 1 ... 3): the two-kernel form.  0, or 1 for arguments the kernels' launcher would never be given.
extern "C" int emu_encode_complex(uint32_t log2n, uint32_t log2c, uint32_t threads, const uint64_t* moduli, uint32_t n_limbs, uint64_t* out, const double* slots,
                                  size_t items, double scale, int real, int plain) {
    const u32 log2h = log2n - 1;
    if (log2c < 7 || log2c > log2h || log2h - log2c > 3 || threads == 0 || (threads << kCencRadixLog) > (1u << log2c)) return 1;
    CencodeHostTables h;
    cenc_host_tables(log2n, moduli, n_limbs, h);
    const CencodeTables tb = h.view(log2n);
    const double scale_over_n = std::ldexp(scale, -(int)log2h);
    const u32 blocks = (u32)(items << (log2h - log2c));
    for (u32 b = 0; b < blocks; ++b) {
        if (log2c == log2h) lds_kernel<true>(out, slots, tb, log2c, scale_over_n, real != 0, plain != 0, b, threads);
        else lds_kernel<false>(out, slots, tb, log2c, 0.0, real != 0, plain != 0, b, threads);
    }
    if (log2c == log2h) return 0;
    for (size_t item = 0; item < items; ++item) {
        u64* item_out = out + item * ((plain ? (size_t)1 : (size_t)n_limbs) << log2n);
        for (u32 k = 0; k < (1u << log2c); k += 2) {   // one lane per pair of columns
            switch (log2h - log2c) {
            case 1: cenc_lane_tail<1>(item_out, k, log2c, scale_over_n, plain != 0, tb); break;
            case 2: cenc_lane_tail<2>(item_out, k, log2c, scale_over_n, plain != 0, tb); break;
            default: cenc_lane_tail<3>(item_out, k, log2c, scale_over_n, plain != 0, tb); break;
            }
        }
    }
    return 0;
}
