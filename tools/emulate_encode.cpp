// emulate_encode.cpp - CPU emulation of the slot-encoding kernels (TEST INFRASTRUCTURE).
//
// Runs the per-lane code of deeppowers_amd/csrc/encode.h (enc_lane_*: exactly what k_encode.hip's kernels call between their barriers) for every lane
// id of every workgroup, step by step, with LDS as a plain array that starts poisoned.  tests/test_emulated_encode.py compares the words with the
// host twin, so the group / chunk / twiddle indexing of both kernel forms - also the two-kernel form, at chunk sizes small enough to run here - is
// proven on the CPU.  Built by the test (g++), never shipped, never on the product path.
#include <cstring>
#include <vector>

#include "../deeppowers_amd/csrc/encode.h"

using namespace dpfhe;

template <bool WHOLE>
static void lds_kernel(u64* out, const u32* slots, const EncodeTables& tb, u32 log2c, bool plain, u32 block, u32 T) {
    const u32 log2n = tb.log2n, C = 1u << log2c, chunk = block & ((1u << (log2n - log2c)) - 1u), base = chunk << log2c;
    const size_t item = block >> (log2n - log2c);
    std::vector<enc_u32x4> lds(C / 4);
    u32* a = reinterpret_cast<u32*>(lds.data());
    for (u32 p = 0; p < C; ++p) a[p] = 0xDEADBEEFu;
    for (u32 tid = 0; tid < T; ++tid) enc_lane_first_pass(a, slots + (item << log2n), tid, T, base, C, tb);
    u32 lg0 = kEncRadixLog;
    for (; log2c - lg0 > kEncRadixLog; lg0 += kEncRadixLog)
        for (u32 tid = 0; tid < T; ++tid) enc_lane_mid_pass(a, tid, T, base, C, lg0, tb);
    for (u32 tid = 0; tid < T; ++tid) enc_lane_last_pass<WHOLE>(a, tid, T, base, log2c, lg0, tb);
    u64* item_out = out + item * ((plain ? (size_t)1 : (size_t)tb.n_limbs) << log2n);
    for (u32 tid = 0; tid < T; ++tid) enc_lane_store<WHOLE>(item_out, a, tid, T, base, C, plain, tb);
}

// out: [items][N] (plain) or [items][L][N], 16-byte aligned.  log2c == log2n: the one-kernel form with `threads` lanes; log2c < log2n (by 1 ... 3): the
// two-kernel form.  0, or 1 for arguments the kernels' launcher would never be given.
extern "C" int emu_encode_slots(uint32_t log2n, uint32_t log2c, uint32_t threads, uint64_t t, const uint64_t* moduli, uint32_t n_limbs, uint64_t* out,
                                const uint32_t* slots, size_t items, int plain) {
    if (log2c < 8 || log2c > log2n || log2n - log2c > 3 || threads == 0 || (threads << kEncRadixLog) > (1u << log2c)) return 1;
    EncodeHostTables h;
    if (!enc_host_tables(log2n, t, moduli, n_limbs, h)) return 1;
    const EncodeTables tb = h.view(log2n, t);
    const u32 blocks = (u32)(items << (log2n - log2c));
    for (u32 b = 0; b < blocks; ++b) {
        if (log2c == log2n) lds_kernel<true>(out, slots, tb, log2c, plain != 0, b, threads);
        else lds_kernel<false>(out, slots, tb, log2c, plain != 0, b, threads);
    }
    if (log2c == log2n) return 0;
    for (size_t item = 0; item < items; ++item) {
        u64* item_out = out + item * ((plain ? (size_t)1 : (size_t)n_limbs) << log2n);
        for (u32 k = 0; k < (1u << log2c); k += 2) {   // one lane per pair of columns
            switch (log2n - log2c) {
            case 1: enc_lane_tail<1>(item_out, k, log2c, plain != 0, tb); break;
            case 2: enc_lane_tail<2>(item_out, k, log2c, plain != 0, tb); break;
            default: enc_lane_tail<3>(item_out, k, log2c, plain != 0, tb); break;
            }
        }
    }
    return 0;
}
