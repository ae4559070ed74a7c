// emulate_rotate_sum.cpp - CPU emulation of hoisted_qp_sum_kernel's per-lane code (TEST INFRASTRUCTURE, like emulate_mul_outer.cpp).
// Runs deeppowers_amd/csrc/rotate_sum.h QpSumLane<Arith> - the very code the kernel runs between its loads and its stores - for ONE word pair of one tile and
// every arithmetic policy that takes the prime, with the precondition counter of the lazy sums armed: the kernel's term loop, u = 0 .. R J - 1 with
// (r, j) = (u / J, u % J), begin_term once per term, then the live rows.  Built by tests/test_emulated_rotate_sum.py (g++), never shipped.
#define DPFHE_EMU_CHECK 1
#include <stddef.h>
#include <string.h>

#include "../deeppowers_amd/csrc/rotate_sum.h"
#include "../deeppowers_amd/csrc/tables.h"

namespace dpfhe {
long g_emu_overflows = 0;
}
using namespace dpfhe;

extern "C" long emu_rotate_sum_overflows() { return g_emu_overflows; }
extern "C" int emu_rotate_sum_tile() { return kQpSumTile; }
extern "C" int emu_rotate_sum_period() { return FoldArith::kDot30Period; }
extern "C" void emu_rotate_sum_notes_reset() { memset(g_emu_notes, 0, sizeof g_emu_notes); }
// the remainder-edge masks (modarith.h DPFHE_EMU_NOTE), one word per EmuSite
extern "C" int emu_rotate_sum_notes_get(unsigned* out, int cap) {
    for (int i = 0; i < kEmuSiteCount && i < cap; ++i) out[i] = g_emu_notes[i];
    return kEmuSiteCount;
}
// 1 when policy `cls` (tables.h LimbClass) takes the prime q
extern "C" int emu_rotate_sum_takes(int cls, u64 q) {
    if (q < 3 || !(q & 1) || (q >> 60)) return 0;
    if (cls == kClassFold) return fold_eligible(q);
    if (cls == kClassF64) return f64_eligible(q);
    if (cls == kClassFoldScaled) return fold_scaled_shift(q) != 0;
    if (cls == kClassF64Wide) return q < (1ull << F64WideArith::kMaxBits);
    return cls == kClassShoup;
}

template <class Arith>
static void run(const LimbConst& lc, u64 p_special, unsigned n_rot, int J, int Ld, unsigned rows, const u64* x, const u64* keys, u64* out) {
    QpSumLane<Arith> lane;
    lane.clear();
    const u64 pmod = QpSumLane<Arith>::p_operand(p_special, lc);
    const unsigned total = n_rot * (unsigned)J;
    for (unsigned u = 0; u < total; ++u) {
        const int j = (int)(u % (unsigned)J);
        const u64* xu = x + (size_t)u * rows * 2;
        lane.begin_term(lc);
        if (j < Ld) {
            const u64* e = keys + (size_t)u * 4;
            const typename QpSumLane<Arith>::Key k = QpSumLane<Arith>::split_key(e[0], e[1], e[2], e[3]);
            for (unsigned i = 0; i < rows; ++i) lane.digit_term((int)i, xu[2 * i], xu[2 * i + 1], k, lc);
        } else {
            const typename QpSumLane<Arith>::PTerm p = QpSumLane<Arith>::split_p(pmod);
            for (unsigned i = 0; i < rows; ++i) lane.p_term((int)i, xu[2 * i], xu[2 * i + 1], p, lc);
        }
    }
    lane.finish(lc);
    for (unsigned i = 0; i < rows; ++i) {
        out[4 * i + 0] = lane.r0[i][0]; out[4 * i + 1] = lane.r0[i][1];
        out[4 * i + 2] = lane.r1[i][0]; out[4 * i + 3] = lane.r1[i][1];
    }
}

// One word pair of one tile.  J terms per rotation; has_p: the last of them is the P c0 term (a data limb: Ld = J - 1), else every term is a digit term (the
// special limb: Ld = J).  x: [n_rot J][rows][2] canonical words, the gathered (and swapped) digit or c0 words of each term; keys: [n_rot J][4] canonical words
// (e0.a, e0.b, e1.a, e1.b; unread for a P term); out: [rows][2 components][2 halves] canonical words.
// returns 0, or 2000 on bad arguments (a policy that does not take q among them).
extern "C" int emu_rotate_sum(int cls, u64 q, u64 p_special, unsigned n_rot, int J, int has_p, unsigned rows, const u64* x, const u64* keys, u64* out) {
    if (!x || !keys || !out || n_rot == 0 || J < 1 || rows == 0 || rows > (unsigned)kQpSumTile || !emu_rotate_sum_takes(cls, q)) return 2000;
    const int Ld = has_p ? J - 1 : J;
    const LimbConst lc = limb_const_of_class(limb_const_of_modulus(q), (LimbClass)cls);
    if (cls == kClassFold) run<FoldArith>(lc, p_special, n_rot, J, Ld, rows, x, keys, out);
    else if (cls == kClassF64) run<F64Arith>(lc, p_special, n_rot, J, Ld, rows, x, keys, out);
    else if (cls == kClassFoldScaled) run<FoldScaledArith>(lc, p_special, n_rot, J, Ld, rows, x, keys, out);
    else if (cls == kClassF64Wide) run<F64WideArith>(lc, p_special, n_rot, J, Ld, rows, x, keys, out);
    else run<ShoupArith>(lc, p_special, n_rot, J, Ld, rows, x, keys, out);
    return 0;
}
