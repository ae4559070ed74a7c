// emulate_mul_outer.cpp - CPU emulation of tensor3_outer_kernel's per-lane code (TEST INFRASTRUCTURE, like emulate_mul_sum.cpp).
// Runs deeppowers_amd/csrc/mul_outer.h MulOuterLane<Arith> - the very code the kernel runs between its loads and its stores - for one word position and every
// arithmetic policy that takes the prime, with the precondition counter of the lazy products armed: the resident operand prepared once, then the streamed
// operands one after the other, as the kernel walks them.  Built by tests/test_emulated_mul_outer.py (g++), never shipped.
#define DPFHE_EMU_CHECK 1
#include <stddef.h>

#include "../deeppowers_amd/csrc/mul_outer.h"
#include "../deeppowers_amd/csrc/tables.h"

namespace dpfhe {
long g_emu_overflows = 0;
}
using namespace dpfhe;

extern "C" long emu_mul_outer_overflows() { return g_emu_overflows; }
// the products that share the middle component's columns before its one fold
extern "C" int emu_mul_outer_mid_products() { return kMulOuterMidProducts; }
// 1 when policy `cls` (tables.h LimbClass) takes the prime q
extern "C" int emu_mul_outer_takes(int cls, u64 q) {
    if (q < 3 || !(q & 1) || (q >> 60)) return 0;
    if (cls == kClassFold) return fold_eligible(q);
    if (cls == kClassF64) return f64_eligible(q);
    if (cls == kClassFoldScaled) return fold_scaled_shift(q) != 0;
    if (cls == kClassF64Wide) return q < (1ull << F64WideArith::kMaxBits);
    return cls == kClassShoup;
}

template <class Arith>
static void run(const LimbConst& lc, u64 a0, u64 a1, const u64* b0, const u64* b1, size_t keys, u64* out) {
    typedef MulOuterLane<Arith> Lane;
    const typename Lane::Prepared p = Lane::prepare(a0, a1, lc);
    for (size_t j = 0; j < keys; ++j) Lane::product(p, b0[j], b1[j], lc, out[3 * j], out[3 * j + 1], out[3 * j + 2]);
}

// a0, a1: the resident operand's canonical words of one position; b0, b1: [keys] canonical words of the streamed operands; out: [keys][3] canonical words.
// returns 0, or 2000 on bad arguments (a policy that does not take q among them).
extern "C" int emu_mul_outer(int cls, u64 q, u64 a0, u64 a1, const u64* b0, const u64* b1, size_t keys, u64* out) {
    if (!b0 || !b1 || !out || keys == 0 || !emu_mul_outer_takes(cls, q)) return 2000;
    const LimbConst lc = limb_const_of_class(limb_const_of_modulus(q), (LimbClass)cls);
    if (cls == kClassFold) run<FoldArith>(lc, a0, a1, b0, b1, keys, out);
    else if (cls == kClassF64) run<F64Arith>(lc, a0, a1, b0, b1, keys, out);
    else if (cls == kClassFoldScaled) run<FoldScaledArith>(lc, a0, a1, b0, b1, keys, out);
    else if (cls == kClassF64Wide) run<F64WideArith>(lc, a0, a1, b0, b1, keys, out);
    else run<ShoupArith>(lc, a0, a1, b0, b1, keys, out);
    return 0;
}
