// emulate_mul_sum.cpp - CPU emulation of tensor3_sum_kernel's per-lane code (TEST INFRASTRUCTURE, like emulate_reduce.cpp).
// Runs deeppowers_amd/csrc/mul_sum.h MulSumLane<Arith> - the very code the kernel runs between its loads and its stores - for one word position and every
// arithmetic policy that takes the prime, with the precondition counter of the lazy sums armed.  Built by tests/test_emulated_mul_sum.py (g++), never shipped.
#define DPFHE_EMU_CHECK 1
#include <stddef.h>

#include "../deeppowers_amd/csrc/mul_sum.h"
#include "../deeppowers_amd/csrc/tables.h"

namespace dpfhe {
long g_emu_overflows = 0;
}
using namespace dpfhe;

extern "C" long emu_mul_sum_overflows() { return g_emu_overflows; }
// the declared fold periods, in PRODUCTS: which = 0 the outer components (one product per term), 1 the middle one (two per term)
extern "C" int emu_mul_sum_period(int which) { return which == 0 ? kMulSumOuterPeriod : kMulSumMidPeriod; }
// 1 when policy `cls` (tables.h LimbClass) takes the prime q
extern "C" int emu_mul_sum_takes(int cls, u64 q) {
    if (q < 3 || !(q & 1) || (q >> 60)) return 0;
    if (cls == kClassFold) return fold_eligible(q);
    if (cls == kClassF64) return f64_eligible(q);
    if (cls == kClassFoldScaled) return fold_scaled_shift(q) != 0;
    if (cls == kClassF64Wide) return q < (1ull << F64WideArith::kMaxBits);
    return cls == kClassShoup;
}

template <class Arith>
static void run(const LimbConst& lc, const u64* a0, const u64* a1, const u64* b0, const u64* b1, size_t terms, const u64* prev, u64* out) {
    typedef MulSumLane<Arith> Lane;
    typename Lane::Acc s = Lane::init(prev ? prev[0] : 0, prev ? prev[1] : 0, prev ? prev[2] : 0, lc);
    for (size_t k = 0; k < terms; ++k) Lane::term(s, a0[k], a1[k], b0[k], b1[k], lc);
    Lane::finish(s, lc, out[0], out[1], out[2]);
}

// a0, a1, b0, b1: [terms] canonical words of one position; prev: null, or the three canonical words the sum continues from (the kernel's `accumulate`);
// out: the three canonical words.  returns 0, or 2000 on bad arguments (a policy that does not take q among them).
extern "C" int emu_mul_sum(int cls, u64 q, const u64* a0, const u64* a1, const u64* b0, const u64* b1, size_t terms, const u64* prev, u64* out) {
    if (!a0 || !a1 || !b0 || !b1 || !out || terms == 0 || !emu_mul_sum_takes(cls, q)) return 2000;
    const LimbConst lc = limb_const_of_class(limb_const_of_modulus(q), (LimbClass)cls);
    if (cls == kClassFold) run<FoldArith>(lc, a0, a1, b0, b1, terms, prev, out);
    else if (cls == kClassF64) run<F64Arith>(lc, a0, a1, b0, b1, terms, prev, out);
    else if (cls == kClassFoldScaled) run<FoldScaledArith>(lc, a0, a1, b0, b1, terms, prev, out);
    else if (cls == kClassF64Wide) run<F64WideArith>(lc, a0, a1, b0, b1, terms, prev, out);
    else run<ShoupArith>(lc, a0, a1, b0, b1, terms, prev, out);
    return 0;
}
