// emulate_mul_complement.cpp - CPU emulation of tensor3_complement_kernel's per-lane code (TEST INFRASTRUCTURE, like emulate_mul_sum.cpp).
// Runs deeppowers_amd/csrc/mul_complement.h MulComplementLane<Arith> - the very code the kernel runs between its loads and its stores - for one word position of
// one group and every arithmetic policy that takes the prime, with the precondition counter of the lazy products armed: the factor once, then the group's
// items one after the other, as the kernel walks them.  Built by tests/test_emulated_mul_complement.py (g++), never shipped.
#define DPFHE_EMU_CHECK 1
#include <stddef.h>

#include "../deeppowers_amd/csrc/mul_complement.h"
#include "../deeppowers_amd/csrc/tables.h"

namespace dpfhe {
long g_emu_overflows = 0;
}
using namespace dpfhe;

extern "C" long emu_mul_complement_overflows() { return g_emu_overflows; }
// 1 when policy `cls` (tables.h LimbClass) takes the prime q
extern "C" int emu_mul_complement_takes(int cls, u64 q) {
    if (q < 3 || !(q & 1) || (q >> 60)) return 0;
    if (cls == kClassFold) return fold_eligible(q);
    if (cls == kClassF64) return f64_eligible(q);
    if (cls == kClassFoldScaled) return fold_scaled_shift(q) != 0;
    if (cls == kClassF64Wide) return q < (1ull << F64WideArith::kMaxBits);
    return cls == kClassShoup;
}

template <class Arith>
static void run(const LimbConst& lc, const u64* x0, const u64* x1, size_t items, u64 b0, u64 b1, u64 kappa, u64* factor, u64* out) {
    typedef MulComplementLane<Arith> Lane;
    const typename Lane::Factor f = Lane::factor(b0, b1, kappa, lc);
    factor[0] = f.f0; factor[1] = f.f1;
    for (size_t k = 0; k < items; ++k) Lane::item(x0[k], x1[k], f, lc, out[3 * k], out[3 * k + 1], out[3 * k + 2]);
}

// x0, x1: [items] canonical words of one position (the group's numerators, and b's own words last when the self product is wanted); b0, b1, kappa: the
// canonical words the factor is formed from; factor: the two words of f; out: [items][3] canonical words.  returns 0, or 2000 on bad arguments (a policy
// that does not take q among them).
extern "C" int emu_mul_complement(int cls, u64 q, const u64* x0, const u64* x1, size_t items, u64 b0, u64 b1, u64 kappa, u64* factor, u64* out) {
    if (!x0 || !x1 || !factor || !out || items == 0 || !emu_mul_complement_takes(cls, q)) return 2000;
    const LimbConst lc = limb_const_of_class(limb_const_of_modulus(q), (LimbClass)cls);
    if (cls == kClassFold) run<FoldArith>(lc, x0, x1, items, b0, b1, kappa, factor, out);
    else if (cls == kClassF64) run<F64Arith>(lc, x0, x1, items, b0, b1, kappa, factor, out);
    else if (cls == kClassFoldScaled) run<FoldScaledArith>(lc, x0, x1, items, b0, b1, kappa, factor, out);
    else if (cls == kClassF64Wide) run<F64WideArith>(lc, x0, x1, items, b0, b1, kappa, factor, out);
    else run<ShoupArith>(lc, x0, x1, items, b0, b1, kappa, factor, out);
    return 0;
}
