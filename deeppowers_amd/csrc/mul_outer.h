// mul_outer.h - the per-lane arithmetic of tensor3_outer_kernel (kernels_mul.h), host + device: one word position of the tensor products of ONE resident
// operand a with many streamed operands b (all pairs of A queries and B keys: the outer product),
//   (d0, d1, d2) = (a0 b0,  a0 b1 + a1 b0,  a1 b1)   mod q,      NTT domain, every word canonical in and out.
// Nothing here loads or stores: `prepare` is called ONCE per resident operand and returns the form of it that pays to keep in registers across its
// products, `product` once per pair.
// tools/emulate_mul_outer.cpp runs this very code on the CPU for every arithmetic policy, with DPFHE_EMU_CHECK armed (tests/test_emulated_mul_outer.py).
//
// Two forms:
//   MulOuterLane<Arith>      any policy with a canonical mul_var: the prepared form is the two words themselves, a product is four mul_var and one add_mod.
//                            No precondition beyond canonical words.  What the kernel runs on generic-prime contexts (ShoupArith).
//   MulOuterLane<FoldArith>  the prepared form is the operand's split30 halves (modarith.h: four 32-bit words, the same registers as the two 64-bit words,
//                            and the two splits are paid once per resident operand, not once per product); a product splits b's two words, runs its four
//                            partial-product chains on EMPTY Dot30 columns and folds each component once: 16 multiply-adds and THREE folds per product
//                            against mul_var's 28 and four - d1's two products go into one Dot30 and take one fold.
// Bounds of the lazy form, in units of 2^60 (q = 2^60 - d, d < 2^24; halves of a canonical word < 2^30, so a product of halves < 1):
//   every component starts from s0 = s1 = s2 = 0.  One product adds < 1 to s0, < 2 to s1 and < 1 to s2:
//     d0, d2 (one product):  s0 < 1, s1 < 2, s2 < 1;
//     d1 (two products):     before the second product s0 < 1, s1 < 2, s2 < 1 - inside dot30_mac's s0 < 15, s1 < 14, s2 < 15 -; after it s0 < 2, s1 < 4, s2 < 2.
//   dot30_fold0 wants s0 < 12 and s2 < 8: both hold with room to spare (the largest column, s1 < 4 = 2^62, does not wrap either).  Its result
//   < 2^60 + 16 d < 3 * 2^59 is what canon_small takes.  The columns are largest where the halves are: a canonical word's high half reaches 2^30 - 1 (at
//   q - 1, whose low half is 2^30 - d - 1) and its low half reaches 2^30 - 1 under a high half of 2^30 - 2 (at 2^60 - 2^30 - 1 < q): tests/mul_outer_ref.py
//   plants d1's pair on both words and on their mixtures.
#pragma once
#include "modarith.h"

namespace dpfhe {

constexpr int kMulOuterMidProducts = 2;   // products that share d1's Dot30 before its one fold
static_assert(kMulOuterMidProducts <= FoldArith::kDot30Period, "d1: its products fit one fold period from empty columns");

template <class Arith>
struct MulOuterLane {
    struct Prepared { u64 a0, a1; };
    static DPF_HD Prepared prepare(u64 a0, u64 a1, const LimbConst& c) {
        DPFHE_EMU_ASSERT(a0 < c.q && a1 < c.q);
        (void)c;
        return Prepared{a0, a1};
    }
    static DPF_HD void product(const Prepared& a, u64 b0, u64 b1, const LimbConst& c, u64& d0, u64& d1, u64& d2) {
        DPFHE_EMU_ASSERT(a.a0 < c.q && a.a1 < c.q && b0 < c.q && b1 < c.q);   // mul_var's and add_mod's: canonical words
        d0 = Arith::mul_var(a.a0, b0, c);
        d1 = add_mod(Arith::mul_var(a.a0, b1, c), Arith::mul_var(a.a1, b0, c), c.q);
        d2 = Arith::mul_var(a.a1, b1, c);
    }
};

template <>
struct MulOuterLane<FoldArith> {
    typedef FoldArith::Half30 Half30;
    typedef FoldArith::Dot30 Dot30;
    struct Prepared { Half30 a0, a1; };
    static DPF_HD Prepared prepare(u64 a0, u64 a1, const LimbConst& c) {
        DPFHE_EMU_ASSERT(a0 < c.q && a1 < c.q);   // split30: words < 2^60
        (void)c;
        return Prepared{FoldArith::split30(a0), FoldArith::split30(a1)};
    }
    static DPF_HD void product(const Prepared& a, u64 b0, u64 b1, const LimbConst& c, u64& d0, u64& d1, u64& d2) {
        DPFHE_EMU_ASSERT(b0 < c.q && b1 < c.q);
        const Half30 hb0 = FoldArith::split30(b0), hb1 = FoldArith::split30(b1);
        Dot30 s0{0, 0, 0}, s1{0, 0, 0}, s2{0, 0, 0};
        FoldArith::dot30_mac(s0, a.a0, hb0);
        FoldArith::dot30_mac(s1, a.a0, hb1);
        FoldArith::dot30_mac(s1, a.a1, hb0);
        FoldArith::dot30_mac(s2, a.a1, hb1);
        // the stated bounds: one product per outer component, kMulOuterMidProducts in the middle one
        DPFHE_EMU_ASSERT(s0.s0 < (1ull << 60) && s0.s1 < (2ull << 60) && s0.s2 < (1ull << 60));
        DPFHE_EMU_ASSERT(s1.s0 < (2ull << 60) && s1.s1 < (4ull << 60) && s1.s2 < (2ull << 60));
        DPFHE_EMU_ASSERT(s2.s0 < (1ull << 60) && s2.s1 < (2ull << 60) && s2.s2 < (1ull << 60));
        d0 = FoldArith::canon_small(FoldArith::dot30_fold0(s0, c), c);
        d1 = FoldArith::canon_small(FoldArith::dot30_fold0(s1, c), c);
        d2 = FoldArith::canon_small(FoldArith::dot30_fold0(s2, c), c);
    }
};

}  // namespace dpfhe
