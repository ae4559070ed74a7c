// mul_sum.h - the per-lane arithmetic of tensor3_sum_kernel (kernels_mul.h), host + device: one word position of a sum of ciphertext tensor products
//   (d0, d1, d2) = sum_k (a0_k b0_k,  a0_k b1_k + a1_k b0_k,  a1_k b1_k)   mod q,      NTT domain, every word canonical in and out.
// Nothing here loads or stores: `term` takes the four words of one pair and updates the running sums, `finish` returns the canonical words.
// tools/emulate_mul_sum.cpp runs this very code on the CPU for every arithmetic policy, with DPFHE_EMU_CHECK armed (tests/test_emulated_mul_sum.py).
//
// Two forms:
//   MulSumLane<Arith>      any policy with a canonical mul_var: the sums stay canonical (mul_var + add_mod per product).  No period, no precondition
//                          beyond canonical words.  What the kernel runs on generic-prime contexts (ShoupArith).
//   MulSumLane<FoldArith>  lazy: each sum is a Dot30 column triple (modarith.h: four multiply-adds per product and nothing else) whose s0 column also
//                          carries the running folded word, refolded by dot30_fold0 every kMulSumOuterPeriod / kMulSumMidPeriod PRODUCTS.  16 multiply-adds
//                          per term against mul_var's 28 and four folds.
// Bounds of the lazy form, in units of 2^60 (q = 2^60 - d, d < 2^24; halves of a canonical word < 2^30, so a product of halves < 1):
//   a period starts from s0 < 1 + 2^-32 (a canonical word, or dot30_fold0's result < 2^60 + 16 d) and s1 = s2 = 0;
//   p products later s0 < 1 + 2^-32 + p, s1 < 2 p, s2 < p.  dot30_mac wants s0 < 15, s1 < 14, s2 < 15 BEFORE a product: p <= 7 there, i.e. at most 8
//   products per period, after which s1 < 16 = 2^64 (no wrap); dot30_fold0 wants s0 < 12 and s2 < 8: p <= 8.  Hence both periods = kDot30Period = 8.
//   d0 and d2 take one product per term, d1 takes TWO: its period of 8 products is 4 terms.
#pragma once
#include "modarith.h"

namespace dpfhe {

constexpr int kMulSumOuterPeriod = FoldArith::kDot30Period;   // products between two folds of d0 (and of d2): one per term
constexpr int kMulSumMidPeriod = FoldArith::kDot30Period;     // products between two folds of d1: two per term
constexpr int kMulSumMidPerTerm = 2;
static_assert(kMulSumOuterPeriod >= 1 && kMulSumOuterPeriod <= 8, "d0 / d2: at most 8 products on top of a folded word (dot30_mac: s1 < 14 * 2^60 before a product)");
static_assert(kMulSumMidPeriod >= kMulSumMidPerTerm && kMulSumMidPeriod <= 8, "d1: at most 8 products on top of a folded word, and room for one term");

template <class Arith>
struct MulSumLane {
    struct Acc { u64 d0, d1, d2; };
    // prev: the canonical words a sum continues from (zeros for a new sum)
    static DPF_HD Acc init(u64 p0, u64 p1, u64 p2, const LimbConst& c) {
        DPFHE_EMU_ASSERT(p0 < c.q && p1 < c.q && p2 < c.q);
        (void)c;
        return Acc{p0, p1, p2};
    }
    static DPF_HD void term(Acc& s, u64 a0, u64 a1, u64 b0, u64 b1, const LimbConst& c) {
        DPFHE_EMU_ASSERT(a0 < c.q && a1 < c.q && b0 < c.q && b1 < c.q);   // mul_var's and add_mod's: canonical words
        s.d0 = add_mod(s.d0, Arith::mul_var(a0, b0, c), c.q);
        s.d1 = add_mod(s.d1, add_mod(Arith::mul_var(a0, b1, c), Arith::mul_var(a1, b0, c), c.q), c.q);
        s.d2 = add_mod(s.d2, Arith::mul_var(a1, b1, c), c.q);
    }
    static DPF_HD void finish(const Acc& s, const LimbConst&, u64& d0, u64& d1, u64& d2) { d0 = s.d0; d1 = s.d1; d2 = s.d2; }
};

template <>
struct MulSumLane<FoldArith> {
    typedef FoldArith::Dot30 Dot30;
    struct Acc {
        Dot30 d0, d1, d2;
        int n_outer, n_mid;   // products since the last fold (uniform over the workgroup: the term loop is)
    };
    static DPF_HD Acc init(u64 p0, u64 p1, u64 p2, const LimbConst& c) {
        DPFHE_EMU_ASSERT(p0 < c.q && p1 < c.q && p2 < c.q);   // a period starts from s0 < 2^60 + 2^28
        (void)c;
        return Acc{Dot30{p0, 0, 0}, Dot30{p1, 0, 0}, Dot30{p2, 0, 0}, 0, 0};
    }
    static DPF_HD void refold(Dot30& s, const LimbConst& c) { s = Dot30{FoldArith::dot30_fold0(s, c), 0, 0}; }
    static DPF_HD void term(Acc& s, u64 a0, u64 a1, u64 b0, u64 b1, const LimbConst& c) {
        DPFHE_EMU_ASSERT(a0 < c.q && a1 < c.q && b0 < c.q && b1 < c.q);                                                 // split30: words < 2^60
        DPFHE_EMU_ASSERT(s.n_outer + 1 <= kMulSumOuterPeriod && s.n_mid + kMulSumMidPerTerm <= kMulSumMidPeriod);      // room for this term's products
        const FoldArith::Half30 ha0 = FoldArith::split30(a0), ha1 = FoldArith::split30(a1), hb0 = FoldArith::split30(b0), hb1 = FoldArith::split30(b1);
        FoldArith::dot30_mac(s.d0, ha0, hb0);
        FoldArith::dot30_mac(s.d1, ha0, hb1);
        FoldArith::dot30_mac(s.d1, ha1, hb0);
        FoldArith::dot30_mac(s.d2, ha1, hb1);
        s.n_outer += 1;
        s.n_mid += kMulSumMidPerTerm;
        if (s.n_mid + kMulSumMidPerTerm > kMulSumMidPeriod) { refold(s.d1, c); s.n_mid = 0; }                          // no room for another term's two products
        if (s.n_outer + 1 > kMulSumOuterPeriod) { refold(s.d0, c); refold(s.d2, c); s.n_outer = 0; }
    }
    static DPF_HD void finish(const Acc& s, const LimbConst& c, u64& d0, u64& d1, u64& d2) {
        // dot30_fold0: s0 < 12 * 2^60 and s2 < 2^63 hold anywhere inside a period; its result < 2^60 + 16 d < 3 * 2^59 is what canon_small takes
        d0 = FoldArith::canon_small(FoldArith::dot30_fold0(s.d0, c), c);
        d1 = FoldArith::canon_small(FoldArith::dot30_fold0(s.d1, c), c);
        d2 = FoldArith::canon_small(FoldArith::dot30_fold0(s.d2, c), c);
    }
};

}  // namespace dpfhe
