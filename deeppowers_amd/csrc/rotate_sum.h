// rotate_sum.h - the per-lane arithmetic of hoisted_qp_sum_kernel (kernels_rotate_sum.h), host + device: ONE word pair (the two halves h = 0, 1 of a 16-byte
// pair) of one limb of the running sums of a tile of up to kQpSumTile items over the R J terms of dpfhe_rotate_sum_hoisted,
//   S.c0 = sum_r ( sum_{j<Ld} x_{r,j} key_{r,j,0} + P c_r ),   S.c1 = sum_r sum_{j<Ld} x_{r,j} key_{r,j,1}      mod q, every word canonical in and out,
// x the gathered (and swapped) digit words of the rotation, c the gathered c0 words (data limbs only: J = Ld + 1 there, Ld on the special limb).
// Nothing here loads, maps or stores: the kernel calls `begin_term` once per term (workgroup-uniform), then `digit_term` or `p_term` per live row, and
// `finish` once.  tools/emulate_rotate_sum.cpp runs this very code on the CPU for every arithmetic policy, with DPFHE_EMU_CHECK armed
// (tests/test_emulated_rotate_sum.py).
//
// Two forms:
//   QpSumLane<Arith>      any policy with a canonical mul_var: canonical running sums, a term is mul_var + add_mod per word.  No precondition beyond
//                         canonical words.  The kernel is launched with ShoupArith (every context that is not all-fold) and FoldArith only
//                         (cabi.h with_ctx_arith); the F64, FoldScaled and F64Wide lanes are run by the emulator alone.
//   QpSumLane<FoldArith>  lazy Dot30 columns (modarith.h) beside a folded running word per sum: a term is 4 multiply-adds per word and nothing else; the
//                         columns are folded into the running word when kDot30Period terms have gone into them, counted ACROSS rotations and whatever the
//                         kind of term (component 1 skips the P term and so holds at most as many).  A key pair is split once for the whole tile, a digit
//                         word's split serves both key components.
// Bounds of the lazy form, in units of 2^60 (halves of a canonical word < 2^30, so a product of halves < 1): a term adds < 1 to s0, < 2 to s1, < 1 to s2.
// Before the k-th term of a period (k = 1 .. 8) s0 < k - 1, s1 < 2 (k - 1), s2 < k - 1: at k = 8 exactly dot30_mac's s0 < 15, s1 < 14, s2 < 15.  After the
// eighth s1 < 16 = 2^64, the capacity of the column: 8 * 2 * (2^30 - 1)^2 < 2^64 <= 9 * 2 * (2^30 - 1)^2, so a period of nine would wrap on the words whose
// halves are largest (q - 1: high half 2^30 - 1; 2^60 - 2^30 - 1: low half 2^30 - 1) - tests/rotate_sum_ref.py plants them.  dot30_fold takes a running word
// < 2^60 + 2^29 and returns one < 2^60 + 16 d < 2^60 + 2^28, which is also what canon_small (< 3 * 2^59) takes at the end.
#pragma once
#include "modarith.h"
#include "workmap.h"

namespace dpfhe {

template <class Arith>
struct QpSumLane {
    static constexpr int TI = kQpSumTile;
    struct Key { u64 k0a, k0b, k1a, k1b; };   // key component 0's and 1's words under halves a and b
    typedef u64 PTerm;
    u64 r0[TI][2], r1[TI][2];                  // the canonical running sums

    DPF_HD void clear() {
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) { r0[i][h] = 0; r1[i][h] = 0; }
    }
    // P mod q, canonical (the generic Barrett product: every limb constant carries its ratio)
    static DPF_HD u64 p_operand(u64 p_special, const LimbConst& c) { return ShoupArith::mul_var(p_special, 1, c); }
    DPF_HD void begin_term(const LimbConst&) {}
    static DPF_HD Key split_key(u64 e0a, u64 e0b, u64 e1a, u64 e1b) { return Key{e0a, e0b, e1a, e1b}; }
    static DPF_HD PTerm split_p(u64 pmod) { return pmod; }
    static DPF_HD u64 accw(u64 acc, u64 a, u64 b, const LimbConst& c) {
        DPFHE_EMU_ASSERT(acc < c.q && a < c.q && b < c.q);
        return add_mod(acc, Arith::mul_var(a, b, c), c.q);
    }
    DPF_HD void digit_term(int i, u64 xa, u64 xb, const Key& k, const LimbConst& c) {
        r0[i][0] = accw(r0[i][0], xa, k.k0a, c); r0[i][1] = accw(r0[i][1], xb, k.k0b, c);
        r1[i][0] = accw(r1[i][0], xa, k.k1a, c); r1[i][1] = accw(r1[i][1], xb, k.k1b, c);
    }
    DPF_HD void p_term(int i, u64 xa, u64 xb, const PTerm& p, const LimbConst& c) {
        r0[i][0] = accw(r0[i][0], xa, p, c); r0[i][1] = accw(r0[i][1], xb, p, c);
    }
    DPF_HD void finish(const LimbConst&) {}
};

template <>
struct QpSumLane<FoldArith> {
    static constexpr int TI = kQpSumTile;
    typedef FoldArith::Half30 Half30;
    typedef FoldArith::Dot30 Dot30;
    struct Key { Half30 k0a, k0b, k1a, k1b; };
    typedef Half30 PTerm;
    Dot30 s0[TI][2], s1[TI][2];                // the lazy columns of the current period ...
    u64 r0[TI][2], r1[TI][2];                  // ... and the folded running words (canonical after finish)
    int terms;                                 // terms gone into the columns since the last fold

    DPF_HD void clear() {
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) { s0[i][h] = Dot30{0, 0, 0}; s1[i][h] = Dot30{0, 0, 0}; r0[i][h] = 0; r1[i][h] = 0; }
        terms = 0;
    }
    static DPF_HD u64 p_operand(u64 p_special, const LimbConst& c) { return FoldArith::canon(p_special, c); }
    DPF_HD void fold_all(const LimbConst& c) {
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                r0[i][h] = FoldArith::dot30_fold(s0[i][h], r0[i][h], c); s0[i][h] = Dot30{0, 0, 0};
                r1[i][h] = FoldArith::dot30_fold(s1[i][h], r1[i][h], c); s1[i][h] = Dot30{0, 0, 0};
            }
        terms = 0;
    }
    // once per term, before its rows: the fold that makes room for it
    DPF_HD void begin_term(const LimbConst& c) {
        if (terms == FoldArith::kDot30Period) fold_all(c);
        ++terms;
        DPFHE_EMU_ASSERT(terms >= 1 && terms <= FoldArith::kDot30Period);
    }
    // all operands are canonical residues (< 2^60), which is what split30 needs
    static DPF_HD Key split_key(u64 e0a, u64 e0b, u64 e1a, u64 e1b) {
        return Key{FoldArith::split30(e0a), FoldArith::split30(e0b), FoldArith::split30(e1a), FoldArith::split30(e1b)};
    }
    static DPF_HD PTerm split_p(u64 pmod) { return FoldArith::split30(pmod); }
    DPF_HD void digit_term(int i, u64 xa, u64 xb, const Key& k, const LimbConst&) {
        const Half30 ha = FoldArith::split30(xa), hb = FoldArith::split30(xb);
        FoldArith::dot30_mac(s0[i][0], ha, k.k0a);
        FoldArith::dot30_mac(s0[i][1], hb, k.k0b);
        FoldArith::dot30_mac(s1[i][0], ha, k.k1a);
        FoldArith::dot30_mac(s1[i][1], hb, k.k1b);
    }
    DPF_HD void p_term(int i, u64 xa, u64 xb, const PTerm& p, const LimbConst&) {
        FoldArith::dot30_mac(s0[i][0], FoldArith::split30(xa), p);
        FoldArith::dot30_mac(s0[i][1], FoldArith::split30(xb), p);
    }
    DPF_HD void finish(const LimbConst& c) {
        fold_all(c);
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) { r0[i][h] = FoldArith::canon_small(r0[i][h], c); r1[i][h] = FoldArith::canon_small(r1[i][h], c); }
    }
};

}  // namespace dpfhe
