// mul_complement.h - the per-lane arithmetic of tensor3_complement_kernel (kernels_mul.h), host + device: one word position of a group of tensor products
// that share the factor  f = (kappa - b0, -b1)  mod q  - the complement of a ciphertext b to the constant kappa (Goldschmidt's F = 2 - D at D's scale):
//   (d0, d1, d2) = (x0 f0,  x0 f1 + x1 f0,  x1 f1)   mod q,      NTT domain, every word canonical in and out.
// The transform of the constant polynomial kappa X^0 is kappa in every word, so f is formed from b's two words and the limb's kappa where they are, with no
// transform of its own.  Nothing here loads or stores: `factor` is called ONCE per group, `item` once per item of the group.
// tools/emulate_mul_complement.cpp runs this very code on the CPU for every arithmetic policy, with DPFHE_EMU_CHECK armed (tests/test_emulated_mul_complement.py).
//
// Canonicality of the factor: b0, b1, kappa in [0, q).  f0 = kappa - b0 when kappa >= b0, else kappa + q - b0: in [0, q) either way (sub_mod).  f1 = q - b1 for
// b1 != 0 and 0 for b1 = 0 (neg_mod): the negation of 0 is 0, not q - a word equal to q would break mul_var's and split30's precondition.
// The product: one MulSumLane term on an EMPTY accumulator (mul_sum.h): init(0, 0, 0) starts a period from s0 = s1 = s2 = 0, one term adds one product to
// d0 and d2 and two to d1 - inside every period stated there (8 products) -, finish folds and canonicalises.  On FoldArith that is 16 multiply-adds and three
// folds per item against mul_var's 28 and four folds; on the other policies it is mul_var + add_mod, canonical throughout.
#pragma once
#include "mul_sum.h"

namespace dpfhe {

template <class Arith>
struct MulComplementLane {
    struct Factor { u64 f0, f1; };
    static DPF_HD Factor factor(u64 b0, u64 b1, u64 kappa, const LimbConst& c) {
        DPFHE_EMU_ASSERT(b0 < c.q && b1 < c.q && kappa < c.q);
        const Factor f{sub_mod(kappa, b0, c.q), neg_mod(b1, c.q)};
        DPFHE_EMU_ASSERT(f.f0 < c.q && f.f1 < c.q);
        return f;
    }
    static DPF_HD void item(u64 x0, u64 x1, const Factor& f, const LimbConst& c, u64& d0, u64& d1, u64& d2) {
        typedef MulSumLane<Arith> Lane;
        typename Lane::Acc s = Lane::init(0, 0, 0, c);
        Lane::term(s, x0, x1, f.f0, f.f1, c);
        Lane::finish(s, c, d0, d1, d2);
    }
};

}  // namespace dpfhe
