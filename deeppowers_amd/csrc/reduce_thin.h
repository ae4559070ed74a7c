// reduce_thin.h - the per-thread sum of reduce_thin_kernel (kernels_linalg.h), host + device: tools/emulate_reduce.cpp runs this very loop on
// the CPU with the wrap-around counter armed (tests/test_reduce_thin_cpu.py).  FoldArith limbs only (q = 2^60 - d, d < 2^24).
#pragma once
#include <stddef.h>

#include "modarith.h"

namespace dpfhe {

constexpr int kThinDepth = 5;    // 16-byte loads in flight per thread: 20 of the kernel's 32 registers (the kernel compiles to 30; six would need 34)
constexpr int kThinRounds = 2;   // rings of kThinDepth terms between two folds: 10 terms on top of a folded word (14 is the most the bound allows)
static_assert(kThinDepth * kThinRounds <= 14, "a folded word plus the terms of one pass must stay below 2^64");

// The word is added BEFORE its register is requested again.  Left alone hipcc moves every add of a pass behind all its loads and gives each load a
// register set of its own (68 registers); a scheduling barrier does not hold the adds either, they are reassociated before scheduling.  The empty
// statement takes the sums as operands and counts as a memory access: the adds stay in front of it, the next load behind it.
DPF_HD void thin_keep_order(u64& s0, u64& s1) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(s0), "+v"(s1) : : "memory");
#else
    (void)s0; (void)s1;
#endif
}

DPF_HD void thin_add(u64& s, u64 x) {
    DPFHE_EMU_ASSERT(s + x >= s);   // the lazy sum must not wrap around 2^64
    s += x;
}

// Sum of the CANONICAL words ld(lo) .. ld(hi - 1) (two adjacent words each) mod q, canonical.  Plain 64-bit adds, one
// FoldArith::reduce (3 instructions) per 10 terms, one canonicalisation at the end - against a compare-subtract-select per term.
// Bound: a folded word is < 2^60 + 15 d; k more terms below q = 2^60 - d make less than (k + 1) 2^60 + 15 d, below 2^64 up to k = 14; the
// fewer than kThinDepth terms of the ragged end come on top of a folded word.  The ring keeps kThinDepth loads in flight all the
// time: a word is added and its register re-requested at once, instead of a batch that drains before the next one starts.
template <class Load>
DPF_HD U64x2 thin_sum(Load ld, size_t lo, size_t hi, const LimbConst& lc) {
    u64 s0 = 0, s1 = 0;
    size_t it = lo;
    if (it + kThinDepth <= hi) {
        U64x2 v[kThinDepth];
#pragma unroll
        for (int u = 0; u < kThinDepth; ++u) v[u] = ld(it + u);
        it += kThinDepth;
        // kThinRounds rings and one fold per pass, as ONE basic block (with a fold behind a counter inside the loop hipcc sinks the
        // loads below that branch, behind all the adds: a batch that drains before the next one is requested)
        for (; it + kThinRounds * kThinDepth <= hi; it += kThinRounds * kThinDepth) {
#pragma unroll
            for (int u = 0; u < kThinRounds * kThinDepth; ++u) {
                thin_add(s0, v[u % kThinDepth].a); thin_add(s1, v[u % kThinDepth].b);
                thin_keep_order(s0, s1);
                v[u % kThinDepth] = ld(it + u);
            }
            s0 = FoldArith::reduce(s0, lc); s1 = FoldArith::reduce(s1, lc);
        }
        for (; it + kThinDepth <= hi; it += kThinDepth) {   // fewer than kThinRounds rings are left: with the ring's own terms at most kThinRounds of them
#pragma unroll
            for (int u = 0; u < kThinDepth; ++u) {
                thin_add(s0, v[u].a); thin_add(s1, v[u].b);
                thin_keep_order(s0, s1);
                v[u] = ld(it + u);
            }
        }
#pragma unroll
        for (int u = 0; u < kThinDepth; ++u) { thin_add(s0, v[u].a); thin_add(s1, v[u].b); }
        s0 = FoldArith::reduce(s0, lc); s1 = FoldArith::reduce(s1, lc);
    }
    for (; it < hi; ++it) {
        const U64x2 v = ld(it);
        thin_add(s0, v.a); thin_add(s1, v.b);
    }
    return U64x2{FoldArith::canon(s0, lc), FoldArith::canon(s1, lc)};
}

}  // namespace dpfhe
