// devtables.h - device-side table handles passed to the kernels by value, and the constants that shape the tables.
// No HIP: the host-side builder (ctx_tables.h) and tools/emulate.cpp read it as plain C++.
#pragma once
#include <stddef.h>

#include "modarith.h"

namespace dpfhe {

struct QuartersTop;   // ntt_quarters.h

// ---- the geometry constants that shape the tables (the launchers read them through launch.h) ----
// words-per-thread exponent of every kernel that runs a transform: 16 words per thread at every ring degree, so a context has ONE twiddle layout.
// Measured, closed: the fused kernels with 8 words per thread were slower (round 3 A/B); the batched transforms with 32 were equal at N = 8192 (3 phases
// against 4: same time, the kernels are VALU-bound), equal to slower at N = 4096 and 5 % slower on the forward transform at N = 16384 (round 4 A/B).
// (Geo / NttBody / pack_table keep their LOGE parameter: tests/test_emulated_kernels.py proves the address maps at other exponents too.)
constexpr int kLoge = 4;
constexpr int kMaxLog2N = 16;
// N = 16384 (128 KiB of LDS per polynomial): 1024 threads, one workgroup per CU; the fused kernels stop at N = 8192 (launch.h kMaxFusedLog2N).
// N > 16384: split transform - log2(N1) top stages in ntt_top_kernel, then N1 transforms of N2 = 4096 points each
constexpr int kSplitLog2N2 = 12;
constexpr int split_log_n1(int log2n) { return log2n > 14 ? log2n - kSplitLog2N2 : 0; }

template <class Tw>
struct InvLast {  // per limb: last inverse stage twiddles with N^-1 folded in
    Tw w_last;    // psi^-brv(1) * N^-1
    Tw w_ninv;    // N^-1
};

// Twiddle tables are stored in the layout of the kernel geometry that reads them (tables.h permute_window0): LOGE = kLoge above,
// for the batched transforms and the fused kernels alike.
template <class Arith>
struct DevTables {
    const typename Arith::Tw* fwd;          // [L][N]  psi^brv(i)
    const typename Arith::Tw* inv;          // [L][N]  psi^-brv(i)
    // split transform (N > 16384): fwd / inv / last then hold one N2-point table per (limb, block) - [L][n_sub][N2] and
    // [L][n_sub] - and the first log2(n_sub) stages run in ntt_top_kernel with these workgroup-uniform twiddles
    const typename Arith::Tw* top_fwd;      // [L][n_sub]  psi^brv(i), entry m + i of the full table, i < n_sub
    const typename Arith::Tw* top_inv;      // [L][n_sub]  psi^-brv(i)
    const InvLast<typename Arith::Tw>* top_last;  // [L]   last inverse stage with N^-1 folded in
    int n_sub;                              // 1: single-kernel transform
    // N = 8192 in "halves" form (ntt_halves.h; null at other ring degrees): per limb the two 4096-point sub-tree tables (roots 2 and 3 of the
    // N = 8192 table) in the (12, 4) kernel layout, the column stage's twiddle psi^brv(1), and the inverse column stage with N^-1 folded in
    const typename Arith::Tw* hfwd;         // [L][2][4096]
    const typename Arith::Tw* hinv;         // [L][2][4096]
    const typename Arith::Tw* htop_fwd;     // [L]
    const InvLast<typename Arith::Tw>* htop_last;  // [L]  {psi^-brv(1) N^-1, N^-1}
    // N = 16384 in "quarters" form (ntt_quarters.h; FoldArith contexts, null elsewhere): per limb the four 4096-point sub-tree tables (roots 4..7 of the
    // N = 16384 table) in the (12, 4) kernel layout, the forward column stages' twiddles, the inverse ones' (psi^-brv(2), psi^-brv(3)) and the last stage
    const typename Arith::Tw* qfwd;         // [L][4][4096]
    const typename Arith::Tw* qinv;         // [L][4][4096]
    const struct QuartersTop* qtop_fwd;     // [L]
    const typename Arith::Tw* qtop_inv;     // [L][2]
    const InvLast<typename Arith::Tw>* qtop_last;  // [L]  {psi^-brv(1) N^-1, N^-1}
    const InvLast<typename Arith::Tw>* last;  // [L]
    // FoldScaledArith class only: the same with s^-1 = 2^-(60-k) folded in - the last stage of an inverse transform whose input is a PRODUCT of two
    // scaled words (the fused multiply's lazy tensor step).  Null elsewhere.
    const InvLast<typename Arith::Tw>* last2;  // [L]
    // FoldArith at N = 4096 only (null elsewhere): the same tables and the last stage once more, every twiddle split at bit 29
    // (FoldArith::mul_tw29_add) - what ct_mul_quad_kernel's lazy transforms read.  A separate blob (ctx_tables.h build_lazy29_blob).
    const typename Arith::Tw* fwd29;        // [L][N]
    const typename Arith::Tw* inv29;        // [L][N]
    const InvLast<typename Arith::Tw>* last29;  // [L]
    const LimbConst* lc;                    // [L]
    int n_limbs;
    // Per-limb arithmetic classes (round 6, cabi.h dpfhe_ctx::classes): a launch may cover only SOME limbs of the context - those whose primes this policy
    // serves.  n_active = 0: all n_limbs limbs (the uniform contexts; block b works on limb b mod n_limbs).  Otherwise block b works on item
    // b / n_active and limb (active_map >> 4 (b mod n_active)) & 15; tables and data stay indexed by the limb's number in the context
    // (n_limbs = the stride), so a class's tables simply leave the other limbs' slots unused.  Contexts of more than 16 limbs are uniform.
    int n_active;
    unsigned long long active_map;
};

// (item, limb) of a workgroup of the transform / fused-multiply kernels; `blk` = blockIdx.x
template <class TB>
DPF_HD void block_item_limb(const TB& tb, size_t blk, size_t& item, int& limb) {
    if (tb.n_active) {
        item = blk / (unsigned)tb.n_active;
        limb = (int)((tb.active_map >> (4u * (unsigned)(blk % (unsigned)tb.n_active))) & 15u);
    } else {
        item = blk / (unsigned)tb.n_limbs;
        limb = (int)(blk % (unsigned)tb.n_limbs);
    }
}

// limb number of index i among the limbs a launch works on (all limbs, or one class through its active_map): what a work map's limb index means
template <class TB>
DPF_HD int launch_limb(const TB& tb, unsigned i) {
    return tb.n_active ? (int)((tb.active_map >> (4u * i)) & 15u) : (int)i;
}

// (polynomial, limb, sub-block) of a workgroup of the batched transforms: block p transforms words [p N, (p + 1) N) - one polynomial, or one of its n_sub
// blocks (SUB = false: kernels that only run with n_sub = 1) -, or, in a launch over one arithmetic class (n_active; n_sub = 1), the class's limb of its item
struct TransformBlock {
    size_t p, sub;
    int limb;
};
template <bool SUB = true, class TB>
DPF_HD TransformBlock transform_block(const TB& tb, size_t blk) {
    size_t p = blk;
    const size_t sub = SUB ? p % (size_t)tb.n_sub : 0;
    int limb = (int)((SUB ? p / (size_t)tb.n_sub : p) % (size_t)tb.n_limbs);
    if (tb.n_active) {
        size_t item;
        block_item_limb(tb, blk, item, limb);
        p = item * (size_t)tb.n_limbs + (size_t)limb;
    }
    return TransformBlock{p, sub, limb};
}

// the batched transforms' view of a context with per-limb arithmetic classes (kernels.h ntt_classes_kernel, ctx_tables.h mixed_layout)
struct MixedTables {
    const void* fwd;            // [L][N] twiddles, slot l in limb l's format, kernel layout of the batched transforms
    const void* inv;
    const void* last;           // [L] InvLast
    const LimbConst* lc;        // [L], each as its class reads it (tables.h limb_const_of_class)
    int n_limbs;
    unsigned long long cls_map; // 4 bits per limb: tables.h LimbClass
};

// per limb below the last: the constants of the rescale / modulus switch to the next level (kernels_keyswitch.h rescale_kernel), relative to the LAST prime
struct RescaleConst {
    u64 h_mod;     // floor(q_last / 2) mod q_i
    u64 inv;       // q_last^-1 mod q_i
    u64 q_last;
    u64 h;         // floor(q_last / 2)
};

}  // namespace dpfhe
