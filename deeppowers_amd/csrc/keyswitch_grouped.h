// keyswitch_grouped.h - hybrid key switching with GROUPED digits and several special primes (include/dpfhe.h dpfhe_switch_key_grouped): the two kernels
// around the batched transforms and the key inner product.  Included by cabi_keyswitch_grouped.hip only.
//
// The extended context has L = Ld + alpha limbs, the last alpha of them special (product P).  Digit group d covers the data limbs [d alpha, min((d + 1) alpha, Ld)),
// product D_d; its digit is the CENTRED integer x_d in (-D_d / 2, D_d / 2], x_d = c mod D_d.  Both kernels are the arithmetic of base_ext.h - mixed-radix digits
//   v_0 = x_0,  v_k = ((x_k - v_0) q_0^-1 - v_1) q_1^-1 ... mod q_k,   X = v_0 + q_0 (v_1 + q_1 (...)),   centred by comparing the digits with those of floor(Qs / 2)
// - on its argument block BaseExtArgs, one block per digit group (source = the group, destination = all L limbs) and one for the division (source = the special
// limbs, destination = the data limbs, Q_inv = P^-1), in ONE device table per (context, alpha) that cabi_keyswitch_grouped.hip builds once with the host code
// of dpfhe_base_extend.  What is new is how the work is cut:
//   digit_group_lift_kernel   a thread owns a pair of coefficients of one (item, group): it reads the group's <= alpha rows ONCE, keeps the digits in registers
//                             and walks all L destination limbs: alpha rows read, L written per group, one launch for all items and groups (beta calls of
//                             dpfhe_base_extend re-read the sources per call and launch beta times);
//   grouped_moddown_kernel    a thread owns a pair of coefficients of one (item, component): the alpha special words are read and reconstructed ONCE, then
//                             every data limb takes (X_i - r) P^-1 and its addend in the same pass: 2 L rows read, (1 or 2) Ld addend rows, 2 Ld written per item.
// grouped_digits / grouped_residue below restate, per word, the digit and Horner loops that sit inline in kernels_bx.h's base_extend_kernel (it has no device
// function to call beyond bx_canon; moving these two there and having it call them is a follow-up that its own tests must prove).  Two of that header's remarks
// do not carry over: its argument block is a kernel ARGUMENT, which a reference would copy to scratch - here the blocks lie in global memory and a reference is a
// pointer (scalar loads); and its generic path stops at 8 sources because ONE loop nest over both words outgrows the unroller - here each word's loops are
// costed alone, and all of NS = 1 .. 10 build with ScratchSize 0.
// The number of source limbs is a template parameter for the reason kernels_bx.h gives (every index into the digit array is a compile-time constant); a short
// last group runs in the kernel of the full ones under workgroup-uniform `k < ns` predicates.  Generic arithmetic (ShoupArith::mul_var on the context's limb
// constants) on every limb, whatever classes the context's transforms run on: correct for every prime below 2^60, all words canonical in and out.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_bx.h"
#include "workmap.h"

namespace dpfhe {

constexpr int kGroupedMaxSpecial = 10;   // alpha <= kBxMaxSrc; L <= kBxMaxDst (the limits of the composition from dpfhe_base_extend / dpfhe_scale_round)
static_assert(kGroupedMaxSpecial == kBxMaxSrc, "a digit group is the source range of a BaseExtArgs");

// v[k]: residue modulo source limb k on entry (k < ns), mixed-radix digit k on return; returns X > floor(Qs / 2), i.e. the centred value is X - Qs.
// One word per call: the unroller costs each call's loops on their own.
template <int NS>
__device__ __forceinline__ bool grouped_digits(u64 (&v)[NS], const BaseExtArgs& a, const LimbConst* __restrict__ lcs, int ns) {
#pragma unroll
    for (int k = 1; k < NS; ++k) {
        if (k < ns) {
            const LimbConst lck = lcs[a.src_limb[k]];
            u64 t = v[k];
#pragma unroll
            for (int i = 0; i < k; ++i) t = ShoupArith::mul_var(sub_mod(t, bx_canon<ShoupArith>(v[i], lck), lck.q), a.inv[i][k], lck);
            v[k] = t;
        }
    }
    bool gt = false, decided = false;
#pragma unroll
    for (int k = NS - 1; k >= 0; --k)
        if (k < ns && !decided && v[k] != a.half[k]) { gt = v[k] > a.half[k]; decided = true; }
    return gt;
}

// the centred value modulo destination j of the block: Horner from the top digit
template <int NS>
__device__ __forceinline__ u64 grouped_residue(const u64 (&v)[NS], bool neg, const BaseExtArgs& a, int j, const LimbConst& lcj, int ns) {
    u64 acc = 0;
#pragma unroll
    for (int k = NS - 1; k >= 0; --k) {
        if (k == ns - 1) acc = bx_canon<ShoupArith>(v[k], lcj);
        else if (k < ns - 1) acc = add_mod(ShoupArith::mul_var(acc, a.q_mod[k][j], lcj), bx_canon<ShoupArith>(v[k], lcj), lcj.q);
    }
    return neg ? sub_mod(acc, a.Q_mod[j], lcj.q) : acc;
}

// digits [batch][groups][L][N] <- the centred digit of every group of component in_comps - 1 of in [batch][in_comps][n_data][N], on every limb.
// tabs[g]: the block of group g (n_src <= NS source limbs from src_limb[0], n_dst = L).
template <int NS>
__global__ __launch_bounds__(256) void digit_group_lift_kernel(u64* __restrict__ digits, const u64* __restrict__ in, int in_comps, const BaseExtArgs* __restrict__ tabs,
                                                               const LimbConst* __restrict__ lcs, int n_data, int n_limbs, unsigned groups, int n, int chunks) {
    const GroupLiftWork wk = GroupedKsMap::lift(blockIdx.x, groups, chunks);
    const int w0 = wk.chunk * 512 + threadIdx.x * 2;
    if (w0 >= n) return;
    const BaseExtArgs& a = tabs[wk.group];
    const int ns = a.n_src, s0 = a.src_limb[0];
    const u64* src = in + ((wk.item * in_comps + (in_comps - 1)) * n_data + s0) * (size_t)n + w0;
    u64* dst = digits + (wk.item * groups + wk.group) * (size_t)n_limbs * n + w0;
    u64 va[NS], vb[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        va[k] = vb[k] = 0;
        if (k < ns) {   // a limb of the group gets its own residue back: x_d = c (mod q_k)
            const U64x2 x = *reinterpret_cast<const U64x2*>(src + (size_t)k * n);
            *reinterpret_cast<U64x2*>(dst + (size_t)(s0 + k) * n) = x;
            va[k] = x.a; vb[k] = x.b;
        }
    }
    const bool na = grouped_digits<NS>(va, a, lcs, ns), nb = grouped_digits<NS>(vb, a, lcs, ns);
#pragma unroll 1
    for (int j = 0; j < n_limbs; ++j) {
        if (j >= s0 && j < s0 + ns) continue;
        const LimbConst lcj = lcs[j];
        *reinterpret_cast<U64x2*>(dst + (size_t)j * n) = U64x2{grouped_residue<NS>(va, na, a, j, lcj, ns), grouped_residue<NS>(vb, nb, a, j, lcj, ns)};
    }
}

// out [batch][2][n_data][N] <- round(work / P) + addend: work [batch][2][L][N] over Q P (coefficient domain), the addend the components of add_mask (bit c:
// component c; 1 after an automorphism, 3 for a relinearisation and for the hoisted slot sums, whose input has two components) of in [batch][in_comps][n_data][N].  a: the division's block (the NS = alpha special limbs as sources, the data limbs as destinations, Q_inv = P^-1).
// round(X / P) = (X - r) / P with r the centred remainder: dpfhe_scale_round with multiplier 1.
template <int NS>
__global__ __launch_bounds__(256) void grouped_moddown_kernel(u64* __restrict__ out, const u64* __restrict__ work, const u64* __restrict__ in, int in_comps,
                                                              int add_mask, const BaseExtArgs* __restrict__ tab, const LimbConst* __restrict__ lcs, int n_data, int n_limbs, int n,
                                                              int chunks) {
    const GroupedModdownWork wk = GroupedKsMap::moddown(blockIdx.x, chunks);
    const int w0 = wk.chunk * 512 + threadIdx.x * 2;
    if (w0 >= n) return;
    const BaseExtArgs& a = *tab;
    const u64* wp = work + (wk.item * 2 + wk.comp) * (size_t)n_limbs * n + w0;
    u64 va[NS], vb[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const U64x2 x = *reinterpret_cast<const U64x2*>(wp + (size_t)(n_data + k) * n);
        va[k] = x.a; vb[k] = x.b;
    }
    const bool na = grouped_digits<NS>(va, a, lcs, NS), nb = grouped_digits<NS>(vb, a, lcs, NS);
    const bool add = (add_mask >> wk.comp) & 1;
    const u64* cp = in + (wk.item * in_comps + wk.comp) * (size_t)n_data * n + w0;
    u64* op = out + (wk.item * 2 + wk.comp) * (size_t)n_data * n + w0;
#pragma unroll 1
    for (int j = 0; j < n_data; ++j) {
        const LimbConst lcj = lcs[j];
        const U64x2 x = *reinterpret_cast<const U64x2*>(wp + (size_t)j * n);
        U64x2 r{ShoupArith::mul_var(sub_mod(x.a, grouped_residue<NS>(va, na, a, j, lcj, NS), lcj.q), a.Q_inv[j], lcj),
                ShoupArith::mul_var(sub_mod(x.b, grouped_residue<NS>(vb, nb, a, j, lcj, NS), lcj.q), a.Q_inv[j], lcj)};
        if (add) {
            const U64x2 ad = *reinterpret_cast<const U64x2*>(cp + (size_t)j * n);
            r.a = add_mod(r.a, ad.a, lcj.q); r.b = add_mod(r.b, ad.b, lcj.q);
        }
        *reinterpret_cast<U64x2*>(op + (size_t)j * n) = r;
    }
}

}  // namespace dpfhe
