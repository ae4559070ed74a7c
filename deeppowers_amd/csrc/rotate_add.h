// rotate_add.h - the last pass of one step of the rotate-and-add ladder (include/dpfhe.h dpfhe_rotate_add_hybrid): acc + rotate(acc, g) without ever
// materialising sigma_g(c0).  work: the key products of sigma_g(c1) over Q P (coefficient domain), (c0, c1): the step's input.
//
//   out.c0[k] = R(work.c0_i, work.c0_P; P)_i[k] + c0[k] + sigma_g(c0)[k]    mod q_i
//   out.c1[k] = R(work.c1_i, work.c1_P; P)_i[k] + c1[k]                     mod q_i        (R: fused_rescale.h rescale_word, the division by P)
//   sigma_g(a)[k] = +a[j] if j = k g^-1 mod 2N < N, else -a[j - N]                          (the signed gather of kernels_rotate.h galois_kernel)
//
// word for word what dpfhe_rotate_hybrid_grouped followed by dpfhe_add gives: every term is a canonical residue and so is every sum, whatever the order.
// The three-term sum is two full modular additions (3 q - 3 does not fit one conditional subtraction); the negation of 0 is 0.
//
// Shared by the device kernel (kernels_rotate.h rotate_add_pass_kernel) and the host twin below (dpfhe_rotate_add_pass_host): one statement of the
// arithmetic.  No HIP in here.
#pragma once
#include <stddef.h>

#include "fused_rescale.h"

namespace dpfhe {

// component 0: `src` is the word the gather found at j mod N, `negate` whether j >= N
template <class Arith>
DPF_HD u64 rotate_add_word0(u64 work_i, u64 work_p, u64 c0, u64 src, bool negate, const LimbConst& lc, const RescaleConst& rc) {
    const u64 rot = negate ? neg_mod(src, lc.q) : src;
    return add_mod(add_mod(rescale_word<Arith>(work_i, work_p, lc, rc), c0, lc.q), rot, lc.q);
}
// component 1
template <class Arith>
DPF_HD u64 rotate_add_word1(u64 work_i, u64 work_p, u64 c1, const LimbConst& lc, const RescaleConst& rc) {
    return add_mod(rescale_word<Arith>(work_i, work_p, lc, rc), c1, lc.q);
}

// ---- host twin: the same words, one coefficient at a time ------------------------------------------------------------------------------------------
// work: [batch][2][L][N] over Q P, in2: [batch][2][Ld][N], out: [batch][2][Ld][N];  lc: [L], rc: [L-1] relative to P;  g_inv = g^-1 mod 2N
template <class Arith>
inline void rotate_add_pass_host(size_t n, size_t L, const LimbConst* lc, const RescaleConst* rc, u64* out, const u64* work, const u64* in2, unsigned g_inv,
                                 size_t batch) {
    const size_t Ld = L - 1;
    const unsigned mask2n = 2u * (unsigned)n - 1u;
    for (size_t t = 0; t < batch; ++t)
        for (size_t i = 0; i < Ld; ++i) {
            const u64 *w0 = work + (t * 2 * L + i) * n, *p0 = work + (t * 2 * L + Ld) * n, *w1 = w0 + L * n, *p1 = p0 + L * n;
            const u64 *c0 = in2 + (t * 2 * Ld + i) * n, *c1 = c0 + Ld * n;
            u64 *o0 = out + (t * 2 * Ld + i) * n, *o1 = o0 + Ld * n;
            for (size_t k = 0; k < n; ++k) {
                const unsigned j = ((unsigned)k * g_inv) & mask2n;
                o0[k] = rotate_add_word0<Arith>(w0[k], p0[k], c0[k], c0[j & ((unsigned)n - 1u)], j >= (unsigned)n, lc[i], rc[i]);
                o1[k] = rotate_add_word1<Arith>(w1[k], p1[k], c1[k], lc[i], rc[i]);
            }
        }
}

}  // namespace dpfhe
