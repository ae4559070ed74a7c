// compact.h - compact result ciphertexts: an exact switch of a 2-component ciphertext from Q = q_0 ... q_{L-1} to 2^k, then bit-packing.
//
//   out_c = round(2^k X / Q) mod 2^k  (k = k_c),  X in [0, Q) the CRT value of one coefficient's residues; Q is odd, so there is never a tie.
//   Write 2^k X = Q a + r with r CENTRED: a = round(2^k X / Q) and, mod 2^k, a = -r Q^-1.  r is the centred value of R = [2^k X]_Q, whose residues
//   are (2^k mod q_i) x_i mod q_i.  Per coefficient: one Shoup product per limb for those residues; the mixed-radix (Garner) digits of R,
//   v_0 = r_0, v_k = ((r_k - v_0) q_0^-1 - v_1) q_1^-1 ... mod q_k  (L(L-1)/2 Shoup products); R > floor(Q/2) (digits compared from the top) means
//   r = R - Q; R mod 2^64 by Horner with wrapping u64 arithmetic, minus Q mod 2^64 when centred; a mod 2^k = (-r Q^-1 mod 2^64) mod 2^k.
//
// Packing: item i's record starts at byte i N (k_0 + k_1) / 8; component 0 (N k_0 / 8 bytes), then component 1; value j of a component holds bits
// [j k, (j + 1) k) of the component's little-endian bit string (bit b = bit b mod 8 of byte b / 8).
//
// Shared by the device kernel (k_compact.hip) and the host twin (dpfhe_compact_host): one statement of the arithmetic.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "modarith.h"

namespace dpfhe {

constexpr u32 kCompactMaxLimbs = 10;             // the base-extension bound (kBxMaxSrc): a caller with more limbs rescales first
constexpr u32 kCompactMinBits = 8, kCompactMaxBits = 60;

struct CompactArgs {
    u64 q[kCompactMaxLimbs];
    u64 lift[kCompactMaxLimbs];                      // the smallest multiple of q_k >= 2^60: y + lift_k - v = y - v mod q_k, no wrap for any v < 2^60
    u64 inv[kCompactMaxLimbs][kCompactMaxLimbs];     // inv[k][i] = q_i^-1 mod q_k, i < k
    u64 inv_sh[kCompactMaxLimbs][kCompactMaxLimbs];  // floor(inv[k][i] 2^64 / q_k)
    u64 pow2[2][kCompactMaxLimbs];                   // 2^{k_c} mod q_i
    u64 pow2_sh[2][kCompactMaxLimbs];                // floor(pow2[c][i] 2^64 / q_i)
    u64 half[kCompactMaxLimbs];                      // mixed-radix digits of floor(Q / 2)
    u64 q64, qinv64;                                 // Q mod 2^64, Q^-1 mod 2^64
    u32 bits[2];                                     // k_0, k_1
    u32 n_limbs;
};
static_assert(sizeof(CompactArgs) + 64 <= 3400, "CompactArgs + the kernel's other arguments must stay inside the 4 KiB kernel-argument segment");

// y w mod q for any y < 2^64, w < q < 2^60, w_sh = floor(w 2^64 / q): the Shoup difference lies in [0, 2q)
DPF_HD u64 compact_shoup(u64 y, u64 w, u64 w_sh, u64 q) { return csub(y * w - mulhi64(y, w_sh) * q, q); }

// in place: residues r_i -> the Garner digits of their CRT value
template <int NL>
DPF_HD void compact_digits(u64 (&v)[NL], const CompactArgs& a) {
#pragma unroll
    for (int k = 1; k < NL; ++k)
#pragma unroll
        for (int i = 0; i < k; ++i) v[k] = compact_shoup(v[k] + a.lift[k] - v[i], a.inv[k][i], a.inv_sh[k][i], a.q[k]);
}

// round(2^{k_c} X / Q) mod 2^{k_c} for the residues x (canonical, or any word: they are taken mod q_i)
template <int NL>
DPF_HD u64 compact_value(const u64 (&x)[NL], int c, const CompactArgs& a) {
    u64 v[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) v[i] = compact_shoup(x[i], a.pow2[c][i], a.pow2_sh[c][i], a.q[i]);
    compact_digits<NL>(v, a);
    int cmp = 0;   // sign of R - floor(Q / 2), decided by the highest digit that differs
#pragma unroll
    for (int i = NL - 1; i >= 0; --i)
        if (cmp == 0) cmp = v[i] > a.half[i] ? 1 : (v[i] < a.half[i] ? -1 : 0);
    u64 r = v[NL - 1];
#pragma unroll
    for (int i = NL - 2; i >= 0; --i) r = r * a.q[i] + v[i];
    if (cmp > 0) r -= a.q64;
    return (0 - r * a.qinv64) & ((1ull << a.bits[c]) - 1);
}

// f(std::integral_constant<int, NL>) for NL = n_limbs in [1, kCompactMaxLimbs]; false for any other count
template <class F>
bool compact_with_limbs(u32 n_limbs, F&& f) {
    switch (n_limbs) {
    case 1: f(std::integral_constant<int, 1>{}); return true;
    case 2: f(std::integral_constant<int, 2>{}); return true;
    case 3: f(std::integral_constant<int, 3>{}); return true;
    case 4: f(std::integral_constant<int, 4>{}); return true;
    case 5: f(std::integral_constant<int, 5>{}); return true;
    case 6: f(std::integral_constant<int, 6>{}); return true;
    case 7: f(std::integral_constant<int, 7>{}); return true;
    case 8: f(std::integral_constant<int, 8>{}); return true;
    case 9: f(std::integral_constant<int, 9>{}); return true;
    case 10: f(std::integral_constant<int, 10>{}); return true;
    default: return false;
    }
}
static_assert(kCompactMaxLimbs == 10, "one case per limb count above");

// bytes of one item's record
DPF_HD size_t compact_record_bytes(u32 log2n, const CompactArgs& a) { return ((size_t)(a.bits[0] + a.bits[1]) << log2n) / 8; }

// host twin of the device launch (k_compact.hip launch_compact)
void compact_host(int log2n, uint8_t* out, const u64* in, size_t batch, const CompactArgs& a);

}  // namespace dpfhe
