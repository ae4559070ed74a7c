// plain_add.h - adding a plaintext over Z_t to an exact (BFV-style) ciphertext: c0 += round(Q b / t) per limb.
//
//   Q = q_0 ... q_{L-1}, t odd and coprime to every q_l, b in [0, 2^32).  Mod q_l, Q = 0, so with r = Q b - t floor(Q b / t) taken CENTRED:
//       round(Q b / t) = (Q b - r) / t  =  -r t^-1  =  c t^-1   (mod q_l),   c = the centred representative in (-t/2, t/2) of -(Q mod t) b mod t.
//   t is odd, so Q b / t is never a half-integer and the rounding has no tie.  Subtracting b is adding round(Q (-b) / t) = -round(Q b / t): the same
//   formula with the multiplier Q mod t instead of -(Q mod t).  Per coefficient: y = m b mod t (m the multiplier, one Barrett reduction with
//   floor(2^64 / t)); c = y or y - t; per limb: c t^-1 = y t^-1 - [y > (t-1)/2]  (one Shoup product by t^-1 mod q_l).
//
// Shared by the device kernel (k_plain_add.hip) and the host twin (dpfhe_add_plain_scaled_host): one statement of the arithmetic.
#pragma once
#include <hip/hip_runtime.h>

#include "modarith.h"

namespace dpfhe {

struct PlainAddLimb {
    u64 q;
    u64 tinv;      // t^-1 mod q
    u64 tinv_sh;   // floor(tinv 2^64 / q)
};

constexpr u32 kPlainAddLimbs = 32;   // limbs per launch: their constants travel as a kernel argument

struct PlainAddArgs {
    u64 t;
    u64 t_mu;    // floor(2^64 / t)
    u64 m;       // -(Q mod t) mod t, or Q mod t to subtract
    u64 half;    // (t - 1) / 2: y > half means c = y - t
    u32 n_limbs; // limbs of this launch (<= kPlainAddLimbs), starting at limb `l0` of the context
    u32 l0;
    PlainAddLimb limb[kPlainAddLimbs];
};

// y = m b mod t, b < 2^32 and m < t < 2^32: the product fits 64 bits; the Barrett quotient is at most one short
DPF_HD u64 plain_add_residue(u64 b, const PlainAddArgs& a) {
    const u64 p = b * a.m;
    const u64 r = p - mulhi64(p, a.t_mu) * a.t;
    return csub(r, a.t);
}

// x + c t^-1 mod q for the y above; x a canonical residue
DPF_HD u64 plain_add_limb(u64 x, u64 y, const PlainAddLimb& c, bool hi) {
    u64 v = csub(y * c.tinv - mulhi64(y, c.tinv_sh) * c.q, c.q);   // Shoup: y t^-1 mod q (the difference lies in [0, 2q))
    if (hi) v = v ? v - 1 : c.q - 1;                                  // c = y - t:  c t^-1 = y t^-1 - 1
    return csub(x + v, c.q);
}

// host twin of the device launch (k_plain_add.hip launch_add_plain_scaled)
void add_plain_scaled_host(int log2n, u64* out, const u64* in, const u64* plain, size_t batch, u32 comps, u32 ctx_limbs, size_t group, const PlainAddArgs& a);

// ---- plaintext addition on residues (dpfhe_add_plain): the plaintext is an RNS polynomial of the ciphertext's own limbs and domain (an encoder's
// residue or NTT output), so c0 +- p needs no scaling - the approximate family's bias add, and a plain add in the exact family's NTT domain.
// x, p canonical: x + p, or x + (q - p), lies in [0, 2q) - one conditional subtraction (p = 0 subtracted: x + q - q = x)
DPF_HD u64 add_plain_word(u64 x, u64 p, u64 q, u32 negate) { return csub(x + (negate ? q - p : p), q); }

// host twin of the device launch (k_plain_add.hip launch_add_plain)
void add_plain_host(int log2n, const u64* moduli, u32 n_limbs, u64* out, const u64* in, const u64* plain, size_t batch, u32 comps, size_t group, bool negate);

}  // namespace dpfhe
