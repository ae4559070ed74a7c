// expand.h - the uniform half of seeded ciphertexts and keys: expand(seed, item, limb, component), a wire format.
//
//   ChaCha20 block function exactly as in RFC 8439 section 2.3 (chacha20.h): constants | key = the 32-byte seed as 8 little-endian words |
//   word 12 = 32-bit block counter | words 13..15 = nonce, here (item, limb, component).  Coefficient k of the polynomial takes
//   block k / 4, output words 4 (k mod 4) .. 4 (k mod 4) + 3, read as ONE 128-bit little-endian integer X, and is X mod q_limb.
//   The statistical distance from uniform is at most q / 2^128 < 2^-68 per coefficient; there is no rejection step.
//   `limb` is the limb's index in the context, so the first m limbs of an expansion do not depend on the limbs after them
//   (a level made by dropping the last limb re-expands the same words).  The same words serve both domains.
//
// Security: the seed is PUBLIC (it replaces a public uniform polynomial); what rests on it is ChaCha20 as a PRG with a public
// seed.  A seed must never be reused under one secret key: equal c1 would make c0 - c0' = Delta (m - m') + e - e' public.
//
// Shared by the device kernel (k_expand.hip) and the host twin (dpfhe_expand_uniform_host): one statement of the format.
#pragma once
#include <hip/hip_runtime.h>

#include "chacha20.h"
#include "modarith.h"

namespace dpfhe {

// X = hi 2^64 + lo  ->  X mod q, exact for ANY X < 2^128 (q < 2^60; br = floor(2^128 / q) = br_hi 2^64 + br_lo, LimbConst).
// Barrett: floor(X br / 2^128) >= floor(X / q) - 1 since br > 2^128 / q - 1 and X < 2^128.  The estimate below is
// hi br_hi + floor((hi br_lo + lo br_hi) / 2^64): it drops lo br_lo / 2^128 < 1, so qhat >= floor(X / q) - 2, hence
// r = X - qhat q lies in [0, 3q) - it fits 64 bits and is computed modulo 2^64 - and two conditional subtractions finish it.
DPF_HD u64 reduce128(u64 lo, u64 hi, u64 q, u64 br_hi, u64 br_lo) {
    const u64 t1lo = lo * br_hi, t1hi = mulhi64(lo, br_hi);
    const u64 t2lo = hi * br_lo, t2hi = mulhi64(hi, br_lo);
    const u64 s = t1lo + t2lo;
    const u64 qhat = hi * br_hi + t1hi + t2hi + (s < t1lo ? 1u : 0u);
    u64 r = lo - qhat * q;
    r = csub(r, 2 * q);
    return csub(r, q);
}

// the four coefficients 4 j .. 4 j + 3 of one (item, limb, component) block, j = the block counter
DPF_HD void expand_block(const ExpandKey& k, u32 j, u32 item, u32 limb, u32 comp, u64 q, u64 br_hi, u64 br_lo, u64 out[4]) {
    u32 w[16];
    chacha20_block(k, j, item, limb, comp, w);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int m = 0; m < 4; ++m) {
        const u64 lo = (u64)w[4 * m] | ((u64)w[4 * m + 1] << 32), hi = (u64)w[4 * m + 2] | ((u64)w[4 * m + 3] << 32);
        out[m] = reduce128(lo, hi, q, br_hi, br_lo);
    }
}

// host twin of the device launch (k_expand.hip launch_expand_uniform): every other word untouched
void expand_uniform_host(int log2n, const u64* moduli, u32 n_limbs, u64* out, size_t batch, size_t comps, u32 comp, const ExpandKey& key, u32 first_item);

}  // namespace dpfhe
