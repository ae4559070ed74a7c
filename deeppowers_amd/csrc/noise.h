// noise.h - secret-seeded noise polynomials for re-randomising result ciphertexts: noise(seed, item, stream_id, kind, param).
//
//   A polynomial of N SIGNED INTEGERS v_k; every limb holds the same integer as its canonical residue v_k mod q_limb in [0, q_limb).
//   Coefficient k takes the ChaCha20 block (RFC 8439 section 2.3, chacha20_block of chacha20.h) with key = the 32-byte seed, block counter k >> 1 and
//   nonce (item, stream_id, 0x6b73616d), and of it the output words 8 (k & 1) .. 8 (k & 1) + 7 read as ONE 256-bit little-endian integer X.
//   The third nonce word keeps these streams apart from expand(seed, item, limb, component) (component < 3) even under a misused common seed.
//     kind 0, ternary:            v = floor(3 (X mod 2^64) / 2^64) - 1           (bias at most 2^-63 per coefficient, no rejection)
//     kind 1, centred binomial:   v = popcount(X & 0x1fffff) - popcount((X >> 21) & 0x1fffff)     (eta = 21: sigma = 3.24, |v| <= 21)
//     kind 2, flood, param = f:   v = (X mod 2^(f + 1)) - 2^f,  1 <= f <= 250   (exactly uniform on [-2^f, 2^f))
//   The key stream does not depend on the limb: one block serves two coefficients on every limb.
//
// Security: the seed is SECRET (the server's).  It travels as a kernel argument and is never written to memory.  One seed must never serve two
// calls: equal masks would make the difference of two results equal the difference of their inputs.
//
// Shared by the device kernel (k_noise.hip) and the host twin (dpfhe_sample_noise_host): one statement of the format.
#pragma once
#include "expand.h"

namespace dpfhe {

constexpr u32 kNoiseDomain = 0x6b73616du;   // third nonce word
constexpr u32 kNoiseTernary = 0, kNoiseCbd21 = 1, kNoiseFlood = 2;
constexpr u32 kNoiseMaxFlood = 250;
constexpr u32 kNoiseLimbs = 16;   // limbs per launch (their constants are a kernel argument); a longer context takes several launches

struct NoiseLimb {
    u64 q, br_hi, br_lo;   // floor(2^128 / q) as in LimbConst
    u64 t128;              // 2^128 mod q  (= two64^2 mod q)
    u64 off;               // flood: 2^f mod q
};

struct NoiseArgs {
    ExpandKey key;
    u32 first_item, stream_id, kind, param;
    u32 comp, comps, ctx_limbs, log2n;
    u32 l0, n_limbs;       // this launch covers limbs [l0, l0 + n_limbs) of the context
    u32 add, pad;
    NoiseLimb limb[kNoiseLimbs];
};

// one coefficient before reduction: a small signed value (ternary, binomial) or the masked 256-bit Y = X mod 2^(f+1) of a flood coefficient
struct NoiseCoeff {
    int small;
    u64 y[4];
};

// x = the 8 words of the coefficient, least significant first
template <u32 KIND>
DPF_HD NoiseCoeff noise_decode(const u32 x[8], u32 f) {
    NoiseCoeff c{};
    const u64 lo = (u64)x[0] | ((u64)x[1] << 32);
    if (KIND == kNoiseTernary) c.small = (int)mulhi64(lo, 3) - 1;
    if (KIND == kNoiseCbd21) c.small = __builtin_popcount((u32)lo & 0x1fffffu) - __builtin_popcount((u32)(lo >> 21) & 0x1fffffu);
    if (KIND == kNoiseFlood) {
        const u32 bits = f + 1;   // 2 .. 251 bits are kept
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (u32 i = 0; i < 4; ++i) {
            const u64 w = (u64)x[2 * i] | ((u64)x[2 * i + 1] << 32);
            c.y[i] = bits >= 64 * (i + 1) ? w : (bits > 64 * i ? w & ((~(u64)0) >> (64 * (i + 1) - bits)) : 0);
        }
    }
    return c;
}

// the canonical residue of a small signed value
DPF_HD u64 noise_small_residue(int v, u64 q) {
    u64 m = (u64)(v < 0 ? -v : v);
    if (m >= q) m %= q;   // only a modulus below 22 gets here (host twin; device limbs exceed 2N)
    return (v < 0 && m) ? q - m : m;
}

// (Y - 2^f) mod q for the 256-bit Y = y[3] 2^192 + ... + y[0]:  Y = H 2^128 + L;  h = H mod q;  h t128 < 2^120;  S = h t128 + L may carry out of
// 128 bits once, and the lost 2^128 is t128 again.  `wide` (f >= 128, the same for every lane) says whether H can be non-zero at all.
DPF_HD u64 noise_flood_residue(const u64 y[4], const NoiseLimb& c, bool wide) {
    u64 r;
    if (wide) {
        const u64 h = reduce128(y[2], y[3], c.q, c.br_hi, c.br_lo);
        const u64 plo = h * c.t128, phi = mulhi64(h, c.t128);
        const u64 slo = plo + y[0];
        const u64 c0 = slo < plo ? 1u : 0u;
        const u64 s1 = phi + y[1];
        const u64 c1 = s1 < phi ? 1u : 0u;
        const u64 shi = s1 + c0;
        const u64 carry = c1 | (shi < s1 ? 1u : 0u);
        r = reduce128(slo, shi, c.q, c.br_hi, c.br_lo);
        if (carry) r = add_mod(r, c.t128, c.q);
    } else {
        r = reduce128(y[0], y[1], c.q, c.br_hi, c.br_lo);
    }
    return sub_mod(r, c.off, c.q);
}

template <u32 KIND>
DPF_HD u64 noise_residue(const NoiseCoeff& v, const NoiseLimb& c, bool wide) {
    return KIND == kNoiseFlood ? noise_flood_residue(v.y, c, wide) : noise_small_residue(v.small, c.q);
}

// the two coefficients 2 j, 2 j + 1 of one item, j = the block counter
template <u32 KIND>
DPF_HD void noise_block(const NoiseArgs& a, u32 j, u32 item, NoiseCoeff& v0, NoiseCoeff& v1) {
    u32 w[16];
    chacha20_block(a.key, j, item, a.stream_id, kNoiseDomain, w);
    v0 = noise_decode<KIND>(w, a.param);
    v1 = noise_decode<KIND>(w + 8, a.param);
}

// the constants of one limb (host side of both the launcher and the twin); q odd, 3 <= q < 2^60
inline NoiseLimb noise_limb(u64 q, u32 kind, u32 f) {
    const unsigned __int128 br = (~(unsigned __int128)0) / q;   // floor(2^128 / q): q is odd, never a power of two
    NoiseLimb c{};
    c.q = q;
    c.br_hi = (u64)(br >> 64);
    c.br_lo = (u64)br;
    const u64 two64 = (u64)((((unsigned __int128)1) << 64) % q);
    c.t128 = (u64)((unsigned __int128)two64 * two64 % q);
    if (kind == kNoiseFlood) {
        u64 p = (u64)((((unsigned __int128)1) << (f & 63)) % q);
        for (u32 i = 0; i < (f >> 6); ++i) p = (u64)((unsigned __int128)p * two64 % q);
        c.off = p;
    }
    return c;
}

// host twin of the device launch (k_noise.hip launch_sample_noise): every other word untouched
void sample_noise_host(u64* out, size_t batch, const NoiseArgs& a);

}  // namespace dpfhe
