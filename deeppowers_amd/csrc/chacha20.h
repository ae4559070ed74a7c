// chacha20.h - the ChaCha20 block function of RFC 8439 section 2.3: the ONE statement of it in the product.
//
// It serves the device kernels (k_expand.hip, k_noise.hip), their host twins (expand.h, noise.h) and the facade's generator of secret keys, errors
// and seeds (fhe_sampler.h).  tests/test_seeded_cpu.py holds it to the RFC's test vector and to openssl; tests/test_facade_sampler_cpu.py holds the
// facade's generator to it.  No HIP runtime: plain g++ includes it too.
#pragma once
#include "modarith.h"

namespace dpfhe {

struct ExpandKey {   // the seed as 8 little-endian words: a kernel argument, so the key words live in SGPRs
    u32 w[8];
};

#if defined(__HIPCC__)
DPF_HD u32 rotl32(u32 v, int c) { return __builtin_rotateleft32(v, (u32)c); }   // one v_alignbit_b32 (v_perm_b32 for 8 / 16)
#else
DPF_HD u32 rotl32(u32 v, int c) { return (v << c) | (v >> (32 - c)); }          // (g++ 11 has no rotate builtin; 0 < c < 32 here)
#endif

#define DPFHE_CHACHA_QR(a, b, c, d)            \
    a += b; d = rotl32(d ^ a, 16);             \
    c += d; b = rotl32(b ^ c, 12);             \
    a += b; d = rotl32(d ^ a, 8);              \
    c += d; b = rotl32(b ^ c, 7)

// RFC 8439 section 2.3: the 16 output words of the block (counter, nonce n0 n1 n2) under key k
DPF_HD void chacha20_block(const ExpandKey& k, u32 counter, u32 n0, u32 n1, u32 n2, u32 out[16]) {
    u32 x0 = 0x61707865u, x1 = 0x3320646eu, x2 = 0x79622d32u, x3 = 0x6b206574u;   // "expand 32-byte k"
    u32 x4 = k.w[0], x5 = k.w[1], x6 = k.w[2], x7 = k.w[3], x8 = k.w[4], x9 = k.w[5], x10 = k.w[6], x11 = k.w[7];
    u32 x12 = counter, x13 = n0, x14 = n1, x15 = n2;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 10; ++i) {
        DPFHE_CHACHA_QR(x0, x4, x8, x12); DPFHE_CHACHA_QR(x1, x5, x9, x13); DPFHE_CHACHA_QR(x2, x6, x10, x14); DPFHE_CHACHA_QR(x3, x7, x11, x15);
        DPFHE_CHACHA_QR(x0, x5, x10, x15); DPFHE_CHACHA_QR(x1, x6, x11, x12); DPFHE_CHACHA_QR(x2, x7, x8, x13); DPFHE_CHACHA_QR(x3, x4, x9, x14);
    }
    out[0] = x0 + 0x61707865u; out[1] = x1 + 0x3320646eu; out[2] = x2 + 0x79622d32u; out[3] = x3 + 0x6b206574u;
    out[4] = x4 + k.w[0]; out[5] = x5 + k.w[1]; out[6] = x6 + k.w[2]; out[7] = x7 + k.w[3];
    out[8] = x8 + k.w[4]; out[9] = x9 + k.w[5]; out[10] = x10 + k.w[6]; out[11] = x11 + k.w[7];
    out[12] = x12 + counter; out[13] = x13 + n0; out[14] = x14 + n1; out[15] = x15 + n2;
}
#undef DPFHE_CHACHA_QR

}  // namespace dpfhe
