// k_plain_add.hip - exact plaintext addition (plain_add.h): the device kernel, its launcher and the host twin.
//
// One lane per pair of coefficients: it reads its two plaintext words (16 bytes; a broadcast plaintext is read from cache), reduces them mod t once
// and walks the limbs of component 0 with one 16-byte load and store per limb - each limb row is contiguous across the wave.  Out of place, the same
// lane copies its pair of every other component.  A one-pass stream: 16 bytes of HBM traffic per c0 word in place.
// Below it, the plaintext addition on residues (dpfhe_add_plain: the approximate family's bias add) in the same shape.
#include "plain_add.h"

namespace dpfhe {

typedef u64 u64x2_t __attribute__((ext_vector_type(2)));

// block b = (item << log2_chunks) + chunk;  lane t of the chunk owns coefficients 2 j, 2 j + 1, j = chunk * blockDim.x + t
// (out and in may be the same buffer: no __restrict__ on them)
__global__ __launch_bounds__(256) void add_plain_scaled_kernel(u64* out, const u64* in, const u64* __restrict__ plain, const PlainAddArgs a,
                                                               u32 comps, u32 ctx_limbs, u32 log2n, u32 log2_chunks, u32 group) {
    const u32 blk = blockIdx.x;
    const u32 chunk = blk & ((1u << log2_chunks) - 1u);
    const u32 item = blk >> log2_chunks;
    const size_t k = 2 * ((size_t)chunk * blockDim.x + threadIdx.x);
    const u64x2_t b = *reinterpret_cast<const u64x2_t*>(plain + ((size_t)(item / group) << log2n) + k);
    const u64 y0 = plain_add_residue(b.x, a), y1 = plain_add_residue(b.y, a);
    const bool hi0 = y0 > a.half, hi1 = y1 > a.half;
    const size_t poly = (size_t)1 << log2n;
    const size_t base = ((size_t)item * comps * ctx_limbs + a.l0) * poly + k;
    for (u32 l = 0; l < a.n_limbs; ++l) {
        const PlainAddLimb c = a.limb[l];
        const u64x2_t x = *reinterpret_cast<const u64x2_t*>(in + base + l * poly);
        *reinterpret_cast<u64x2_t*>(out + base + l * poly) = u64x2_t{plain_add_limb(x.x, y0, c, hi0), plain_add_limb(x.y, y1, c, hi1)};
    }
    if (out != in)
        for (u32 j = 1; j < comps; ++j)
            for (u32 l = 0; l < a.n_limbs; ++l) {
                const size_t off = base + ((size_t)j * ctx_limbs + l) * poly;
                *reinterpret_cast<u64x2_t*>(out + off) = *reinterpret_cast<const u64x2_t*>(in + off);
            }
}

int launch_add_plain_scaled(int log2n, u64* out, const u64* in, const u64* plain, size_t batch, u32 comps, u32 ctx_limbs, size_t group, const PlainAddArgs& a,
                            hipStream_t s) {
    const u32 pairs = 1u << (log2n - 1);                       // lanes per residue polynomial (log2n >= 8: at least two waves)
    const u32 threads = pairs < 256u ? pairs : 256u;
    u32 log2_chunks = 0;
    while ((threads << log2_chunks) < pairs) ++log2_chunks;
    const size_t grid = batch << log2_chunks;
    if (grid == 0 || grid > 0x7fffffffu || group == 0 || group > 0xffffffffu) return -1;
    hipLaunchKernelGGL(add_plain_scaled_kernel, dim3((unsigned)grid), dim3(threads), 0, s, out, in, plain, a, comps, ctx_limbs, (u32)log2n, log2_chunks,
                       (u32)group);
    return 0;
}

void add_plain_scaled_host(int log2n, u64* out, const u64* in, const u64* plain, size_t batch, u32 comps, u32 ctx_limbs, size_t group, const PlainAddArgs& a) {
    const size_t n = (size_t)1 << log2n;
    for (size_t i = 0; i < batch; ++i) {
        const u64* b = plain + (i / group) * n;
        for (u32 l = 0; l < a.n_limbs; ++l) {
            const size_t row = (i * comps * ctx_limbs + a.l0 + l) * n;
            for (size_t k = 0; k < n; ++k) {
                const u64 y = plain_add_residue(b[k], a);
                out[row + k] = plain_add_limb(in[row + k], y, a.limb[l], y > a.half);
            }
            if (out != in)
                for (u32 j = 1; j < comps; ++j)
                    for (size_t k = 0; k < n; ++k) out[row + j * ctx_limbs * n + k] = in[row + j * ctx_limbs * n + k];
        }
    }
}

// ---- plaintext addition on residues: c0 +- p mod q_l, the plaintext [plain_items][L][N] canonical words of the ciphertext's own domain -------------
// The same blocks and lanes as above; q comes from the context's LimbConst (a scalar load: the limb is uniform over the launch's inner loop), the
// plaintext row of a limb is read with one 16-byte load per lane like the c0 row.  In place: 24 bytes of traffic per c0 word, 16 of them HBM when
// the plaintext is broadcast (it then stays in cache).
__global__ __launch_bounds__(256) void add_plain_kernel(u64* out, const u64* in, const u64* __restrict__ plain, const LimbConst* __restrict__ lc, u32 comps,
                                                        u32 n_limbs, u32 log2n, u32 log2_chunks, u32 group, u32 negate) {
    const u32 blk = blockIdx.x;
    const u32 chunk = blk & ((1u << log2_chunks) - 1u);
    const u32 item = blk >> log2_chunks;
    const size_t k = 2 * ((size_t)chunk * blockDim.x + threadIdx.x);
    const size_t poly = (size_t)1 << log2n;
    const size_t base = (size_t)item * comps * n_limbs * poly + k;
    const size_t pbase = (size_t)(item / group) * n_limbs * poly + k;
    for (u32 l = 0; l < n_limbs; ++l) {
        const u64 q = lc[l].q;
        const u64x2_t x = *reinterpret_cast<const u64x2_t*>(in + base + l * poly);
        const u64x2_t p = *reinterpret_cast<const u64x2_t*>(plain + pbase + l * poly);
        *reinterpret_cast<u64x2_t*>(out + base + l * poly) = u64x2_t{add_plain_word(x.x, p.x, q, negate), add_plain_word(x.y, p.y, q, negate)};
    }
    if (out != in)
        for (u32 j = 1; j < comps; ++j)
            for (u32 l = 0; l < n_limbs; ++l) {
                const size_t off = base + ((size_t)j * n_limbs + l) * poly;
                *reinterpret_cast<u64x2_t*>(out + off) = *reinterpret_cast<const u64x2_t*>(in + off);
            }
}

int launch_add_plain(int log2n, u64* out, const u64* in, const u64* plain, size_t batch, u32 comps, u32 n_limbs, size_t group, bool negate,
                     const LimbConst* lc, hipStream_t s) {
    const u32 pairs = 1u << (log2n - 1);                       // lanes per residue polynomial (log2n >= 8: at least two waves)
    const u32 threads = pairs < 256u ? pairs : 256u;
    u32 log2_chunks = 0;
    while ((threads << log2_chunks) < pairs) ++log2_chunks;
    const size_t grid = batch << log2_chunks;
    if (grid == 0 || grid > 0x7fffffffu || group == 0 || group > 0xffffffffu) return -1;
    hipLaunchKernelGGL(add_plain_kernel, dim3((unsigned)grid), dim3(threads), 0, s, out, in, plain, lc, comps, n_limbs, (u32)log2n, log2_chunks, (u32)group,
                       negate ? 1u : 0u);
    return 0;
}

void add_plain_host(int log2n, const u64* moduli, u32 n_limbs, u64* out, const u64* in, const u64* plain, size_t batch, u32 comps, size_t group, bool negate) {
    const size_t n = (size_t)1 << log2n;
    for (size_t i = 0; i < batch; ++i)
        for (u32 l = 0; l < n_limbs; ++l) {
            const u64* p = plain + ((i / group) * n_limbs + l) * n;
            const size_t row = (i * comps * n_limbs + l) * n;
            for (size_t k = 0; k < n; ++k) out[row + k] = add_plain_word(in[row + k], p[k], moduli[l], negate);
            if (out != in)
                for (u32 j = 1; j < comps; ++j)
                    for (size_t k = 0; k < n; ++k) out[row + j * n_limbs * n + k] = in[row + j * n_limbs * n + k];
        }
}

}  // namespace dpfhe
