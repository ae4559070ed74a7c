// k_noise.hip - noise polynomials for re-randomisation (noise.h): the device kernel, its launcher, the host twin, and the accumulate pass of
// dpfhe_rerandomize.
//
// One lane per ChaCha20 block: the block gives two adjacent coefficients, and since the key stream does not depend on the limb the lane decodes them
// once and walks the limbs, writing one 16-byte store per limb row; consecutive lanes write consecutive 16-byte words, so every wave store covers 1 KiB
// of one row without LDS.  The limb constants and the seed's key words are kernel arguments (scalar loads, SGPRs).  Without `add` the kernel loads
// nothing from memory; with it, one 16-byte load per store.
#include "noise.h"

namespace dpfhe {

typedef u64 u64x2_t __attribute__((ext_vector_type(2)));

// block b = (item << log2_chunks) + chunk;  lane t of the chunk computes ChaCha block j = chunk * blockDim.x + t, coefficients 2 j and 2 j + 1
template <u32 KIND, bool ADD>
__global__ __launch_bounds__(256) void sample_noise_kernel(u64* __restrict__ buf, const NoiseArgs a, u32 log2_chunks) {
    const u32 blk = blockIdx.x;
    const u32 chunk = blk & ((1u << log2_chunks) - 1u);
    const u32 b = blk >> log2_chunks;
    const u32 j = chunk * blockDim.x + threadIdx.x;
    NoiseCoeff v0, v1;
    noise_block<KIND>(a, j, a.first_item + b, v0, v1);
    const bool wide = a.param >= 128;
    const size_t poly = (size_t)1 << a.log2n;
    u64* p = buf + (((size_t)b * a.comps + a.comp) * a.ctx_limbs + a.l0) * poly + 2 * (size_t)j;
    for (u32 l = 0; l < a.n_limbs; ++l, p += poly) {
        const NoiseLimb c = a.limb[l];
        u64 r0 = noise_residue<KIND>(v0, c, wide), r1 = noise_residue<KIND>(v1, c, wide);
        if (ADD) {
            const u64x2_t x = *reinterpret_cast<const u64x2_t*>(p);
            r0 = add_mod(x.x, r0, c.q);
            r1 = add_mod(x.y, r1, c.q);
        }
        *reinterpret_cast<u64x2_t*>(p) = u64x2_t{r0, r1};
    }
}

template <u32 KIND>
static void launch_kind(u64* buf, const NoiseArgs& a, unsigned grid, unsigned threads, u32 log2_chunks, hipStream_t s) {
    if (a.add) hipLaunchKernelGGL((sample_noise_kernel<KIND, true>), dim3(grid), dim3(threads), 0, s, buf, a, log2_chunks);
    else hipLaunchKernelGGL((sample_noise_kernel<KIND, false>), dim3(grid), dim3(threads), 0, s, buf, a, log2_chunks);
}

int launch_sample_noise(u64* buf, size_t batch, const NoiseArgs& a, hipStream_t s) {
    const u32 pairs = 1u << (a.log2n - 1);                     // ChaCha blocks of one polynomial (log2n >= 8: at least two waves)
    const u32 threads = pairs < 256u ? pairs : 256u;
    u32 log2_chunks = 0;
    while ((threads << log2_chunks) < pairs) ++log2_chunks;
    const size_t grid = batch << log2_chunks;
    if (grid == 0 || grid > 0x7fffffffu || batch > 0xffffffffu || a.n_limbs == 0 || a.n_limbs > kNoiseLimbs) return -1;
    switch (a.kind) {
        case kNoiseTernary: launch_kind<kNoiseTernary>(buf, a, (unsigned)grid, threads, log2_chunks, s); break;
        case kNoiseCbd21: launch_kind<kNoiseCbd21>(buf, a, (unsigned)grid, threads, log2_chunks, s); break;
        case kNoiseFlood: launch_kind<kNoiseFlood>(buf, a, (unsigned)grid, threads, log2_chunks, s); break;
        default: return -1;
    }
    return 0;
}

template <u32 KIND>
static void host_kind(u64* out, size_t batch, const NoiseArgs& a) {
    const size_t n = (size_t)1 << a.log2n;
    const bool wide = a.param >= 128;
    for (size_t b = 0; b < batch; ++b) {
        u64* row0 = out + ((b * a.comps + a.comp) * a.ctx_limbs + a.l0) * n;
        for (u32 j = 0; j < (u32)(n / 2); ++j) {
            NoiseCoeff v[2];
            noise_block<KIND>(a, j, a.first_item + (u32)b, v[0], v[1]);
            for (u32 l = 0; l < a.n_limbs; ++l)
                for (int h = 0; h < 2; ++h) {
                    u64& w = row0[l * n + 2 * (size_t)j + h];
                    const u64 r = noise_residue<KIND>(v[h], a.limb[l], wide);
                    w = a.add ? add_mod(w, r, a.limb[l].q) : r;
                }
        }
    }
}

void sample_noise_host(u64* out, size_t batch, const NoiseArgs& a) {
    if (a.kind == kNoiseTernary) host_kind<kNoiseTernary>(out, batch, a);
    else if (a.kind == kNoiseCbd21) host_kind<kNoiseCbd21>(out, batch, a);
    else host_kind<kNoiseFlood>(out, batch, a);
}

// one workgroup per residue polynomial of the ciphertexts: p = (item * 2 + comp) * L + limb reads product polynomial (comp * batch + item) * L + limb
__global__ __launch_bounds__(256) void add_products_kernel(u64* __restrict__ ct, const u64* __restrict__ prod, const LimbConst* __restrict__ lc, u32 batch,
                                                           u32 n_limbs, u32 log2n) {
    const u32 p = blockIdx.x;
    const u32 limb = p % n_limbs, ic = p / n_limbs, comp = ic & 1u, item = ic >> 1;
    const u64 q = lc[limb].q;
    u64x2_t* pc = reinterpret_cast<u64x2_t*>(ct + ((size_t)p << log2n));
    const u64x2_t* pp = reinterpret_cast<const u64x2_t*>(prod + ((((size_t)comp * batch + item) * n_limbs + limb) << log2n));
    const u32 nv = 1u << (log2n - 1);
    for (u32 i = threadIdx.x; i < nv; i += 256) {
        const u64x2_t x = pc[i], y = pp[i];
        pc[i] = u64x2_t{add_mod(x.x, y.x, q), add_mod(x.y, y.y, q)};
    }
}

int launch_add_products(u64* ct, const u64* prod, size_t batch, u32 n_limbs, int log2n, const LimbConst* lc, hipStream_t s) {
    const size_t grid = batch * 2 * n_limbs;
    if (grid == 0 || grid > 0x7fffffffu) return -1;
    hipLaunchKernelGGL(add_products_kernel, dim3((unsigned)grid), dim3(256), 0, s, ct, prod, lc, (u32)batch, n_limbs, (u32)log2n);
    return 0;
}

}  // namespace dpfhe
