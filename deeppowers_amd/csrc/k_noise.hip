// k_noise.hip - noise polynomials for re-randomisation (noise.h): the device kernel, its launcher, the host twin, the accumulate pass of
// dpfhe_rerandomize, and the entries of include/dpfhe.h.
//
// One lane per ChaCha20 block: the block gives two adjacent coefficients, and since the key stream does not depend on the limb the lane decodes them
// once and walks the limbs, writing one 16-byte store per limb row; consecutive lanes write consecutive 16-byte words, so every wave store covers 1 KiB
// of one row without LDS (workmap.h ItemChunkMap: outer = item, N / 2 lanes).  The limb constants and the seed's key words are kernel arguments (scalar
// loads, SGPRs).  Without `add` the kernel loads nothing from memory; with it, one 16-byte load per store.
#include <cstring>

#include "cabi.h"
#include "noise.h"

namespace dpfhe {

// lane j of an item computes ChaCha block j, coefficients 2 j and 2 j + 1
template <u32 KIND, bool ADD>
__global__ __launch_bounds__(256) void sample_noise_kernel(u64* __restrict__ buf, const NoiseArgs a, u32 log2_chunks) {
    const ItemChunkWork w = ItemChunkMap::decode(blockIdx.x, log2_chunks);
    const u32 j = ItemChunkMap::lane(w.chunk, blockDim.x, threadIdx.x);
    NoiseCoeff v0, v1;
    noise_block<KIND>(a, j, a.first_item + w.outer, v0, v1);
    const bool wide = a.param >= 128;
    const size_t poly = (size_t)1 << a.log2n;
    u64* p = buf + (((size_t)w.outer * a.comps + a.comp) * a.ctx_limbs + a.l0) * poly + 2 * (size_t)j;
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
static void launch_kind(u64* buf, const NoiseArgs& a, const ItemChunkPlan& p, hipStream_t s) {
    if (a.add) hipLaunchKernelGGL((sample_noise_kernel<KIND, true>), dim3((unsigned)p.grid), dim3(p.threads), 0, s, buf, a, p.log2_chunks);
    else hipLaunchKernelGGL((sample_noise_kernel<KIND, false>), dim3((unsigned)p.grid), dim3(p.threads), 0, s, buf, a, p.log2_chunks);
}

// device: component a.comp of items [0, batch) of buf [batch][comps][ctx_limbs][N], limbs [a.l0, a.l0 + a.n_limbs): = noise, or += noise mod q with a.add;
// 0, or -1 if the grid is too large
static int launch_sample_noise(u64* buf, size_t batch, const NoiseArgs& a, hipStream_t s) {
    const ItemChunkPlan p = ItemChunkMap::pairs(batch, a.log2n);   // a ChaCha block per pair
    if (!p.ok || a.n_limbs == 0 || a.n_limbs > kNoiseLimbs) return -1;
    switch (a.kind) {
        case kNoiseTernary: launch_kind<kNoiseTernary>(buf, a, p, s); break;
        case kNoiseCbd21: launch_kind<kNoiseCbd21>(buf, a, p, s); break;
        case kNoiseFlood: launch_kind<kNoiseFlood>(buf, a, p, s); break;
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

// device: ct [batch][2][L][N] += prod [2][batch][L][N] mod q, word by word (the last step of dpfhe_rerandomize); 0, or -1 if the grid is too large
static int launch_add_products(u64* ct, const u64* prod, size_t batch, u32 n_limbs, int log2n, const LimbConst* lc, hipStream_t s) {
    const size_t grid = batch * 2 * n_limbs;
    if (grid == 0 || grid > kMaxGrid) return -1;
    hipLaunchKernelGGL(add_products_kernel, dim3((unsigned)grid), dim3(256), 0, s, ct, prod, lc, (u32)batch, n_limbs, (u32)log2n);
    return 0;
}

}  // namespace dpfhe

// ------------------------------------------------------------------------------------------------
// noise polynomials and re-randomisation (noise.h, k_noise.hip): noise(seed, item, stream_id, kind, param) into one component of a batch
static int noise_args(const char* what, const void* out, size_t batch, size_t comps, uint32_t comp, uint32_t kind, uint32_t param, uint32_t stream_id,
                      const uint8_t* seed, uint32_t first_item, uint32_t flags, uint32_t ctx_limbs, uint32_t log2_n, NoiseArgs& a) {
    if (!out || !seed || batch == 0) return fail(DPFHE_INVALID_ARGUMENT, what, "null buffer or seed, or batch 0");
    if (kind > kNoiseFlood) return fail(DPFHE_INVALID_ARGUMENT, what, "kind must be 0 (ternary), 1 (centred binomial) or 2 (flood)");
    if (kind == kNoiseFlood && (param < 1 || param > kNoiseMaxFlood)) return fail(DPFHE_INVALID_ARGUMENT, what, "flood bits must lie in [1, 250]");
    if (comp >= comps || comps > 0xffffffffu) return fail(DPFHE_INVALID_ARGUMENT, what, "component must be < components");
    if (flags & ~(uint32_t)DPFHE_NOISE_ADD) return fail(DPFHE_INVALID_ARGUMENT, what, "unknown flag");
    if (batch > ((uint64_t)1 << 32) - first_item) return fail(DPFHE_INVALID_ARGUMENT, what, "first_item + batch must be <= 2^32");
    a = NoiseArgs{};
    std::memcpy(a.key.w, seed, 32);   // little-endian words (x86-64 and gfx950 hosts)
    a.first_item = first_item; a.stream_id = stream_id; a.kind = kind; a.param = kind == kNoiseFlood ? param : 0;
    a.comp = comp; a.comps = (uint32_t)comps; a.ctx_limbs = ctx_limbs; a.log2n = log2_n;
    a.add = flags & DPFHE_NOISE_ADD ? 1u : 0u;
    return DPFHE_SUCCESS;
}

// the limbs in launches of at most kNoiseLimbs (for_limb_groups): f() runs with a's limbs and their constants set
template <class F>
static int noise_limb_groups(NoiseArgs& a, const uint64_t* moduli, uint32_t n_limbs, F f) {
    return for_limb_groups(n_limbs, kNoiseLimbs, [&](uint32_t l0, uint32_t count) {
        a.l0 = l0;
        a.n_limbs = count;
        for (uint32_t l = 0; l < count; ++l) a.limb[l] = noise_limb(moduli[l0 + l], a.kind, a.param);
    }, f);
}

// arguments validated, device selected by the caller
static int noise_launch(const char* what, dpfhe_ctx* c, uint64_t* d_out, size_t batch, NoiseArgs& a, hipStream_t s) {
    return noise_limb_groups(a, c->moduli.data(), c->n_limbs, [&] {
        if (launch_sample_noise(d_out, batch, a, s)) return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
        return check_launch("sample_noise kernel launch");
    });
}

extern "C" int dpfhe_sample_noise(dpfhe_ctx* c, uint64_t* d_out, size_t batch, size_t comps, uint32_t comp, uint32_t kind, uint32_t param, uint32_t stream_id,
                                  const uint8_t seed[32], uint32_t first_item, uint32_t flags, void* stream) {
    static const char* what = "dpfhe_sample_noise";
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    NoiseArgs a;
    if (int rc = noise_args(what, d_out, batch, comps, comp, kind, param, stream_id, seed, first_item, flags, c->n_limbs, c->log2n, a)) return rc;
    if (misaligned(d_out)) return fail(DPFHE_INVALID_ARGUMENT, what, "misaligned buffer");
    if (!ItemChunkMap::pairs(batch, c->log2n).ok) return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    DPFHE_ON_DEVICE(c, what);
    return noise_launch(what, c, d_out, batch, a, static_cast<hipStream_t>(stream));
}

extern "C" int dpfhe_sample_noise_host(const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n, uint64_t* out, size_t batch, size_t comps, uint32_t comp,
                                       uint32_t kind, uint32_t param, uint32_t stream_id, const uint8_t seed[32], uint32_t first_item, uint32_t flags) {
    static const char* what = "dpfhe_sample_noise_host";
    if (!moduli) return fail(DPFHE_INVALID_ARGUMENT, what, "null moduli");
    if (int rc = check_host_ring(what, moduli, n_limbs, log2_n)) return rc;
    NoiseArgs a;
    if (int rc = noise_args(what, out, batch, comps, comp, kind, param, stream_id, seed, first_item, flags, n_limbs, log2_n, a)) return rc;
    return noise_limb_groups(a, moduli, n_limbs, [&] {
        sample_noise_host(out, batch, a);
        return (int)DPFHE_SUCCESS;
    });
}

// floor(log2 of the product of the moduli), exactly (the product in 64-bit words)
static uint32_t floor_log2_product(const std::vector<uint64_t>& moduli) {
    std::vector<uint64_t> w(1, 1);
    for (uint64_t q : moduli) {
        uint64_t carry = 0;
        for (uint64_t& x : w) {
            const unsigned __int128 t = (unsigned __int128)x * q + carry;
            x = (uint64_t)t;
            carry = (uint64_t)(t >> 64);
        }
        if (carry) w.push_back(carry);
    }
    return (uint32_t)(64 * (w.size() - 1) + (63 - __builtin_clzll(w.back())));
}

// u = ternary, e0 = flood, e1 = centred binomial:  (c0, c1) += (INTT(pk0 (.) NTT(u)) + e0, INTT(pk1 (.) NTT(u)) + e1).
// d_work: u [batch][L][N] | products [2][batch][L][N]
extern "C" int dpfhe_rerandomize(dpfhe_ctx* c, uint64_t* d_ct2, const uint64_t* d_pk, size_t batch, uint32_t flood_bits, const uint8_t seed[32],
                                 uint32_t first_item, uint64_t* d_work, void* stream) {
    static const char* what = "dpfhe_rerandomize";
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    if (!d_ct2 || !d_pk || !d_work || !seed || batch == 0) return fail(DPFHE_INVALID_ARGUMENT, what, "null buffer or seed, or batch 0");
    if (misaligned(d_ct2) || misaligned(d_pk) || misaligned(d_work)) return fail(DPFHE_INVALID_ARGUMENT, what, "misaligned buffer");
    const uint32_t log2_q = floor_log2_product(c->moduli);
    if (flood_bits < 1 || flood_bits > kNoiseMaxFlood || flood_bits + 3 > log2_q)
        return fail(DPFHE_INVALID_ARGUMENT, what, "flood_bits must lie in [1, min(250, floor(log2 Q) - 3)]");
    if (batch > ((uint64_t)1 << 32) - first_item) return fail(DPFHE_INVALID_ARGUMENT, what, "first_item + batch must be <= 2^32");
    const size_t poly = (size_t)c->n_limbs << c->log2n, npolys = batch * c->n_limbs;
    if (!ntt_grid_fits(c, 2 * npolys) || !ItemChunkMap::pairs(batch, c->log2n).ok)
        return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    if (overlaps(d_work, 3 * batch * poly, d_ct2, 2 * batch * poly) || overlaps(d_work, 3 * batch * poly, d_pk, 2 * poly) ||
        overlaps(d_ct2, 2 * batch * poly, d_pk, 2 * poly))
        return fail(DPFHE_INVALID_ARGUMENT, what, "the work buffer, the ciphertexts and the public key must not overlap");
    DPFHE_ON_DEVICE(c, what);
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint64_t* u = d_work;
    uint64_t* prod = d_work + batch * poly;
    NoiseArgs a;
    if (int rc = noise_args(what, u, batch, 1, 0, kNoiseTernary, 0, 0, seed, first_item, 0, c->n_limbs, c->log2n, a)) return rc;
    if (int rc = noise_launch(what, c, u, batch, a, s)) return rc;
    if (int rc = ntt_launch(c, false, u, u, npolys, s)) return rc;
    (void)launch_dyadic(c, DY_MUL, prod, u, d_pk, npolys, s, (int)c->n_limbs);
    (void)launch_dyadic(c, DY_MUL, prod + batch * poly, u, d_pk + poly, npolys, s, (int)c->n_limbs);
    if (int rc = check_launch("dyadic kernel launch")) return rc;
    if (int rc = ntt_launch(c, true, prod, prod, 2 * npolys, s)) return rc;
    if (launch_add_products(d_ct2, prod, batch, c->n_limbs, (int)c->log2n, c->lc, s)) return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    if (int rc = check_launch("add_products kernel launch")) return rc;
    if (int rc = noise_args(what, d_ct2, batch, 2, 0, kNoiseFlood, flood_bits, 2, seed, first_item, DPFHE_NOISE_ADD, c->n_limbs, c->log2n, a)) return rc;
    if (int rc = noise_launch(what, c, d_ct2, batch, a, s)) return rc;
    if (int rc = noise_args(what, d_ct2, batch, 2, 1, kNoiseCbd21, 0, 1, seed, first_item, DPFHE_NOISE_ADD, c->n_limbs, c->log2n, a)) return rc;
    return noise_launch(what, c, d_ct2, batch, a, s);
}
