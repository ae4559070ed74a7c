// k_plain_add.hip - exact plaintext addition (plain_add.h): the device kernels, their launchers, the host twins and the entries of include/dpfhe.h.
//
// One lane per pair of coefficients: it reads its two plaintext words (16 bytes; a broadcast plaintext is read from cache), reduces them mod t once
// and walks the limbs of component 0 with one 16-byte load and store per limb - each limb row is contiguous across the wave.  Out of place, the same
// lane copies its pair of every other component.  A one-pass stream: 16 bytes of HBM traffic per c0 word in place.  Blocks and lanes: workmap.h
// ItemChunkMap::pairs.  Below it, the plaintext addition on residues (dpfhe_add_plain: the approximate family's bias add) in the same shape.
#include <algorithm>
#include <vector>

#include "cabi.h"
#include "plain_add.h"

namespace dpfhe {

// out of place, the lane copies its pair (at `base` in row 0 of component 0) of rows [0, n_limbs) of every other component; components are ctx_limbs rows apart
__device__ __forceinline__ void copy_other_components(u64* out, const u64* in, size_t base, size_t poly, u32 comps, u32 ctx_limbs, u32 n_limbs) {
    if (out != in)
        for (u32 j = 1; j < comps; ++j)
            for (u32 l = 0; l < n_limbs; ++l) {
                const size_t off = base + ((size_t)j * ctx_limbs + l) * poly;
                *reinterpret_cast<u64x2_t*>(out + off) = *reinterpret_cast<const u64x2_t*>(in + off);
            }
}
// the same for the host twins: row `row` of component 0, n words
static void copy_other_components_host(u64* out, const u64* in, size_t row, size_t n, u32 comps, u32 ctx_limbs) {
    if (out != in)
        for (u32 j = 1; j < comps; ++j)
            for (size_t k = 0; k < n; ++k) out[row + j * ctx_limbs * n + k] = in[row + j * ctx_limbs * n + k];
}

// lane j of an item owns coefficients 2 j, 2 j + 1  (out and in may be the same buffer: no __restrict__ on them)
__global__ __launch_bounds__(256) void add_plain_scaled_kernel(u64* out, const u64* in, const u64* __restrict__ plain, const PlainAddArgs a,
                                                               u32 comps, u32 ctx_limbs, u32 log2n, u32 log2_chunks, u32 group) {
    const ItemChunkWork w = ItemChunkMap::decode(blockIdx.x, log2_chunks);
    const size_t k = 2 * ItemChunkMap::lane<size_t>(w.chunk, blockDim.x, threadIdx.x);
    const u64x2_t b = *reinterpret_cast<const u64x2_t*>(plain + ((size_t)(w.outer / group) << log2n) + k);
    const u64 y0 = plain_add_residue(b.x, a), y1 = plain_add_residue(b.y, a);
    const bool hi0 = y0 > a.half, hi1 = y1 > a.half;
    const size_t poly = (size_t)1 << log2n;
    const size_t base = ((size_t)w.outer * comps * ctx_limbs + a.l0) * poly + k;
    for (u32 l = 0; l < a.n_limbs; ++l) {
        const PlainAddLimb c = a.limb[l];
        const u64x2_t x = *reinterpret_cast<const u64x2_t*>(in + base + l * poly);
        *reinterpret_cast<u64x2_t*>(out + base + l * poly) = u64x2_t{plain_add_limb(x.x, y0, c, hi0), plain_add_limb(x.y, y1, c, hi1)};
    }
    copy_other_components(out, in, base, poly, comps, ctx_limbs, a.n_limbs);
}

// device: out[i][0][l0 .. l0 + n_limbs) = in[i][0] + round(Q plain[i / group] / t), out[i][k >= 1] = in[i][k] of those limbs when out != in.
// 0, or -1 if the grid is too large for one launch.
static int launch_add_plain_scaled(int log2n, u64* out, const u64* in, const u64* plain, size_t batch, u32 comps, u32 ctx_limbs, size_t group, const PlainAddArgs& a,
                            hipStream_t s) {
    const ItemChunkPlan p = ItemChunkMap::pairs(batch, (unsigned)log2n);
    if (!p.ok || group == 0 || group > 0xffffffffu) return -1;
    hipLaunchKernelGGL(add_plain_scaled_kernel, dim3((unsigned)p.grid), dim3(p.threads), 0, s, out, in, plain, a, comps, ctx_limbs, (u32)log2n, p.log2_chunks,
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
            copy_other_components_host(out, in, row, n, comps, ctx_limbs);
        }
    }
}

// ---- plaintext addition on residues: c0 +- p mod q_l, the plaintext [plain_items][L][N] canonical words of the ciphertext's own domain -------------
// The same map as above; q comes from the context's LimbConst (a scalar load: the limb is uniform over the launch's inner loop), the
// plaintext row of a limb is read with one 16-byte load per lane like the c0 row.  In place: 24 bytes of traffic per c0 word, 16 of them HBM when
// the plaintext is broadcast (it then stays in cache).
__global__ __launch_bounds__(256) void add_plain_kernel(u64* out, const u64* in, const u64* __restrict__ plain, const LimbConst* __restrict__ lc, u32 comps,
                                                        u32 n_limbs, u32 log2n, u32 log2_chunks, u32 group, u32 negate) {
    const ItemChunkWork w = ItemChunkMap::decode(blockIdx.x, log2_chunks);
    const size_t k = 2 * ItemChunkMap::lane<size_t>(w.chunk, blockDim.x, threadIdx.x);
    const size_t poly = (size_t)1 << log2n;
    const size_t base = (size_t)w.outer * comps * n_limbs * poly + k;
    const size_t pbase = (size_t)(w.outer / group) * n_limbs * poly + k;
    for (u32 l = 0; l < n_limbs; ++l) {
        const u64 q = lc[l].q;
        const u64x2_t x = *reinterpret_cast<const u64x2_t*>(in + base + l * poly);
        const u64x2_t p = *reinterpret_cast<const u64x2_t*>(plain + pbase + l * poly);
        *reinterpret_cast<u64x2_t*>(out + base + l * poly) = u64x2_t{add_plain_word(x.x, p.x, q, negate), add_plain_word(x.y, p.y, q, negate)};
    }
    copy_other_components(out, in, base, poly, comps, n_limbs, n_limbs);
}

// device: out[i][0] = in[i][0] +- plain[i / group] on every limb, out[i][k >= 1] = in[i][k] when out != in; q_l from lc[l].q.
// 0, or -1 if the grid is too large for one launch.
static int launch_add_plain(int log2n, u64* out, const u64* in, const u64* plain, size_t batch, u32 comps, u32 n_limbs, size_t group, bool negate,
                     const LimbConst* lc, hipStream_t s) {
    const ItemChunkPlan p = ItemChunkMap::pairs(batch, (unsigned)log2n);
    if (!p.ok || group == 0 || group > 0xffffffffu) return -1;
    hipLaunchKernelGGL(add_plain_kernel, dim3((unsigned)p.grid), dim3(p.threads), 0, s, out, in, plain, lc, comps, n_limbs, (u32)log2n, p.log2_chunks, (u32)group,
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
            copy_other_components_host(out, in, row, n, comps, n_limbs);
        }
}

}  // namespace dpfhe

// ------------------------------------------------------------------------------------------------
// exact plaintext addition (plain_add.h, k_plain_add.hip): c0 += round(Q b / t) (or -=), one item of `plain` per batch / plain_items ciphertexts
// validates the shape and t, then fills the launch-independent constants and every limb's (q, t^-1, floor(t^-1 2^64 / q))
static int plain_add_args(const char* what, const uint64_t* out, const uint64_t* in, const uint64_t* plain, size_t batch, size_t comps, size_t plain_items,
                          uint64_t t, int negate, const uint64_t* moduli, uint32_t n_limbs, PlainAddArgs& a, std::vector<PlainAddLimb>& limbs) {
    if (!out || !in || !plain) return fail(DPFHE_INVALID_ARGUMENT, what, "null buffer");
    if (comps != 2 && comps != 3) return fail(DPFHE_INVALID_ARGUMENT, what, "ciphertexts have 2 or 3 components");
    if (plain_items == 0 || batch % plain_items) return fail(DPFHE_INVALID_ARGUMENT, what, "batch must be a multiple of plain_items");
    if (t < 3 || (t >> 32) || !(t & 1)) return fail(DPFHE_INVALID_ARGUMENT, what, "plain modulus t must be odd, >= 3 and < 2^32");
    uint64_t q_mod_t = 1 % t;
    limbs.resize(n_limbs);
    for (uint32_t l = 0; l < n_limbs; ++l) {
        const uint64_t q = moduli[l];
        uint64_t inv = 0;
        if (!inverse_mod(t, q, inv)) return fail(DPFHE_INVALID_ARGUMENT, what, "t must be coprime to every modulus");
        limbs[l] = PlainAddLimb{q, inv, (uint64_t)(((unsigned __int128)inv << 64) / q)};
        q_mod_t = (uint64_t)((unsigned __int128)q_mod_t * (q % t) % t);
    }
    a = PlainAddArgs{};
    a.t = t;
    a.t_mu = ~(uint64_t)0 / t;   // = floor(2^64 / t): t is odd, never a power of two
    a.m = negate ? q_mod_t : (t - q_mod_t) % t;
    a.half = (t - 1) / 2;
    return DPFHE_SUCCESS;
}

// the limbs in launches of at most kPlainAddLimbs (for_limb_groups): f() runs with a's limbs and their constants set
template <class F>
static int plain_add_limb_groups(PlainAddArgs& a, const std::vector<PlainAddLimb>& limbs, F f) {
    return for_limb_groups((uint32_t)limbs.size(), kPlainAddLimbs, [&](uint32_t l0, uint32_t count) {
        a.l0 = l0;
        a.n_limbs = count;
        std::copy(limbs.begin() + l0, limbs.begin() + l0 + count, a.limb);
    }, f);
}

extern "C" int dpfhe_add_plain_scaled(dpfhe_ctx* c, uint64_t* d_out, const uint64_t* d_in, const uint64_t* d_plain, size_t batch, size_t comps,
                                      size_t plain_items, uint64_t t, int negate, void* stream) {
    static const char* what = "dpfhe_add_plain_scaled";
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    PlainAddArgs a;
    std::vector<PlainAddLimb> limbs;
    if (int rc = plain_add_args(what, d_out, d_in, d_plain, batch, comps, plain_items, t, negate, c->moduli.data(), c->n_limbs, a, limbs)) return rc;
    if (misaligned(d_out) || misaligned(d_in) || misaligned(d_plain)) return fail(DPFHE_INVALID_ARGUMENT, what, "misaligned buffer");
    const size_t words = batch * comps * ((size_t)c->n_limbs << c->log2n);
    if (d_out != d_in && overlaps(d_out, words, d_in, words)) return fail(DPFHE_INVALID_ARGUMENT, what, "out and in overlap without being the same buffer");
    if (batch == 0) return DPFHE_SUCCESS;
    DPFHE_ON_DEVICE(c, what);
    const size_t group = batch / plain_items;
    return plain_add_limb_groups(a, limbs, [&] {
        if (launch_add_plain_scaled((int)c->log2n, d_out, d_in, d_plain, batch, (u32)comps, c->n_limbs, group, a, static_cast<hipStream_t>(stream)))
            return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
        return check_launch("add_plain_scaled kernel launch");
    });
}

extern "C" int dpfhe_add_plain_scaled_host(const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n, uint64_t* out, const uint64_t* in, const uint64_t* plain,
                                           size_t batch, size_t comps, size_t plain_items, uint64_t t, int negate) {
    static const char* what = "dpfhe_add_plain_scaled_host";
    if (!moduli) return fail(DPFHE_INVALID_ARGUMENT, what, "null moduli");
    if (int rc = check_host_ring(what, moduli, n_limbs, log2_n)) return rc;
    PlainAddArgs a;
    std::vector<PlainAddLimb> limbs;
    if (int rc = plain_add_args(what, out, in, plain, batch, comps, plain_items, t, negate, moduli, n_limbs, a, limbs)) return rc;
    const size_t n = (size_t)1 << log2_n, words = batch * comps * n_limbs * n;
    if (out != in && overlaps(out, words, in, words)) return fail(DPFHE_INVALID_ARGUMENT, what, "out and in overlap without being the same buffer");
    for (size_t i = 0; i < plain_items * n; ++i)
        if (plain[i] >> 32) return fail(DPFHE_INVALID_ARGUMENT, what, "plaintext words must be < 2^32");
    if (batch == 0) return DPFHE_SUCCESS;
    const size_t group = batch / plain_items;
    return plain_add_limb_groups(a, limbs, [&] {
        add_plain_scaled_host((int)log2_n, out, in, plain, batch, (u32)comps, n_limbs, group, a);
        return (int)DPFHE_SUCCESS;
    });
}

// plaintext addition on residues (plain_add.h, k_plain_add.hip): c0 +- p mod q_l, p [plain_items][L][N] canonical words of the ciphertext's domain
// the shape checks the device entry and the host twin share; `limbs` and `log2n` are the ring's
static int add_plain_args(const char* what, const uint64_t* out, const uint64_t* in, const uint64_t* plain, size_t batch, size_t comps, size_t plain_items,
                          uint32_t limbs, uint32_t log2n) {
    if (!out || !in || !plain) return fail(DPFHE_INVALID_ARGUMENT, what, "null buffer");
    if (comps != 2 && comps != 3) return fail(DPFHE_INVALID_ARGUMENT, what, "ciphertexts have 2 or 3 components");
    if (batch == 0 || plain_items == 0 || batch % plain_items) return fail(DPFHE_INVALID_ARGUMENT, what, "batch must be a positive multiple of plain_items");
    if (!ItemChunkMap::pairs(batch, log2n).ok) return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    const size_t poly = (size_t)limbs << log2n, words = batch * comps * poly;
    if (out != in && overlaps(out, words, in, words)) return fail(DPFHE_INVALID_ARGUMENT, what, "out and in overlap without being the same buffer");
    if (overlaps(out, words, plain, plain_items * poly)) return fail(DPFHE_INVALID_ARGUMENT, what, "out overlaps the plaintext");
    return DPFHE_SUCCESS;
}

extern "C" int dpfhe_add_plain(dpfhe_ctx* c, uint64_t* d_out, const uint64_t* d_in, const uint64_t* d_plain, size_t batch, size_t comps, size_t plain_items,
                               int negate, void* stream) {
    static const char* what = "dpfhe_add_plain";
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    if (int rc = add_plain_args(what, d_out, d_in, d_plain, batch, comps, plain_items, c->n_limbs, c->log2n)) return rc;
    if (misaligned(d_out) || misaligned(d_in) || misaligned(d_plain)) return fail(DPFHE_INVALID_ARGUMENT, what, "misaligned buffer");
    DPFHE_ON_DEVICE(c, what);
    if (launch_add_plain((int)c->log2n, d_out, d_in, d_plain, batch, (u32)comps, c->n_limbs, batch / plain_items, negate != 0, c->lc,
                         static_cast<hipStream_t>(stream)))
        return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    return check_launch("add_plain kernel launch");
}

extern "C" int dpfhe_add_plain_host(const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n, uint64_t* out, const uint64_t* in, const uint64_t* plain,
                                    size_t batch, size_t comps, size_t plain_items, int negate) {
    static const char* what = "dpfhe_add_plain_host";
    if (!moduli) return fail(DPFHE_INVALID_ARGUMENT, what, "null moduli");
    if (int rc = check_host_ring(what, moduli, n_limbs, log2_n)) return rc;
    if (int rc = add_plain_args(what, out, in, plain, batch, comps, plain_items, n_limbs, log2_n)) return rc;
    const size_t n = (size_t)1 << log2_n;
    for (size_t i = 0; i < plain_items * n_limbs; ++i)
        for (size_t k = 0; k < n; ++k)
            if (plain[i * n + k] >= moduli[i % n_limbs]) return fail(DPFHE_INVALID_ARGUMENT, what, "plaintext words must be canonical residues");
    add_plain_host((int)log2_n, moduli, n_limbs, out, in, plain, batch, (u32)comps, batch / plain_items, negate != 0);
    return DPFHE_SUCCESS;
}
