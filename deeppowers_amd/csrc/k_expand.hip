// k_expand.hip - seeded uniform polynomials (expand.h): the device kernel, its launcher, the host twin and the entries of include/dpfhe.h.
//
// One lane per ChaCha20 block: a lane produces 4 coefficients (32 contiguous bytes, two 16-byte stores) and consecutive lanes write
// consecutive blocks, so the stores coalesce without LDS.  A workgroup covers one (item, limb) range of blocks (workmap.h ItemChunkMap: outer =
// item x limb, N / 4 lanes), so the limb's constants are workgroup-uniform scalar loads; the seed's key words are kernel arguments (SGPRs).  No loads
// from memory besides the LimbConst: the kernel is VALU-bound (20 ChaCha rounds + four exact 128-bit reductions per lane).
#include <cstring>

#include "cabi.h"
#include "expand.h"

namespace dpfhe {

// lane j of (item, limb) computes ChaCha block j
__global__ __launch_bounds__(256) void expand_uniform_kernel(u64* __restrict__ buf, const ExpandKey key, const LimbConst* __restrict__ lc, u32 first_item,
                                                             u32 comp, u32 comps, u32 n_limbs, u32 log2n, u32 log2_chunks) {
    const ItemChunkWork w = ItemChunkMap::decode(blockIdx.x, log2_chunks);
    const u32 limb = w.outer % n_limbs, b = w.outer / n_limbs;
    const u32 j = ItemChunkMap::lane(w.chunk, blockDim.x, threadIdx.x);
    const u64 q = lc[limb].q, br_hi = lc[limb].br_hi, br_lo = lc[limb].br_lo;
    u64 v[4];
    expand_block(key, j, first_item + b, limb, comp, q, br_hi, br_lo, v);
    u64* p = buf + ((((size_t)b * comps + comp) * n_limbs + limb) << log2n) + 4 * (size_t)j;
    reinterpret_cast<u64x2_t*>(p)[0] = u64x2_t{v[0], v[1]};
    reinterpret_cast<u64x2_t*>(p)[1] = u64x2_t{v[2], v[3]};
}

// device: component `comp` of items [0, batch) of buf [batch][comps][L][N] = expand(seed, first_item + b, limb, comp); 0, or -1 if the grid is too large
static int launch_expand_uniform(int log2n, u64* buf, size_t batch, size_t comps, u32 comp, u32 n_limbs, const LimbConst* lc, const ExpandKey& key, u32 first_item,
                          hipStream_t s) {
    // the ChaCha blocks of one residue polynomial (log2n >= 8: at least one wave); batch <= 2^32 (expand_args), so batch * n_limbs cannot wrap
    const ItemChunkPlan p = ItemChunkMap::plan(batch * n_limbs, 1u << (log2n - 2), 256u);
    if (!p.ok) return -1;
    hipLaunchKernelGGL(expand_uniform_kernel, dim3((unsigned)p.grid), dim3(p.threads), 0, s, buf, key, lc, first_item, comp, (u32)comps, n_limbs, (u32)log2n,
                       p.log2_chunks);
    return 0;
}

void expand_uniform_host(int log2n, const u64* moduli, u32 n_limbs, u64* out, size_t batch, size_t comps, u32 comp, const ExpandKey& key, u32 first_item) {
    const size_t n = (size_t)1 << log2n;
    for (u32 l = 0; l < n_limbs; ++l) {
        const u64 q = moduli[l];
        const unsigned __int128 br = (~(unsigned __int128)0) / q;   // floor(2^128 / q): q is odd, never a power of two
        const u64 br_hi = (u64)(br >> 64), br_lo = (u64)br;
        for (size_t b = 0; b < batch; ++b) {
            u64* p = out + ((b * comps + comp) * n_limbs + l) * n;
            for (u32 j = 0; j < (u32)(n / 4); ++j) expand_block(key, j, first_item + (u32)b, l, comp, q, br_hi, br_lo, p + 4 * (size_t)j);
        }
    }
}

}  // namespace dpfhe

// ------------------------------------------------------------------------------------------------
// seeded uniform polynomials (expand.h, k_expand.hip): component `component` of items 0 .. batch-1 = expand(seed, first_item + b, limb, component)
static int expand_args(const char* what, const void* buf, size_t components, uint32_t component, const uint8_t* seed, uint64_t first_item, size_t batch,
                       ExpandKey& key) {
    if (!buf || !seed) return fail(DPFHE_INVALID_ARGUMENT, what, "null buffer or seed");
    if (component >= components) return fail(DPFHE_INVALID_ARGUMENT, what, "component must be < components");
    if (first_item > ((uint64_t)1 << 32) || batch > ((uint64_t)1 << 32) - first_item) return fail(DPFHE_INVALID_ARGUMENT, what, "first_item + batch must be <= 2^32");
    std::memcpy(key.w, seed, 32);   // little-endian words (x86-64 and gfx950 hosts)
    return DPFHE_SUCCESS;
}

extern "C" int dpfhe_expand_uniform(dpfhe_ctx* c, uint64_t* d_buf, size_t batch, size_t components, uint32_t component, const uint8_t seed[32],
                                    uint64_t first_item, void* stream) {
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_expand_uniform", "null context");
    ExpandKey key;
    if (int rc = expand_args("dpfhe_expand_uniform", d_buf, components, component, seed, first_item, batch, key)) return rc;
    if (misaligned(d_buf)) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_expand_uniform", "misaligned buffer");
    if (batch == 0) return DPFHE_SUCCESS;
    DPFHE_ON_DEVICE(c, "dpfhe_expand_uniform");
    // c->lc holds q and floor(2^128 / q) of every limb, whatever its class
    if (launch_expand_uniform((int)c->log2n, d_buf, batch, components, component, c->n_limbs, c->lc, key, (uint32_t)first_item, static_cast<hipStream_t>(stream)))
        return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_expand_uniform", "batch too large for one launch");
    return check_launch("expand_uniform kernel launch");
}

extern "C" int dpfhe_expand_uniform_host(const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n, uint64_t* out, size_t batch, size_t components,
                                         uint32_t component, const uint8_t seed[32], uint64_t first_item) {
    if (!moduli) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_expand_uniform_host", "null moduli");
    ExpandKey key;
    if (int rc = expand_args("dpfhe_expand_uniform_host", out, components, component, seed, first_item, batch, key)) return rc;
    if (int rc = check_host_ring("dpfhe_expand_uniform_host", moduli, n_limbs, log2_n)) return rc;
    expand_uniform_host((int)log2_n, moduli, n_limbs, out, batch, components, component, key, (uint32_t)first_item);
    return DPFHE_SUCCESS;
}
