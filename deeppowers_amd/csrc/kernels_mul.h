// kernels_mul.h - the multiply at ring degrees above 8192, and sums of products, complement products and all-pairs (outer) products at every ring degree (device).
// Included by cabi_mul.hip only.
//
// The fused multiply kernels of kernels.h keep whole polynomials in one workgroup's registers and LDS, which stops at
// N = 8192 (one 1024-thread workgroup at N = 16384 has 128 VGPRs per thread; four polynomials of 16 words per thread do not fit).
// Above, the same operation is COMPOSED (cabi_mul.hip: ct_mul_composed) from the batched transforms of kernels.h / ntt_top.h and the
// streaming kernel below: one HBM pass, 16 bytes per lane, one workgroup per 512-word chunk of one residue polynomial.  All words canonical
// in and out; results equal the fused kernels' (tests/test_gpu_parity.py (test_large_rings_multiply_and_key_switch_composed_behind_the_c_abi and the slicing test)).
#pragma once
#include <hip/hip_runtime.h>

#include "modarith.h"
#include "mul_complement.h"
#include "mul_outer.h"
#include "mul_sum.h"
#include "workmap.h"

namespace dpfhe {

// (a0, a1) (x) (b0, b1) -> (a0 b0, a0 b1 + a1 b0, a1 b1), NTT domain.  a2, b2: [batch][2][L][N]; out3: [batch][3][L][N].
template <class Arith>
__global__ __launch_bounds__(256) void tensor3_kernel(u64* __restrict__ out3, const u64* __restrict__ a2, const u64* __restrict__ b2, const LimbConst* lcs,
                                                      int n_limbs, int n, int chunks) {
    const ChunkWork wk = chunk_work(blockIdx.x, chunks, n_limbs);
    const int chunk = wk.chunk, limb = wk.limb;
    const size_t pair = wk.poly;
    const int w0 = chunk * 512 + threadIdx.x * 2;
    if (w0 >= n) return;
    const LimbConst lc = lcs[limb];
    const size_t poly = (size_t)n_limbs * n, off = (size_t)limb * n + w0;
    const U64x2 a0 = *reinterpret_cast<const U64x2*>(a2 + (pair * 2 + 0) * poly + off), a1 = *reinterpret_cast<const U64x2*>(a2 + (pair * 2 + 1) * poly + off);
    const U64x2 b0 = *reinterpret_cast<const U64x2*>(b2 + (pair * 2 + 0) * poly + off), b1 = *reinterpret_cast<const U64x2*>(b2 + (pair * 2 + 1) * poly + off);
    U64x2 d0, d1, d2;
    d0.a = Arith::mul_var(a0.a, b0.a, lc); d0.b = Arith::mul_var(a0.b, b0.b, lc);
    d1.a = add_mod(Arith::mul_var(a0.a, b1.a, lc), Arith::mul_var(a1.a, b0.a, lc), lc.q);
    d1.b = add_mod(Arith::mul_var(a0.b, b1.b, lc), Arith::mul_var(a1.b, b0.b, lc), lc.q);
    d2.a = Arith::mul_var(a1.a, b1.a, lc); d2.b = Arith::mul_var(a1.b, b1.b, lc);
    *reinterpret_cast<U64x2*>(out3 + (pair * 3 + 0) * poly + off) = d0;
    *reinterpret_cast<U64x2*>(out3 + (pair * 3 + 1) * poly + off) = d1;
    *reinterpret_cast<U64x2*>(out3 + (pair * 3 + 2) * poly + off) = d2;
}

// A SUM of tensor products, one pass: out3[g] (+)= sum_{k < terms} a[g][k] (x) b[g][k], NTT domain, canonical in and out (mul_sum.h holds the lane arithmetic
// and its bounds).  a2: [groups][terms][2][L][N]; b2: the same, or [terms][2][L][N] read by every group (b_shared); out3: [groups][3][L][N].  The tensor
// product is bilinear, so whatever follows - inverse transforms, key switch, rescale - is paid once per group, not once per term.  `accumulate`: the sums
// continue from the canonical words already in out3 (a group cut into ranges of terms).  One workgroup per (group, limb, 512-word chunk), 16 bytes per lane.
// kMulSumDepth terms are loaded before the first of them is used: 16 independent 16-byte loads per lane in flight (a loop that waits on one term's four
// loads per iteration leaves the memory pipeline idle for most of a round trip).  Traffic per group and limb in rows of N words: 4 terms + 3, or 2 terms + 3
// and the shared rows once per XCD from HBM (groups of one limb and chunk are `L chunks` ids apart: the shared rows are L2 hits at best, not guaranteed).
constexpr int kMulSumDepth = 4;
template <class Arith>
__global__ __launch_bounds__(256) void tensor3_sum_kernel(u64* __restrict__ out3, const u64* __restrict__ a2, const u64* __restrict__ b2, const LimbConst* lcs,
                                                          int n_limbs, int n, int chunks, int terms, int b_shared, int accumulate) {
    typedef MulSumLane<Arith> Lane;
    const ChunkWork wk = chunk_work(blockIdx.x, chunks, n_limbs);
    const int chunk = wk.chunk, limb = wk.limb;
    const size_t group = wk.poly;
    const int w0 = chunk * 512 + threadIdx.x * 2;
    if (w0 >= n) return;
    const LimbConst lc = lcs[limb];
    const size_t poly = (size_t)n_limbs * n, off = (size_t)limb * n + w0;
    const u64* pa = a2 + group * (size_t)terms * 2 * poly + off;
    const u64* pb = b2 + (b_shared ? 0 : group * (size_t)terms * 2 * poly) + off;
    u64* po = out3 + group * 3 * poly + off;
    U64x2 p0{0, 0}, p1{0, 0}, p2{0, 0};
    if (accumulate) {
        p0 = *reinterpret_cast<const U64x2*>(po); p1 = *reinterpret_cast<const U64x2*>(po + poly); p2 = *reinterpret_cast<const U64x2*>(po + 2 * poly);
    }
    typename Lane::Acc sa = Lane::init(p0.a, p1.a, p2.a, lc), sb = Lane::init(p0.b, p1.b, p2.b, lc);
    int k = 0;
    for (; k + kMulSumDepth <= terms; k += kMulSumDepth) {
        U64x2 a0[kMulSumDepth], a1[kMulSumDepth], b0[kMulSumDepth], b1[kMulSumDepth];
#pragma unroll
        for (int u = 0; u < kMulSumDepth; ++u) {
            const size_t t = (size_t)(k + u) * 2 * poly;
            a0[u] = *reinterpret_cast<const U64x2*>(pa + t); a1[u] = *reinterpret_cast<const U64x2*>(pa + t + poly);
            b0[u] = *reinterpret_cast<const U64x2*>(pb + t); b1[u] = *reinterpret_cast<const U64x2*>(pb + t + poly);
        }
#pragma unroll
        for (int u = 0; u < kMulSumDepth; ++u) {
            Lane::term(sa, a0[u].a, a1[u].a, b0[u].a, b1[u].a, lc);
            Lane::term(sb, a0[u].b, a1[u].b, b0[u].b, b1[u].b, lc);
        }
    }
    for (; k < terms; ++k) {   // the ragged end: fewer than kMulSumDepth terms
        const size_t t = (size_t)k * 2 * poly;
        const U64x2 a0 = *reinterpret_cast<const U64x2*>(pa + t), a1 = *reinterpret_cast<const U64x2*>(pa + t + poly);
        const U64x2 b0 = *reinterpret_cast<const U64x2*>(pb + t), b1 = *reinterpret_cast<const U64x2*>(pb + t + poly);
        Lane::term(sa, a0.a, a1.a, b0.a, b1.a, lc);
        Lane::term(sb, a0.b, a1.b, b0.b, b1.b, lc);
    }
    U64x2 d0, d1, d2;
    Lane::finish(sa, lc, d0.a, d1.a, d2.a);
    Lane::finish(sb, lc, d0.b, d1.b, d2.b);
    *reinterpret_cast<U64x2*>(po) = d0;
    *reinterpret_cast<U64x2*>(po + poly) = d1;
    *reinterpret_cast<U64x2*>(po + 2 * poly) = d2;
}

// Products that share a COMPLEMENT factor, one pass (Goldschmidt's n_j <- n_j F, D <- D F with F = 2 - D): per group g
//   f = (kappa_l - b0, -b1),   out3[g * terms + k] = a[g][k] (x) f  (k < terms),   out_self[g] = b[g] (x) f  (when out_self is not null),
// NTT domain, canonical in and out (mul_complement.h holds the lane arithmetic).  a2: [groups][terms][2][L][N]; b2: [groups][2][L][N]; kappa: [L] canonical
// residues; out3: [groups * terms][3][L][N]; out_self: [groups][3][L][N] or null.  The factor is never written and never transformed: the lane forms it ONCE
// per group from b's two words and walks the group's items, kMulSumDepth items' loads (8 x 16 bytes per lane) in flight before the first is used, three
// 16-byte stores per item; the self product takes its operand from the registers b already sits in.  One workgroup per (group, limb, 512-word chunk): the
// grid is mul_complement_grid (workmap.h).  Traffic per group and limb in rows of N words: 2 terms + 2 read, 3 (terms + self) written.
template <class Arith>
__global__ __launch_bounds__(256) void tensor3_complement_kernel(u64* __restrict__ out3, u64* __restrict__ out_self, const u64* __restrict__ a2,
                                                                 const u64* __restrict__ b2, const u64* __restrict__ kappa, const LimbConst* lcs, int n_limbs, int n,
                                                                 int chunks, int terms) {
    typedef MulComplementLane<Arith> Lane;
    const ChunkWork wk = chunk_work(blockIdx.x, chunks, n_limbs);
    const int chunk = wk.chunk, limb = wk.limb;
    const size_t group = wk.poly;
    const int w0 = chunk * 512 + threadIdx.x * 2;
    if (w0 >= n) return;
    const LimbConst lc = lcs[limb];
    const u64 kap = kappa[limb];
    const size_t poly = (size_t)n_limbs * n, off = (size_t)limb * n + w0;
    const u64* pb = b2 + group * 2 * poly + off;
    const u64* pa = a2 + group * (size_t)terms * 2 * poly + off;
    u64* po = out3 + group * (size_t)terms * 3 * poly + off;
    const U64x2 b0 = *reinterpret_cast<const U64x2*>(pb), b1 = *reinterpret_cast<const U64x2*>(pb + poly);
    const typename Lane::Factor fa = Lane::factor(b0.a, b1.a, kap, lc), fb = Lane::factor(b0.b, b1.b, kap, lc);
    auto product = [&](u64* o, const U64x2& x0, const U64x2& x1) {
        U64x2 d0, d1, d2;
        Lane::item(x0.a, x1.a, fa, lc, d0.a, d1.a, d2.a);
        Lane::item(x0.b, x1.b, fb, lc, d0.b, d1.b, d2.b);
        *reinterpret_cast<U64x2*>(o) = d0;
        *reinterpret_cast<U64x2*>(o + poly) = d1;
        *reinterpret_cast<U64x2*>(o + 2 * poly) = d2;
    };
    int k = 0;
    for (; k + kMulSumDepth <= terms; k += kMulSumDepth) {
        U64x2 x0[kMulSumDepth], x1[kMulSumDepth];
#pragma unroll
        for (int u = 0; u < kMulSumDepth; ++u) {
            const size_t t = (size_t)(k + u) * 2 * poly;
            x0[u] = *reinterpret_cast<const U64x2*>(pa + t); x1[u] = *reinterpret_cast<const U64x2*>(pa + t + poly);
        }
#pragma unroll
        for (int u = 0; u < kMulSumDepth; ++u) product(po + (size_t)(k + u) * 3 * poly, x0[u], x1[u]);
    }
    for (; k < terms; ++k) {   // the ragged end: fewer than kMulSumDepth items
        const size_t t = (size_t)k * 2 * poly;
        const U64x2 x0 = *reinterpret_cast<const U64x2*>(pa + t), x1 = *reinterpret_cast<const U64x2*>(pa + t + poly);
        product(po + (size_t)k * 3 * poly, x0, x1);
    }
    if (out_self) product(out_self + group * 3 * poly + off, b0, b1);
}

// ALL PAIRS of a_count resident operands (queries) and b_count streamed ones (keys), one pass: the tensor product a[i] (x) b[j] of every pair, NTT domain,
// canonical in and out (mul_outer.h holds the lane arithmetic).  a2: [a_count][2][L][N]; b2: [b_count][2][L][N]; out3: the WHOLE output of the call, pair
// (gi, gj) = (a_off + i, b_off + j) at item gi * b_total + gj, or under `causal` pair (gi, gj <= gi) at item gi (gi + 1) / 2 + gj (workmap.h MulOuterMap::item:
// a_off, b_off place a launch over ranges of the operands inside the whole; every index is size_t).  A workgroup owns one 512-word chunk of one limb of a TILE
// of kMulOuterTile queries (MulOuterMap::decode: the tiles of a (limb, chunk) share one XCD): the tile is loaded once and prepared in registers, then the
// workgroup walks the keys, kMulOuterDepth keys' loads (8 x 16 bytes per lane) in flight before the first is used, three 16-byte stores per product.  A ragged
// last tile skips its missing rows; the ragged end of the key loop runs key by key; under `causal` a tile walks the keys up to its last row's and skips the
// pairs above the diagonal (all three predicates are uniform over the workgroup).  Traffic per limb in rows of N words: 2 a_count + 2 b_count ceil(a_count /
// tile) read - the re-reads L2 hits -, 3 per pair written.
constexpr int kMulOuterDepth = 4;   // keys whose loads are in flight before the first is used (its own constant: the block of keys below is written out)
template <class Arith>
__global__ __launch_bounds__(256) void tensor3_outer_kernel(u64* __restrict__ out3, const u64* __restrict__ a2, const u64* __restrict__ b2, const LimbConst* lcs, int n_limbs,
                                                            int n, int chunks, unsigned tiles, size_t a_count, size_t b_count, size_t a_off, size_t b_off, size_t b_total,
                                                            int causal) {
    typedef MulOuterLane<Arith> Lane;
    const MulOuterWork wk = MulOuterMap::decode(blockIdx.x, tiles, (unsigned)n_limbs, (unsigned)chunks);
    if (!wk.live) return;
    const int w0 = wk.chunk * 512 + threadIdx.x * 2;
    if (w0 >= n) return;
    const size_t r0 = wk.tile * kMulOuterTile;
    const size_t keys = MulOuterMap::keys(r0, a_count, b_count, a_off, b_off, causal != 0);
    if (keys == 0) return;   // a tile wholly above the diagonal
    const int rows = a_count - r0 < (size_t)kMulOuterTile ? (int)(a_count - r0) : kMulOuterTile;
    const LimbConst lc = lcs[wk.limb];
    const size_t poly = (size_t)n_limbs * n, off = (size_t)wk.limb * n + w0;
    const u64* pb = b2 + off;
    typename Lane::Prepared qa[kMulOuterTile], qb[kMulOuterTile];   // the tile: the lane's first and second word of every row
#pragma unroll
    for (int t = 0; t < kMulOuterTile; ++t) {
        const u64* pa = a2 + (r0 + (t < rows ? t : 0)) * 2 * poly + off;   // a missing row re-reads the first: no load out of bounds, no product, no store
        const U64x2 a0 = *reinterpret_cast<const U64x2*>(pa), a1 = *reinterpret_cast<const U64x2*>(pa + poly);
        qa[t] = Lane::prepare(a0.a, a1.a, lc);
        qb[t] = Lane::prepare(a0.b, a1.b, lc);
    }
    // key j against every row of the tile (always inlined: a call would take the key buffers and the tile through memory)
    auto products = [&](size_t j, const U64x2& b0, const U64x2& b1) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < kMulOuterTile; ++t) {
            if (t >= rows || !MulOuterMap::writes(r0 + t, j, a_off, b_off, causal != 0)) continue;
            U64x2 d0, d1, d2;
            Lane::product(qa[t], b0.a, b1.a, lc, d0.a, d1.a, d2.a);
            Lane::product(qb[t], b0.b, b1.b, lc, d0.b, d1.b, d2.b);
            u64* o = out3 + MulOuterMap::item(r0 + t, j, a_off, b_off, b_total, causal != 0) * 3 * poly + off;
            *reinterpret_cast<U64x2*>(o) = d0;
            *reinterpret_cast<U64x2*>(o + poly) = d1;
            *reinterpret_cast<U64x2*>(o + 2 * poly) = d2;
        }
    };
    size_t j = 0;
    for (; j + kMulOuterDepth <= keys; j += kMulOuterDepth) {
        U64x2 b0[kMulOuterDepth], b1[kMulOuterDepth];
#pragma unroll
        for (int u = 0; u < kMulOuterDepth; ++u) {
            const size_t t = (j + u) * 2 * poly;
            b0[u] = *reinterpret_cast<const U64x2*>(pb + t); b1[u] = *reinterpret_cast<const U64x2*>(pb + t + poly);
        }
        // written out: 4 keys x 4 rows x 2 words of products are past the size up to which hipcc unrolls a loop on request, and a loop left rolled
        // keeps b0 / b1 in scratch memory
        static_assert(kMulOuterDepth == 4, "the products of a block of keys are written out");
        products(j, b0[0], b1[0]);
        products(j + 1, b0[1], b1[1]);
        products(j + 2, b0[2], b1[2]);
        products(j + 3, b0[3], b1[3]);
    }
    for (; j < keys; ++j) {   // the ragged end: fewer than kMulOuterDepth keys
        const size_t t = j * 2 * poly;
        const U64x2 b0 = *reinterpret_cast<const U64x2*>(pb + t), b1 = *reinterpret_cast<const U64x2*>(pb + t + poly);
        products(j, b0, b1);
    }
}

}  // namespace dpfhe
