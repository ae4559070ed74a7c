// kernels_rotate_sum.h - the SUM of an item's hoisted rotations over Q P, output-stationary (include/dpfhe.h dpfhe_rotate_sum_hoisted).
// Included by cabi_rotate_sum.hip only.  No reference counterpart.
#pragma once
#include <hip/hip_runtime.h>

#include "launch.h"
#include "modarith.h"
#include "stream_access.h"
#include "workmap.h"

namespace dpfhe {

// Per item t and limb l of the extended basis, NTT domain, forward-output order (the sum mod q_l of blocks 1 .. R of dpfhe_rotate_hoisted_qp, canonical):
//   S_t.c0 = sum_{r<R} ( sum_{j<Ld} perm_{g_r}(digit_{t,j}) (.) key_{r,j,0} + P perm_{g_r}(NTT(c0_t)) ),   S_t.c1 = sum_{r<R} sum_{j<Ld} perm_{g_r}(digit_{t,j}) (.) key_{r,j,1}.
// hoisted_qp_stream_kernel (kernels_rotate.h) is source-stationary and writes one Q P block per rotation; here a workgroup owns ONE OUTPUT segment (256 threads
// x one 16-byte pair) of one limb for a tile of up to kQpSumTile items (workmap.h QpSumMap) and keeps its 2 x 2 x kQpSumTile accumulators in registers over
// all R (Ld + 1) terms of component 0 and R Ld of component 1: each output word is stored once and no rotation's block ever exists.
//   - per rotation the thread derives its source pair and swap flag from its output pair (QpSumMap::source); a rotation's sources lie in one segment;
//   - the terms of a rotation are j = 0 .. Ld - 1 (digit j x key (r, j)) and, on the data limbs, j = Ld (c0 x P: no key);
//   - a key pair (e0, e1) of (r, j) is loaded once and split once for the whole tile; a digit word's split serves both key components;
//   - the loads of term u + 1 are issued before term u multiplies (the last term re-requests itself: cache hits instead of a branch);
//   - fold limbs: Dot30 columns, one dot30_fold per kDot30Period terms counted ACROSS rotations; other classes: mul_var + add_mod per term.
// Traffic per item: R (Ld + 1) digit / input rows gathered (each digit segment by R different workgroups: L2 and the Infinity Cache are asked to absorb
// that), R 2 Ld key rows per TILE, 2 rows written - per limb.
struct QpSumElts { unsigned v[kMaxGaloisBatch]; };

template <class Arith>
__global__ __launch_bounds__(256) void hoisted_qp_sum_kernel(u64* __restrict__ out, const u64* __restrict__ digits, const u64* __restrict__ xntt,
                                                             const u64* __restrict__ keys, size_t key_stride, QpSumElts elts, unsigned n_rot, unsigned n_items,
                                                             unsigned tiles, u64 p_special, const LimbConst* __restrict__ lcs, int n_limbs, int log2n) {
    constexpr int TI = kQpSumTile;
    const int L = n_limbs, Ld = L - 1;
    const QpGeo geo = QpSumMap::geo(log2n);
    const QpSumWork wk = QpSumMap::decode(blockIdx.x, geo, (unsigned)L, tiles);
    if (!wk.live) return;
    const int limb = wk.limb;
    const LimbConst lc = lcs[limb];
    const size_t N = geo.n, row = (size_t)L * N / 2;   // a digit's or a key component's L rows, in 16-byte units
    const unsigned t0 = wk.tile * (unsigned)TI, rows = n_items - t0 < (unsigned)TI ? n_items - t0 : (unsigned)TI;   // workgroup-uniform
    const QpPair po = QpSumMap::source(1u, wk.oseg, threadIdx.x, geo);   // (the output side alone: the identity's source is the pair itself)
    const bool ok = po.ok;
    const unsigned mo = po.out;
    const int J = limb < Ld ? Ld + 1 : Ld;   // terms per rotation: the P c0 term is absent on the special limb
    const unsigned total = n_rot * (unsigned)J;
    const U64x2* dig = reinterpret_cast<const U64x2*>(digits + ((size_t)t0 * Ld * L + limb) * N);   // item i, digit j at + (i Ld + j) * row
    const U64x2* cin = reinterpret_cast<const U64x2*>(xntt + ((size_t)t0 * 2 * Ld + limb) * N);     // item i's c0 at + i * 2 Ld N words
    const U64x2* evk = reinterpret_cast<const U64x2*>(keys + (size_t)limb * N) + mo;                // key (r, j, comp) at + r key_stride words + (2 j + comp) * row

    // term (r, j) into (x, e0, e1): the tile's gathered pairs and, for a digit term, the key pairs; ms = the rotation's source pair
    auto request = [&](U64x2 (&x)[TI], U64x2& e0, U64x2& e1, unsigned r, int j, unsigned ms) {
        if (!ok) return;
        if (j < Ld) {
            const U64x2* kp = evk + ((size_t)r * key_stride / 2 + (size_t)(2 * j) * row);
            e0 = kp[0];
            e1 = kp[row];
#pragma unroll
            for (int i = 0; i < TI; ++i)
                if ((unsigned)i < rows) x[i] = dig[((size_t)i * Ld + j) * row + ms];
        } else {
#pragma unroll
            for (int i = 0; i < TI; ++i)
                if ((unsigned)i < rows) x[i] = cin[(size_t)i * Ld * N + ms];
        }
    };

    U64x2 x[TI], e0{0, 0}, e1{0, 0};
#pragma unroll
    for (int i = 0; i < TI; ++i) x[i] = U64x2{0, 0};
    unsigned r = 0;
    int j = 0;
    QpPair pm = QpSumMap::source(elts.v[0], wk.oseg, threadIdx.x, geo);
    bool sw = pm.swap;
    request(x, e0, e1, 0u, 0, pm.src);

    // what differs between the arithmetic classes: the accumulators, one term's products, the final words
    typedef FoldArith::Dot30 Dot;
    typedef FoldArith::Half30 Half;
    Dot s0[TI][2], s1[TI][2];      // fold: lazy columns ...
    u64 r0[TI][2], r1[TI][2];      // ... and the folded running words; generic: the canonical running sums
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int h = 0; h < 2; ++h) { s0[i][h] = Dot{0, 0, 0}; s1[i][h] = Dot{0, 0, 0}; r0[i][h] = 0; r1[i][h] = 0; }
    int terms = 0;
    auto fold_all = [&]() {
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                r0[i][h] = FoldArith::dot30_fold(s0[i][h], r0[i][h], lc); s0[i][h] = Dot{0, 0, 0};
                r1[i][h] = FoldArith::dot30_fold(s1[i][h], r1[i][h], lc); s1[i][h] = Dot{0, 0, 0};
            }
        terms = 0;
    };
    const u64 pmod = Arith::kFold ? FoldArith::canon(p_special, lc) : ShoupArith::mul_var(p_special, 1, lc);
    auto accw = [&](u64 acc, u64 a, u64 b) -> u64 { return add_mod(acc, ShoupArith::mul_var(a, b, lc), lc.q); };

#pragma unroll 1
    for (unsigned u = 0; u < total; ++u) {
        // the next term: (r, j + 1), or (r + 1, 0) with that rotation's map; the last term re-requests itself
        unsigned rn = r;
        int jn = j + 1;
        QpPair pn = pm;
        if (jn == J) {
            if (r + 1 < n_rot) {
                rn = r + 1;
                jn = 0;
                pn = QpSumMap::source(elts.v[rn], wk.oseg, threadIdx.x, geo);
            } else {
                jn = j;
            }
        }
        U64x2 xn[TI], e0n = e0, e1n = e1;
#pragma unroll
        for (int i = 0; i < TI; ++i) xn[i] = x[i];
        request(xn, e0n, e1n, rn, jn, pn.src);

        if constexpr (Arith::kFold) {
            // all operands are canonical residues (< 2^60), which is what split30 needs
            if (terms == FoldArith::kDot30Period) fold_all();   // workgroup-uniform
            ++terms;
            if (j < Ld) {
                const Half k0a = FoldArith::split30(e0.a), k0b = FoldArith::split30(e0.b), k1a = FoldArith::split30(e1.a), k1b = FoldArith::split30(e1.b);
#pragma unroll
                for (int i = 0; i < TI; ++i) {
                    if ((unsigned)i >= rows) continue;
                    const Half xa = FoldArith::split30(sw ? x[i].b : x[i].a), xb = FoldArith::split30(sw ? x[i].a : x[i].b);
                    FoldArith::dot30_mac(s0[i][0], xa, k0a);
                    FoldArith::dot30_mac(s0[i][1], xb, k0b);
                    FoldArith::dot30_mac(s1[i][0], xa, k1a);
                    FoldArith::dot30_mac(s1[i][1], xb, k1b);
                }
            } else {
                const Half hp = FoldArith::split30(pmod);
#pragma unroll
                for (int i = 0; i < TI; ++i) {
                    if ((unsigned)i >= rows) continue;
                    FoldArith::dot30_mac(s0[i][0], FoldArith::split30(sw ? x[i].b : x[i].a), hp);
                    FoldArith::dot30_mac(s0[i][1], FoldArith::split30(sw ? x[i].a : x[i].b), hp);
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                if ((unsigned)i >= rows) continue;
                const u64 xa = sw ? x[i].b : x[i].a, xb = sw ? x[i].a : x[i].b;
                if (j < Ld) {
                    r0[i][0] = accw(r0[i][0], xa, e0.a); r0[i][1] = accw(r0[i][1], xb, e0.b);
                    r1[i][0] = accw(r1[i][0], xa, e1.a); r1[i][1] = accw(r1[i][1], xb, e1.b);
                } else {
                    r0[i][0] = accw(r0[i][0], xa, pmod); r0[i][1] = accw(r0[i][1], xb, pmod);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < TI; ++i) x[i] = xn[i];
        e0 = e0n; e1 = e1n;
        r = rn; j = jn; pm = pn; sw = pn.swap;
    }
    if (!ok) return;
    if constexpr (Arith::kFold) {
        fold_all();
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) { r0[i][h] = FoldArith::canon_small(r0[i][h], lc); r1[i][h] = FoldArith::canon_small(r1[i][h], lc); }
    }
    // written once, read by the inverse transform's launch: around the caches the keys and digits live in
#pragma unroll
    for (int i = 0; i < TI; ++i) {
        if ((unsigned)i >= rows) continue;
        U64x2* o0 = reinterpret_cast<U64x2*>(out + (((size_t)(t0 + i) * 2 + 0) * L + limb) * N) + mo;
        st_vec<true>(o0, U64x2{r0[i][0], r0[i][1]});
        st_vec<true>(o0 + row, U64x2{r1[i][0], r1[i][1]});
    }
}

}  // namespace dpfhe
