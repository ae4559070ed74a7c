// kernels_rotate_sum.h - the SUM of an item's hoisted rotations over Q P, output-stationary (include/dpfhe.h dpfhe_rotate_sum_hoisted and, on grouped digits,
// dpfhe_rotate_sum_hoisted_grouped).
// Included by cabi_rotate_sum.hip only.  No reference counterpart.
#pragma once
#include <hip/hip_runtime.h>

#include "base_ext.h"
#include "launch.h"
#include "modarith.h"
#include "rotate_sum.h"
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
//   - the loads of term u + 1 are issued before term u multiplies (the last term re-requests itself: cache hits instead of a branch), and the next
//     rotation's map is made one term ahead of its first use ("How the term loop is cut" below);
//   - fold limbs: Dot30 columns, one dot30_fold per kDot30Period terms counted ACROSS rotations; other classes: mul_var + add_mod per term.  That
//     arithmetic - accumulators, a term's products, the period, the final words - is rotate_sum.h QpSumLane, which tools/emulate_rotate_sum.cpp runs on the
//     CPU; this kernel keeps the loads, the map, the prefetch and the stores.
// Traffic per item: R (Ld + 1) digit / input rows gathered (each digit segment by R different workgroups: L2 and the Infinity Cache are asked to absorb
// that), R 2 Ld key rows per TILE, 2 rows written - per limb.
struct QpSumElts { unsigned v[kMaxGaloisBatch]; };

// The GROUPED form (include/dpfhe.h dpfhe_rotate_sum_hoisted_grouped) is the same sum over another digit set: n_dig = beta = ceil(Ld / alpha) centred group
// digits per item (keyswitch_grouped.h) under alpha special limbs, so J = beta + 1 terms per rotation on a data limb and beta on each special limb, digit rows
// strided by beta, a key of beta 2 L rows, and P mod q_l read per limb from the division block of the grouped table.  ONE body, qp_sum_body, serves both; what a
// form owns is its P operand:
//   QpSumOneP    the one special prime as a kernel argument, reduced per limb (hoisted_qp_sum_kernel);
//   QpSumTableP  Q_mod[l] = P mod q_l of the division block, already canonical, in global memory: a scalar load (hoisted_qp_sum_grouped_kernel).
// How the term loop is cut.  With 4 or 5 terms per rotation instead of 13 the per-rotation fixed work - the source-pair map of the next element (two bit
// reversals and a multiply per thread) and the P c0 gather - weighs three times as much, so neither may sit in front of a load.  The loop stays flat over the
// R J terms, one term deep: iteration (r, j) first issues the loads of the term after it, then multiplies its own.  The map of rotation r + 1 is computed
// right AFTER the loads of rotation r's LAST term have been issued - one whole term before the iteration that needs it to issue (r + 1, 0) - so its ALU chain
// runs under that term's loads and the previous term's multiplies, and the first load of a rotation never waits for a map.  The P c0 term is that last term
// on a data limb: a plain gather with no key pair, so the rotation's shortest load set is the one the map hides under.  The last term re-requests itself.
template <class Arith>
struct QpSumOneP {
    u64 p;
    __device__ __forceinline__ u64 operator()(int, int, const LimbConst& lc) const { return QpSumLane<Arith>::p_operand(p, lc); }
};
struct QpSumTableP {
    const BaseExtArgs* div;   // the division's block: sources = the special limbs, destinations = the data limbs
    __device__ __forceinline__ u64 operator()(int limb, int n_data, const LimbConst&) const { return limb < n_data ? div->Q_mod[limb] : 0; }
};

// digits [n_items][n_dig][L][N], xntt [n_items][2][n_data][N], keys n_rot x [n_dig][2][L][N] (key_stride words apart), out [n_items][2][L][N]
template <class Arith, class POp>
__device__ __forceinline__ void qp_sum_body(u64* __restrict__ out, const u64* __restrict__ digits, const u64* __restrict__ xntt, const u64* __restrict__ keys,
                                            size_t key_stride, const QpSumElts& elts, unsigned n_rot, unsigned n_items, unsigned tiles, POp p_of,
                                            const LimbConst* __restrict__ lcs, int n_limbs, int n_dig, int n_data, int log2n) {
    constexpr int TI = kQpSumTile;
    const int L = n_limbs;
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
    const int J = limb < n_data ? n_dig + 1 : n_dig;   // terms per rotation: the P c0 term is absent on a special limb
    const unsigned total = n_rot * (unsigned)J;
    const U64x2* dig = reinterpret_cast<const U64x2*>(digits + ((size_t)t0 * n_dig * L + limb) * N);   // item i, digit j at + (i n_dig + j) * row
    const U64x2* cin = reinterpret_cast<const U64x2*>(xntt + ((size_t)t0 * 2 * n_data + limb) * N);    // item i's c0 at + i * 2 n_data N words
    const U64x2* evk = reinterpret_cast<const U64x2*>(keys + (size_t)limb * N) + mo;                   // key (r, j, comp) at + r key_stride words + (2 j + comp) * row

    // term (r, j) into (x, e0, e1): the tile's gathered pairs and, for a digit term, the key pairs; ms = the rotation's source pair
    auto request = [&](U64x2 (&x)[TI], U64x2& e0, U64x2& e1, unsigned r, int j, unsigned ms) {
        if (!ok) return;
        if (j < n_dig) {
            const U64x2* kp = evk + ((size_t)r * key_stride / 2 + (size_t)(2 * j) * row);
            e0 = kp[0];
            e1 = kp[row];
#pragma unroll
            for (int i = 0; i < TI; ++i)
                if ((unsigned)i < rows) x[i] = dig[((size_t)i * n_dig + j) * row + ms];
        } else {
#pragma unroll
            for (int i = 0; i < TI; ++i)
                if ((unsigned)i < rows) x[i] = cin[(size_t)i * n_data * N + ms];
        }
    };
    // the map of the rotation after r, or r's own when it is the last (never read then)
    auto map_after = [&](unsigned r) { return QpSumMap::source(elts.v[r + 1 < n_rot ? r + 1 : r], wk.oseg, threadIdx.x, geo); };

    U64x2 x[TI], e0{0, 0}, e1{0, 0};
#pragma unroll
    for (int i = 0; i < TI; ++i) x[i] = U64x2{0, 0};
    unsigned r = 0;
    int j = 0;
    QpPair pm = QpSumMap::source(elts.v[0], wk.oseg, threadIdx.x, geo), pn = pm;   // pm: the current rotation's map; pn: the next one's, from its cut on
    bool sw = pm.swap;
    request(x, e0, e1, 0u, 0, pm.src);
    if (J == 1) pn = map_after(0u);

    // what differs between the arithmetic classes - the accumulators, one term's products, the fold period, the final words - is the lane's (rotate_sum.h)
    typedef QpSumLane<Arith> Lane;
    Lane lane;
    lane.clear();
    const u64 pmod = p_of(limb, n_data, lc);

#pragma unroll 1
    for (unsigned u = 0; u < total; ++u) {
        // the next term: (r, j + 1), or (r + 1, 0) under the map made one term ago; the last term re-requests itself
        unsigned rn = r;
        int jn = j + 1;
        QpPair pq = pm;
        if (jn == J) {
            if (r + 1 < n_rot) {
                rn = r + 1;
                jn = 0;
                pq = pn;
            } else {
                jn = j;
            }
        }
        U64x2 xn[TI], e0n = e0, e1n = e1;
#pragma unroll
        for (int i = 0; i < TI; ++i) xn[i] = x[i];
        request(xn, e0n, e1n, rn, jn, pq.src);
        if (jn == J - 1) pn = map_after(rn);   // the cut: rotation rn's last term is in flight, the next rotation's map runs under it

        lane.begin_term(lc);   // (fold: the period's fold, workgroup-uniform)
        if constexpr (Arith::kFold) {   // the kind of term outside the rows: a key pair is split once for the tile
            if (j < n_dig) {
                const typename Lane::Key k = Lane::split_key(e0.a, e0.b, e1.a, e1.b);
#pragma unroll
                for (int i = 0; i < TI; ++i) {
                    if ((unsigned)i >= rows) continue;
                    lane.digit_term(i, sw ? x[i].b : x[i].a, sw ? x[i].a : x[i].b, k, lc);
                }
            } else {
                const typename Lane::PTerm hp = Lane::split_p(pmod);
#pragma unroll
                for (int i = 0; i < TI; ++i) {
                    if ((unsigned)i >= rows) continue;
                    lane.p_term(i, sw ? x[i].b : x[i].a, sw ? x[i].a : x[i].b, hp, lc);
                }
            }
        } else {                        // nothing to split: the rows outside (fewer registers live across the branch)
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                if ((unsigned)i >= rows) continue;
                const u64 xa = sw ? x[i].b : x[i].a, xb = sw ? x[i].a : x[i].b;
                if (j < n_dig) lane.digit_term(i, xa, xb, Lane::split_key(e0.a, e0.b, e1.a, e1.b), lc);
                else lane.p_term(i, xa, xb, Lane::split_p(pmod), lc);
            }
        }
#pragma unroll
        for (int i = 0; i < TI; ++i) x[i] = xn[i];
        e0 = e0n; e1 = e1n;
        r = rn; j = jn; pm = pq; sw = pq.swap;
    }
    if (!ok) return;
    lane.finish(lc);
    // written once, read by the inverse transform's launch: around the caches the keys and digits live in
#pragma unroll
    for (int i = 0; i < TI; ++i) {
        if ((unsigned)i >= rows) continue;
        U64x2* o0 = reinterpret_cast<U64x2*>(out + (((size_t)(t0 + i) * 2 + 0) * L + limb) * N) + mo;
        st_vec<true>(o0, U64x2{lane.r0[i][0], lane.r0[i][1]});
        st_vec<true>(o0 + row, U64x2{lane.r1[i][0], lane.r1[i][1]});
    }
}

// one special prime, one data limb per digit: n_dig = n_data = L - 1
template <class Arith>
__global__ __launch_bounds__(256) void hoisted_qp_sum_kernel(u64* __restrict__ out, const u64* __restrict__ digits, const u64* __restrict__ xntt,
                                                             const u64* __restrict__ keys, size_t key_stride, QpSumElts elts, unsigned n_rot, unsigned n_items,
                                                             unsigned tiles, u64 p_special, const LimbConst* __restrict__ lcs, int n_limbs, int log2n) {
    qp_sum_body<Arith>(out, digits, xntt, keys, key_stride, elts, n_rot, n_items, tiles, QpSumOneP<Arith>{p_special}, lcs, n_limbs, n_limbs - 1, n_limbs - 1, log2n);
}

// grouped digits: n_dig = beta groups over n_data = L - alpha data limbs; div = the division block of the context's grouped table (tabs + beta)
template <class Arith>
__global__ __launch_bounds__(256) void hoisted_qp_sum_grouped_kernel(u64* __restrict__ out, const u64* __restrict__ digits, const u64* __restrict__ xntt,
                                                                     const u64* __restrict__ keys, size_t key_stride, QpSumElts elts, unsigned n_rot,
                                                                     unsigned n_items, unsigned tiles, const BaseExtArgs* __restrict__ div,
                                                                     const LimbConst* __restrict__ lcs, int n_limbs, int n_dig, int n_data, int log2n) {
    qp_sum_body<Arith>(out, digits, xntt, keys, key_stride, elts, n_rot, n_items, tiles, QpSumTableP{div}, lcs, n_limbs, n_dig, n_data, log2n);
}

}  // namespace dpfhe
