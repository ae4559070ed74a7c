// rotate_matvec.h - the baby steps of a packed layer WEIGHTED by its pre-rotated diagonals in one pass, output-stationary (include/dpfhe.h
// dpfhe_rotate_matvec_hoisted_qp): the lane arithmetic (host + device) and hoisted_qp_matvec_kernel.  Included by cabi_rotate_matvec.hip only.
// No reference counterpart.
//
// Per row i of W, item t and limb l of the extended basis, NTT domain, forward-output order, canonical - the words of dpfhe_rotate_hoisted_qp followed by
// dpfhe_matvec_plain_multi, whose (1 + R) Q P blocks per item are never written:
//   y_{i,t} = W[i][0] (.) (P c0_t, P c1_t)  +  sum_{r<R} W[i][1 + r] (.) B_{r,t},
//   B_{r,t}.c0 = sum_{j<Ld} perm_{g_r}(digit_{t,j}) (.) key_{r,j,0} + P perm_{g_r}(NTT(c0_t)),   B_{r,t}.c1 = sum_{j<Ld} perm_{g_r}(digit_{t,j}) (.) key_{r,j,1}
// (the P terms are absent on the special limb, where block 0 is zero).
//
// The split (workmap.h RotMatvecMap).  A workgroup owns ONE OUTPUT segment (256 threads x one 16-byte pair) of one limb of ONE item, BOTH components, for a
// tile of kRotMatvecRows = 6 rows of W.  Per rotation it forms the four words of B_r (2 components x the pair's 2 halves) ONCE - gathered through
// QpSumMap::source like hoisted_qp_sum_kernel's - and multiplies them into the tile's 6 x 4 row accumulators, which stay in registers until the one store.
// Why this shape, per thread and rotation on a data limb, in 32 x 32 -> 64 multiply-adds (fold limbs; Ld = 7 in brackets):
//   key products   4 words x (Ld + 1) terms x 4 = 16 (Ld + 1)   [128]       weights   4 words x 6 rows x 4 = 96
//   loads          Ld digit + 2 Ld key + 1 input + 6 W pairs of 16 bytes    [28: 8 multiply-adds per load, all but W from L2]
// so per OUTPUT word 4 (1 + R) multiply-adds of weighting + 4 R (Ld + 1) / 6 of key products: the key product is recomputed once per ROW TILE, and
// `rows` above 6 cost rows / 6 recomputations inside the one launch (unfused it is formed once and costs a block written and re-read per rotation).
// The accumulators of one key product are shared by as many weights as there are rows in the tile, whatever else the workgroup holds, so registers go to
// rows first: one item (no idle accumulators at one token; the items of a row tile are neighbours on the XCD and share W and keys in L2), both components
// (one digit load and split serves both), 6 rows.  Accumulators are LAZY Dot30 columns (6 registers a word): 6 x 4 x 6 = 144 for the rows + 4 x 6 = 24 for
// the key product; folded words (2 registers) would take a dot30_fold per term, 18 instructions against 4.  Build log, fold: 238 VGPRs, no AGPR, no scratch, no LDS, two
// waves per SIMD (generic: 147, three); a tile of 8 rows takes 256 VGPRs + 40 AGPRs at ONE wave per SIMD, a tile of 4 (182) doubles the recomputation for no third wave.
// Traffic per item and limb, in rows of N words: read  ceil(rows / 6) R (Ld + 1) gathered digit / input rows + 2 (block 0), ceil(rows / 6) 2 R Ld key rows and
// rows (1 + R) rows of W (the latter two once per XCD from HBM for all items); written 2 rows per row of W.  Unfused: + 2 (1 + R) rows written and
// 2 (1 + R) ceil(rows / 4) re-read.  Registers, LDS and the measured standing: MEASUREMENTS.md, "Baby steps fused with their diagonal products".
//
// Lazy bounds (fold limbs), in units of 2^60 as in rotate_sum.h: a column set takes at most kDot30Period = 8 products between folds (s1 < 16 = 2^64).  A fold
// in the middle of a sum re-seeds the set with the folded word in s0 (< 1 + 2^-32) and zero s1, s2: s0 < 1.01 + 8 before the next fold, inside dot30_mac's
// s0 < 15 before every product and 2^64 after the eighth.  The key product counts its P c0 term like any other (Ld = 8: nine terms, one fold after the
// eighth); B_r is canonicalised (canon_small) before it is split for the weights; the row accumulators count block 0 as one term and fold every eighth block.
#pragma once
#include <hip/hip_runtime.h>

#include "launch.h"
#include "modarith.h"
#include "stream_access.h"
#include "workmap.h"

namespace dpfhe {

// ---- the lane: one 16-byte pair (halves h = 0, 1) of both components, a tile of rows ----------------------------------------------------------
// any policy with a canonical mul_var: canonical words throughout, a term is mul_var + add_mod (launched with ShoupArith on every context that is not all-fold)
template <class Arith>
struct RotMatvecLane {
    static constexpr int RT = kRotMatvecRows;
    struct Key { u64 k0a, k0b, k1a, k1b; };
    typedef u64 PTerm;
    u64 y[RT][2][2];   // [row][component][half]
    u64 b[2][2];       // the current block's words

    DPF_HD void clear() {
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) y[i][c >> 1][c & 1] = 0;
    }
    static DPF_HD u64 p_operand(u64 p_special, const LimbConst& c) { return ShoupArith::mul_var(p_special, 1, c); }
    static DPF_HD Key split_key(u64 e0a, u64 e0b, u64 e1a, u64 e1b) { return Key{e0a, e0b, e1a, e1b}; }
    static DPF_HD PTerm split_p(u64 pmod) { return pmod; }
    static DPF_HD u64 accw(u64 acc, u64 a, u64 w, const LimbConst& c) { return add_mod(acc, Arith::mul_var(a, w, c), c.q); }
    DPF_HD void begin_block() { b[0][0] = b[0][1] = b[1][0] = b[1][1] = 0; }
    DPF_HD void begin_key_term(const LimbConst&) {}
    DPF_HD void digit_term(u64 xa, u64 xb, const Key& k, const LimbConst& c) {
        b[0][0] = accw(b[0][0], xa, k.k0a, c); b[0][1] = accw(b[0][1], xb, k.k0b, c);
        b[1][0] = accw(b[1][0], xa, k.k1a, c); b[1][1] = accw(b[1][1], xb, k.k1b, c);
    }
    DPF_HD void p_term(int comp, u64 xa, u64 xb, const PTerm& p, const LimbConst& c) {
        b[comp][0] = accw(b[comp][0], xa, p, c); b[comp][1] = accw(b[comp][1], xb, p, c);
    }
    DPF_HD void finish_block(const LimbConst&) {}
    DPF_HD void begin_weight(const LimbConst&) {}
    DPF_HD void weight(int i, u64 wa, u64 wb, const LimbConst& c) {
        y[i][0][0] = accw(y[i][0][0], b[0][0], wa, c); y[i][0][1] = accw(y[i][0][1], b[0][1], wb, c);
        y[i][1][0] = accw(y[i][1][0], b[1][0], wa, c); y[i][1][1] = accw(y[i][1][1], b[1][1], wb, c);
    }
    DPF_HD u64 word(int i, int comp, int h, const LimbConst&) const { return y[i][comp][h]; }
};

// fold limbs: lazy Dot30 columns for the key product of the block and for every row (the header comment states the bounds)
template <>
struct RotMatvecLane<FoldArith> {
    static constexpr int RT = kRotMatvecRows;
    typedef FoldArith::Half30 Half30;
    typedef FoldArith::Dot30 Dot30;
    struct Key { Half30 k0a, k0b, k1a, k1b; };
    typedef Half30 PTerm;
    Dot30 y[RT][2][2];
    Dot30 k[2][2];
    Half30 b[2][2];        // the block's canonical words, split for the weights
    int yterms, kterms;    // products gone into the columns since their last fold (workgroup-uniform)

    static DPF_HD void refold(Dot30& s, const LimbConst& c) { s = Dot30{FoldArith::dot30_fold(s, 0, c), 0, 0}; }
    DPF_HD void clear() {
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) y[i][c >> 1][c & 1] = Dot30{0, 0, 0};
        yterms = 0;
    }
    static DPF_HD u64 p_operand(u64 p_special, const LimbConst& c) { return FoldArith::canon(p_special, c); }
    static DPF_HD Key split_key(u64 e0a, u64 e0b, u64 e1a, u64 e1b) {
        return Key{FoldArith::split30(e0a), FoldArith::split30(e0b), FoldArith::split30(e1a), FoldArith::split30(e1b)};
    }
    static DPF_HD PTerm split_p(u64 pmod) { return FoldArith::split30(pmod); }
    DPF_HD void begin_block() {
#pragma unroll
        for (int c = 0; c < 4; ++c) k[c >> 1][c & 1] = Dot30{0, 0, 0};
        kterms = 0;
    }
    DPF_HD void begin_key_term(const LimbConst& c) {
        if (kterms == FoldArith::kDot30Period) {
#pragma unroll
            for (int e = 0; e < 4; ++e) refold(k[e >> 1][e & 1], c);
            kterms = 0;
        }
        ++kterms;
        DPFHE_EMU_ASSERT(kterms >= 1 && kterms <= FoldArith::kDot30Period);
    }
    // all operands are canonical residues (< 2^60), which is what split30 needs
    DPF_HD void digit_term(u64 xa, u64 xb, const Key& e, const LimbConst&) {
        const Half30 ha = FoldArith::split30(xa), hb = FoldArith::split30(xb);
        FoldArith::dot30_mac(k[0][0], ha, e.k0a);
        FoldArith::dot30_mac(k[0][1], hb, e.k0b);
        FoldArith::dot30_mac(k[1][0], ha, e.k1a);
        FoldArith::dot30_mac(k[1][1], hb, e.k1b);
    }
    DPF_HD void p_term(int comp, u64 xa, u64 xb, const PTerm& p, const LimbConst&) {
        FoldArith::dot30_mac(k[comp][0], FoldArith::split30(xa), p);
        FoldArith::dot30_mac(k[comp][1], FoldArith::split30(xb), p);
    }
    DPF_HD void finish_block(const LimbConst& c) {
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e >> 1][e & 1] = FoldArith::split30(FoldArith::canon_small(FoldArith::dot30_fold(k[e >> 1][e & 1], 0, c), c));
    }
    DPF_HD void begin_weight(const LimbConst& c) {
        if (yterms == FoldArith::kDot30Period) {
#pragma unroll
            for (int i = 0; i < RT; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) refold(y[i][e >> 1][e & 1], c);
            yterms = 0;
        }
        ++yterms;
        DPFHE_EMU_ASSERT(yterms >= 1 && yterms <= FoldArith::kDot30Period);
    }
    DPF_HD void weight(int i, u64 wa, u64 wb, const LimbConst&) {
        const Half30 ha = FoldArith::split30(wa), hb = FoldArith::split30(wb);
        FoldArith::dot30_mac(y[i][0][0], b[0][0], ha);
        FoldArith::dot30_mac(y[i][0][1], b[0][1], hb);
        FoldArith::dot30_mac(y[i][1][0], b[1][0], ha);
        FoldArith::dot30_mac(y[i][1][1], b[1][1], hb);
    }
    DPF_HD u64 word(int i, int comp, int h, const LimbConst& c) const { return FoldArith::canon_small(FoldArith::dot30_fold(y[i][comp][h], 0, c), c); }
};

// ---- the kernel: the loads, the map, the prefetch and the stores ---------------------------------------------------------------------------------
struct RotMatvecElts { unsigned v[kMaxGaloisBatch]; };

template <class Arith>
__global__ __launch_bounds__(256) void hoisted_qp_matvec_kernel(u64* __restrict__ out, const u64* __restrict__ W, const u64* __restrict__ digits,
                                                                const u64* __restrict__ xntt, const u64* __restrict__ keys, size_t key_stride, RotMatvecElts elts,
                                                                unsigned n_rot, unsigned n_items, unsigned n_rows, unsigned row_tiles, u64 p_special,
                                                                const LimbConst* __restrict__ lcs, int n_limbs, int log2n) {
    constexpr int RT = kRotMatvecRows;
    const int L = n_limbs, Ld = L - 1;
    const QpGeo geo = RotMatvecMap::geo(log2n);
    const RotMatvecWork wk = RotMatvecMap::decode(blockIdx.x, geo, (unsigned)L, n_items, row_tiles);
    if (!wk.live) return;
    const int limb = wk.limb;
    const LimbConst lc = lcs[limb];
    const size_t N = geo.n, row = (size_t)L * N / 2;   // a digit's, a key component's or a W polynomial's L rows, in 16-byte units
    const unsigned t = wk.item, r0 = wk.row_tile * (unsigned)RT, rows = n_rows - r0 < (unsigned)RT ? n_rows - r0 : (unsigned)RT;   // workgroup-uniform
    const size_t cols = (size_t)n_rot + 1;
    const QpPair po = QpSumMap::source(1u, wk.oseg, threadIdx.x, geo);   // (the output side alone: the identity's source is the pair itself)
    const bool ok = po.ok;
    const unsigned mo = po.out;
    const bool data = limb < Ld;
    const int J = data ? Ld + 1 : Ld;   // terms per rotation: the P c0 term is absent on the special limb
    const unsigned total = n_rot * (unsigned)J;
    const U64x2* dig = reinterpret_cast<const U64x2*>(digits + ((size_t)t * Ld * L + limb) * N);   // digit j at + j * row
    const U64x2* cin = reinterpret_cast<const U64x2*>(xntt + ((size_t)t * 2 * Ld + limb) * N);     // c0 (data limbs only); c1 at + Ld N / 2
    const U64x2* evk = reinterpret_cast<const U64x2*>(keys + (size_t)limb * N) + mo;                // key (r, j, comp) at + r key_stride words + (2 j + comp) * row
    const U64x2* wp = reinterpret_cast<const U64x2*>(W + ((size_t)r0 * cols * L + limb) * N) + mo;  // row i, column c at + (i cols + c) * row

    typedef RotMatvecLane<Arith> Lane;
    Lane lane;
    lane.clear();
    const typename Lane::PTerm hp = Lane::split_p(Lane::p_operand(p_special, lc));

    U64x2 w[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) w[i] = U64x2{0, 0};
    auto load_w = [&](unsigned col) {
        if (!ok) return;
#pragma unroll
        for (int i = 0; i < RT; ++i)
            if ((unsigned)i < rows) w[i] = wp[((size_t)i * cols + col) * row];
    };
    auto weights = [&]() {
        lane.begin_weight(lc);   // (fold: the period's fold, workgroup-uniform)
#pragma unroll
        for (int i = 0; i < RT; ++i)
            if ((unsigned)i < rows) lane.weight(i, w[i].a, w[i].b, lc);
    };

    // block 0 = (P c0, P c1) under column 0: zero on the special limb
    if (data) {
        U64x2 c0{0, 0}, c1{0, 0};
        load_w(0u);
        if (ok) {
            c0 = cin[mo];
            c1 = cin[(size_t)Ld * N / 2 + mo];
        }
        lane.begin_block();
        lane.begin_key_term(lc);
        lane.p_term(0, c0.a, c0.b, hp, lc);
        lane.p_term(1, c1.a, c1.b, hp, lc);
        lane.finish_block(lc);
        weights();
    }

    // term (r, j) into (x, e0, e1): the gathered pair and, for a digit term, the key pairs; ms = the rotation's source pair
    auto request = [&](U64x2& x, U64x2& e0, U64x2& e1, unsigned r, int j, unsigned ms) {
        if (!ok) return;
        if (j < Ld) {
            const U64x2* kp = evk + ((size_t)r * key_stride / 2 + (size_t)(2 * j) * row);
            e0 = kp[0];
            e1 = kp[row];
            x = dig[(size_t)j * row + ms];
        } else {
            x = cin[ms];
        }
    };

    U64x2 x{0, 0}, e0{0, 0}, e1{0, 0};
    unsigned r = 0;
    int j = 0;
    QpPair pm = QpSumMap::source(elts.v[0], wk.oseg, threadIdx.x, geo);
    bool sw = pm.swap;
    request(x, e0, e1, 0u, 0, pm.src);

#pragma unroll 1
    for (unsigned u = 0; u < total; ++u) {
        // the next term: (r, j + 1), or (r + 1, 0) with that rotation's map; the last term re-requests itself (cache hits instead of a branch)
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
        U64x2 xn = x, e0n = e0, e1n = e1;
        request(xn, e0n, e1n, rn, jn, pn.src);
        if (j == 0) {   // a rotation begins: its column of W is requested a whole key product ahead of its use
            lane.begin_block();
            load_w(r + 1u);
        }
        lane.begin_key_term(lc);
        const u64 xa = sw ? x.b : x.a, xb = sw ? x.a : x.b;
        if (j < Ld) lane.digit_term(xa, xb, Lane::split_key(e0.a, e0.b, e1.a, e1.b), lc);
        else lane.p_term(0, xa, xb, hp, lc);
        if (j == J - 1) {   // the rotation's block is complete: into every row of the tile
            lane.finish_block(lc);
            weights();
        }
        x = xn; e0 = e0n; e1 = e1n;
        r = rn; j = jn; pm = pn; sw = pn.swap;
    }
    if (!ok) return;
    // written once, read by the inverse transform's launch: around the caches the keys, digits and W live in
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        if ((unsigned)i >= rows) continue;
        U64x2* o = reinterpret_cast<U64x2*>(out + ((((size_t)(r0 + i) * n_items + t) * 2) * L + limb) * N) + mo;
        st_vec<true>(o, U64x2{lane.word(i, 0, 0, lc), lane.word(i, 0, 1, lc)});
        st_vec<true>(o + row, U64x2{lane.word(i, 1, 0, lc), lane.word(i, 1, 1, lc)});
    }
}

}  // namespace dpfhe
