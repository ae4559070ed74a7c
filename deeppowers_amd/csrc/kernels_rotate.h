// kernels_rotate.h - streaming (HBM-bound) kernels of the rotations: Galois automorphisms, the last pass of a rotate-and-add step and the hoisted baby steps over Q P.
// Included by cabi_rotate.hip only.  No reference counterpart.
#pragma once
#include <hip/hip_runtime.h>

#include "launch.h"
#include "modarith.h"
#include "rotate_add.h"
#include "stream_access.h"
#include "workmap.h"

namespace dpfhe {

// N3: Galois automorphism a(X) -> a(X^g), g odd, coefficient domain (a signed permutation; HBM-bound).
// Gather form: out[k] = +in[j] if j = k g^-1 mod 2N < N, else -in[j - N]  (coalesced writes, scattered 8-byte reads).
__global__ __launch_bounds__(256) void galois_kernel(u64* out, const u64* in, const LimbConst* lcs, int n_limbs, int n, unsigned g_inv) {
    const size_t p = blockIdx.x;
    const u64 q = lcs[p % (size_t)n_limbs].q;
    const unsigned mask2n = 2u * (unsigned)n - 1u;
    for (int k = threadIdx.x; k < n; k += 256) {
        const unsigned j = ((unsigned)k * g_inv) & mask2n;
        const u64 v = in[p * n + (j & ((unsigned)n - 1u))];
        out[p * n + k] = (j < (unsigned)n) ? v : neg_mod(v, q);
    }
}

// batched rotations: item i applies its own element (g_inv.v[i]) to input item i (or to the single input item when
// in_item_stride == 0); polys_per_item residue polynomials per item
struct GaloisInvs { unsigned v[kMaxGaloisBatch]; };
// in_mod > 0: output item i reads input item (item0 + i) % in_mod (several rotations of each of in_mod inputs: rotation-major order)
// output items are out_item_stride words apart (polys_per_item * n: back to back)
// LDS_STAGE (N <= 8192: the polynomial fits 64 KiB of dynamic LDS): the source polynomial is read with coalesced 16-byte loads
// into LDS and gathered from there - the odd multiplier g^-1 spreads consecutive k over distinct banks - instead of 8-byte
// global gathers that touch a different cache line per lane (packed GPT-2 layer, 8 tokens per application: 0.278 -> 0.265 ms per token).
template <bool LDS_STAGE>
__global__ __launch_bounds__(256) void galois_multi_kernel(u64* out, const u64* in, size_t in_item_stride, const LimbConst* lcs, int n_limbs, int n,
                                                           int polys_per_item, GaloisInvs g_inv, unsigned in_mod, unsigned item0, size_t out_item_stride) {
    extern __shared__ __attribute__((aligned(16))) u64 stage[];
    const size_t item = blockIdx.x / (unsigned)polys_per_item, p = blockIdx.x % (unsigned)polys_per_item;
    const u64 q = lcs[p % (size_t)n_limbs].q;
    const unsigned mask2n = 2u * (unsigned)n - 1u, gi = g_inv.v[item];
    const size_t in_item = in_mod ? (item0 + item) % in_mod : item;
    const u64* src = in + in_item * in_item_stride + p * n;
    u64* dst = out + item * out_item_stride + p * n;
    if (LDS_STAGE) {
        for (int k = threadIdx.x * 2; k < n; k += 512) *reinterpret_cast<U64x2*>(stage + k) = *reinterpret_cast<const U64x2*>(src + k);
        __syncthreads();
        for (int k = threadIdx.x * 2; k < n; k += 512) {
            const unsigned j0 = ((unsigned)k * gi) & mask2n, j1 = (j0 + gi) & mask2n;
            const u64 v0 = stage[j0 & ((unsigned)n - 1u)], v1 = stage[j1 & ((unsigned)n - 1u)];
            *reinterpret_cast<U64x2*>(dst + k) = U64x2{(j0 < (unsigned)n) ? v0 : neg_mod(v0, q), (j1 < (unsigned)n) ? v1 : neg_mod(v1, q)};
        }
        return;
    }
    for (int k = threadIdx.x; k < n; k += 256) {
        const unsigned j = ((unsigned)k * gi) & mask2n;
        const u64 v = src[j & ((unsigned)n - 1u)];
        dst[k] = (j < (unsigned)n) ? v : neg_mod(v, q);
    }
}

// The last pass of a rotate-and-add step (rotate_add.h): divide the key products of sigma_g(c1) by P, add the step's input and sigma_g(c0), which is gathered
// here and never written.  work: [batch][2][L][N] over Q P, in2 / out: [batch][2][Ld][N].  One workgroup per (item, data limb, slice of the polynomial's
// 512-word chunks - workmap.h RotateAddMap), both components of the slice.  LDS_STAGE (N <= 8192): the c0 polynomial is read once with 16-byte loads into LDS
// and serves the direct addend and the gather (the odd multiplier g^-1 spreads consecutive k over the banks, as in galois_multi_kernel); otherwise the
// gather goes to global memory, 8 bytes per word, from the L2 of the XCD that runs all slices of the polynomial.  Per slice word: the rows of limb i and
// of P of both components of `work`, c1, and one store per component.
template <class Arith, bool LDS_STAGE>
__global__ __launch_bounds__(256) void rotate_add_pass_kernel(u64* __restrict__ out, const u64* __restrict__ work, const u64* __restrict__ in2, const LimbConst* lcs,
                                                              const RescaleConst* rcs, int n_limbs, int n, unsigned slices, size_t n_polys, unsigned g_inv) {
    extern __shared__ __attribute__((aligned(16))) u64 stage[];
    const int Ld = n_limbs - 1;
    const RotateAddWork wk = RotateAddMap::decode(blockIdx.x, slices, n_polys, (unsigned)Ld);
    if (!wk.live) return;
    const int limb = wk.limb;
    const LimbConst lc = lcs[limb];
    const RescaleConst rc = rcs[limb];
    const u64* c0 = in2 + (wk.item * 2 * Ld + limb) * n;
    const u64* c1 = c0 + (size_t)Ld * n;
    const u64* w0 = work + (wk.item * 2 * n_limbs + limb) * n;
    const u64* p0 = work + (wk.item * 2 * n_limbs + Ld) * n;
    const u64 *w1 = w0 + (size_t)n_limbs * n, *p1 = p0 + (size_t)n_limbs * n;
    u64* o0 = out + (wk.item * 2 * Ld + limb) * n;
    u64* o1 = o0 + (size_t)Ld * n;
    if (LDS_STAGE) {
        for (int k = threadIdx.x * 2; k < n; k += 512) *reinterpret_cast<U64x2*>(stage + k) = *reinterpret_cast<const U64x2*>(c0 + k);
        __syncthreads();
    }
    const u64* src = LDS_STAGE ? stage : c0;
    const unsigned mask2n = 2u * (unsigned)n - 1u, maskn = (unsigned)n - 1u;
    const int per = chunks_of(n) / (int)slices;
    for (int ch = (int)wk.slice * per; ch < ((int)wk.slice + 1) * per; ++ch) {
        const int k = ch * 512 + threadIdx.x * 2;
        if (k >= n) break;   // (rings below 512 words: one partial chunk)
        const U64x2 a0 = *reinterpret_cast<const U64x2*>(w0 + k), b0 = *reinterpret_cast<const U64x2*>(p0 + k);
        const U64x2 a1 = *reinterpret_cast<const U64x2*>(w1 + k), b1 = *reinterpret_cast<const U64x2*>(p1 + k);
        const U64x2 d1 = *reinterpret_cast<const U64x2*>(c1 + k);
        const U64x2 d0 = *reinterpret_cast<const U64x2*>(src + k);
        const unsigned j0 = ((unsigned)k * g_inv) & mask2n, j1 = (j0 + g_inv) & mask2n;
        const u64 s0 = src[j0 & maskn], s1 = src[j1 & maskn];
        *reinterpret_cast<U64x2*>(o0 + k) = U64x2{rotate_add_word0<Arith>(a0.a, b0.a, d0.a, s0, j0 > maskn, lc, rc), rotate_add_word0<Arith>(a0.b, b0.b, d0.b, s1, j1 > maskn, lc, rc)};
        *reinterpret_cast<U64x2*>(o1 + k) = U64x2{rotate_add_word1<Arith>(a1.a, b1.a, d1.a, lc, rc), rotate_add_word1<Arith>(a1.b, b1.b, d1.b, lc, rc)};
    }
}

// N3 (round 3): a ciphertext in the NTT domain on the data limbs, lifted to the extended basis as P * ct: word * (P mod q_i) on the
// data limbs, 0 on the special limb (P = 0 mod P).  in: [n_polys][Ld][N] -> out: [n_polys][L][N].  The un-rotated baby step.
template <class Arith>
__global__ __launch_bounds__(256) void lift_qp_kernel(u64* out, const u64* in, const LimbConst* lcs, u64 p_special, int n_limbs, int n, int chunks) {
    const ChunkWork wk = chunk_work(blockIdx.x, chunks, n_limbs);
    const int chunk = wk.chunk, limb = wk.limb;
    const size_t poly = wk.poly;
    const int w0 = chunk * 512 + threadIdx.x * 2;
    if (w0 >= n) return;
    U64x2 r{0, 0};
    if (limb < n_limbs - 1) {
        const LimbConst lc = lcs[limb];
        const u64 pmod = Arith::kFold ? FoldArith::canon(p_special, lc) : ShoupArith::mul_var(p_special, 1, lc);
        const U64x2 v = *reinterpret_cast<const U64x2*>(in + (poly * (n_limbs - 1) + limb) * n + w0);
        r.a = Arith::mul_var(v.a, pmod, lc);
        r.b = Arith::mul_var(v.b, pmod, lc);
    }
    *reinterpret_cast<U64x2*>(out + (poly * n_limbs + limb) * n + w0) = r;
}

// ------------------------------------------------------------------------------------------------
// N3, round 4: the baby-step pass of the double-hoisted packed products as a STREAM (replaces kernels.h hoisted_qp_kernel, whose one
// workgroup per (rotation, limb, token) re-read the digit images once per rotation: 2.3 x its algorithmic bytes in L2 misses).
//   out[(r, t)] = ( sum_j perm_g(digit_{t,j}) (.) key_{r,j,0} + P perm_g(NTT(c0_t)),  sum_j perm_g(digit_{t,j}) (.) key_{r,j,1} )   over all L limbs.
// No transform, so no NTT geometry: a workgroup is 256 threads x PP 16-byte pairs = one SEGMENT of 512 PP words of one (rotation, limb, token).
// Keys and results are read / written in natural (forward-output) order, lane-contiguous; only the digit words are permuted, and sigma_g
// in forward-output order maps every aligned pair ONTO an aligned pair (swapped or not) and every aligned segment onto an aligned segment:
//   pair m -> pair m' = brv((c - 1) / 2),  c = g (2 brv(m) + 1) mod 2N reduced mod N,  words swapped iff that product is >= N
// (brv over log2 N - 1 bits) - one 16-byte gather per pair inside ONE source segment, indices computed once per thread and reused for
// all digits.  What makes the traffic algorithmic is WHERE workgroups run: ids are dealt to the 8 XCDs round-robin, and XCD x gets, one
// block of 16 rotations x n_items tokens at a time, all workgroups of one (limb, SOURCE segment): the block's workgroups are resident
// together (5 per CU), every key segment is fetched from HBM once for its n_items tokens and every digit segment once for its 16 rotations.
// ------------------------------------------------------------------------------------------------
// (kQpPairs, kQpRotGroup, the id layout and the pair map: workmap.h QpMap)
struct QpElts { unsigned v[kMaxGaloisBatch]; };

template <class Arith, int PP>
__global__ __launch_bounds__(256) void hoisted_qp_stream_kernel(u64* __restrict__ out, const u64* __restrict__ digits, const u64* __restrict__ xntt,
                                                                const u64* __restrict__ keys, size_t key_stride, QpElts elts, unsigned n_rot, unsigned n_items,
                                                                u64 p_special, const LimbConst* __restrict__ lcs, int n_limbs, int log2n) {
    const int L = n_limbs, Ld = L - 1;
    const QpGeo geo = QpMap::geo(log2n, PP);
    // id -> (XCD x, block of one (limb, source segment, rotation group), rotation in group, token)
    const QpWork wk = QpMap::decode(blockIdx.x, geo, (unsigned)L, n_rot, n_items);
    if (!wk.live) return;
    const int limb = wk.limb;
    const unsigned rot = wk.rot, token = wk.token;
    const unsigned g = elts.v[rot];
    const LimbConst lc = lcs[limb];
    const size_t N = geo.n;
    unsigned ms[PP], mo[PP];
    bool sw[PP], ok[PP];
#pragma unroll
    for (int c = 0; c < PP; ++c) {
        const QpPair pm = QpMap::pair_map(g, wk.sseg, (unsigned)c * 256u + threadIdx.x, geo);
        mo[c] = pm.out; ms[c] = pm.src; sw[c] = pm.swap; ok[c] = pm.ok;
    }
    const size_t item = (size_t)rot * n_items + token;
    const u64* dig = digits + ((size_t)token * Ld * L + limb) * N;      // digit j at + j L N
    const u64* evk = keys + (size_t)rot * key_stride + (size_t)limb * N; // key (j, comp) at + (j 2 + comp) L N
    auto gather = [&](U64x2 (&x)[PP], const u64* tile) {
#pragma unroll
        for (int c = 0; c < PP; ++c)
            if (ok[c]) x[c] = reinterpret_cast<const U64x2*>(tile)[ms[c]];
    };
    auto unswap = [&](U64x2 (&x)[PP]) {
#pragma unroll
        for (int c = 0; c < PP; ++c) { const u64 a = x[c].a, b = x[c].b; x[c].a = sw[c] ? b : a; x[c].b = sw[c] ? a : b; }
    };
    auto stream = [&](U64x2 (&e)[PP], const u64* tile) {
#pragma unroll
        for (int c = 0; c < PP; ++c)
            if (ok[c]) e[c] = reinterpret_cast<const U64x2*>(tile)[mo[c]];
    };
    u64* o0 = out + ((item * 2 + 0) * L + limb) * N;
    u64* o1 = out + ((item * 2 + 1) * L + limb) * N;
    U64x2 x[PP], e0[PP], e1[PP];
#pragma unroll
    for (int c = 0; c < PP; ++c) { x[c] = U64x2{0, 0}; e0[c] = U64x2{0, 0}; e1[c] = U64x2{0, 0}; }
    if constexpr (Arith::kFold) {
        // Lazy inner products on 30-bit halves (modarith.h Dot30: FOUR multiply-adds per term, the split of a digit word shared by both key
        // components, one fold per kDot30Period terms) instead of one mul60 (15 instructions) per product: the pass is VALU-bound once its
        // traffic is algorithmic.  All operands are canonical residues (< 2^60), which is what split30 needs.
        typedef FoldArith::Dot30 Dot;
        typedef FoldArith::Half30 Half;
        Dot s0[PP][2], s1[PP][2];
        u64 r0[PP][2], r1[PP][2];
#pragma unroll
        for (int c = 0; c < PP; ++c)
#pragma unroll
            for (int h = 0; h < 2; ++h) { s0[c][h] = Dot{0, 0, 0}; s1[c][h] = Dot{0, 0, 0}; r0[c][h] = 0; r1[c][h] = 0; }
        int terms = 0;
        auto fold_all = [&]() {
#pragma unroll
            for (int c = 0; c < PP; ++c)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    r0[c][h] = FoldArith::dot30_fold(s0[c][h], r0[c][h], lc); s0[c][h] = Dot{0, 0, 0};
                    r1[c][h] = FoldArith::dot30_fold(s1[c][h], r1[c][h], lc); s1[c][h] = Dot{0, 0, 0};
                }
            terms = 0;
        };
        if (limb < Ld) {   // component 0 starts with P perm_g(NTT(c0)) on the data limbs (P = 0 on the special limb)
            U64x2 c0[PP];
#pragma unroll
            for (int c = 0; c < PP; ++c) c0[c] = U64x2{0, 0};
            gather(c0, xntt + ((size_t)token * 2 * Ld + limb) * N);
            gather(x, dig);
            stream(e0, evk);
            stream(e1, evk + (size_t)L * N);
            unswap(c0);
            const Half hp = FoldArith::split30(FoldArith::canon(p_special, lc));
#pragma unroll
            for (int c = 0; c < PP; ++c) {
                FoldArith::dot30_mac(s0[c][0], FoldArith::split30(c0[c].a), hp);
                FoldArith::dot30_mac(s0[c][1], FoldArith::split30(c0[c].b), hp);
            }
            terms = 1;
        } else {
            gather(x, dig);
            stream(e0, evk);
            stream(e1, evk + (size_t)L * N);
        }
#pragma unroll 1
        for (int j = 0; j < Ld; ++j) {
            U64x2 xn[PP], e0n[PP], e1n[PP];
            const int jn = j + 1 < Ld ? j + 1 : j;   // the last iteration re-requests its own segments (cache hits) instead of branching
#pragma unroll
            for (int c = 0; c < PP; ++c) { xn[c] = x[c]; e0n[c] = e0[c]; e1n[c] = e1[c]; }
            gather(xn, dig + (size_t)jn * L * N);
            stream(e0n, evk + (size_t)(jn * 2) * L * N);
            stream(e1n, evk + (size_t)(jn * 2 + 1) * L * N);
            unswap(x);
            if (terms == FoldArith::kDot30Period) fold_all();   // workgroup-uniform
            ++terms;
#pragma unroll
            for (int c = 0; c < PP; ++c) {
                const Half xa = FoldArith::split30(x[c].a), xb = FoldArith::split30(x[c].b);
                FoldArith::dot30_mac(s0[c][0], xa, FoldArith::split30(e0[c].a));
                FoldArith::dot30_mac(s0[c][1], xb, FoldArith::split30(e0[c].b));
                FoldArith::dot30_mac(s1[c][0], xa, FoldArith::split30(e1[c].a));
                FoldArith::dot30_mac(s1[c][1], xb, FoldArith::split30(e1[c].b));
            }
#pragma unroll
            for (int c = 0; c < PP; ++c) { x[c] = xn[c]; e0[c] = e0n[c]; e1[c] = e1n[c]; }
        }
        fold_all();
#pragma unroll
        for (int c = 0; c < PP; ++c) {
            if (!ok[c]) continue;
            // written once, read by the next launch: around the caches the keys and digits live in
            st_vec<true>(reinterpret_cast<U64x2*>(o0) + mo[c], U64x2{FoldArith::canon_small(r0[c][0], lc), FoldArith::canon_small(r0[c][1], lc)});
            st_vec<true>(reinterpret_cast<U64x2*>(o1) + mo[c], U64x2{FoldArith::canon_small(r1[c][0], lc), FoldArith::canon_small(r1[c][1], lc)});
        }
    } else {
        U64x2 acc0[PP], acc1[PP];
#pragma unroll
        for (int c = 0; c < PP; ++c) { acc0[c] = U64x2{0, 0}; acc1[c] = U64x2{0, 0}; }
        auto accw = [&](u64 acc, u64 a, u64 b) -> u64 { return add_mod(acc, ShoupArith::mul_var(a, b, lc), lc.q); };
        if (limb < Ld) {
            U64x2 c0[PP];
#pragma unroll
            for (int c = 0; c < PP; ++c) c0[c] = U64x2{0, 0};
            gather(c0, xntt + ((size_t)token * 2 * Ld + limb) * N);
            unswap(c0);
            const u64 pmod = ShoupArith::mul_var(p_special, 1, lc);
#pragma unroll
            for (int c = 0; c < PP; ++c) { acc0[c].a = ShoupArith::mul_var(c0[c].a, pmod, lc); acc0[c].b = ShoupArith::mul_var(c0[c].b, pmod, lc); }
        }
#pragma unroll 1
        for (int j = 0; j < Ld; ++j) {
            gather(x, dig + (size_t)j * L * N);
            stream(e0, evk + (size_t)(j * 2) * L * N);
            stream(e1, evk + (size_t)(j * 2 + 1) * L * N);
            unswap(x);
#pragma unroll
            for (int c = 0; c < PP; ++c) {
                acc0[c].a = accw(acc0[c].a, x[c].a, e0[c].a); acc0[c].b = accw(acc0[c].b, x[c].b, e0[c].b);
                acc1[c].a = accw(acc1[c].a, x[c].a, e1[c].a); acc1[c].b = accw(acc1[c].b, x[c].b, e1[c].b);
            }
        }
#pragma unroll
        for (int c = 0; c < PP; ++c) {
            if (!ok[c]) continue;
            st_vec<true>(reinterpret_cast<U64x2*>(o0) + mo[c], acc0[c]);
            st_vec<true>(reinterpret_cast<U64x2*>(o1) + mo[c], acc1[c]);
        }
    }
}
// The same pass with EVERY operand segment of the workgroup requested up front (round 4, after the workgroup timeline of the multiply put the
// cost of a first HBM touch at ~3.6 us): the loop form above keeps one digit's segments in flight while it multiplies the previous one, i.e. it
// pays that latency once per digit; here a thread owns ONE pair of words, the digit count LD is a template parameter, and the 3 LD + 1 loads of
// the thread are all issued before the first product (straight-line code: hipcc counts vmcnt exactly).  FoldArith, LD <= 6.
template <int LD>
__global__ __launch_bounds__(256) void hoisted_qp_upfront_kernel(u64* __restrict__ out, const u64* __restrict__ digits, const u64* __restrict__ xntt,
                                                                 const u64* __restrict__ keys, size_t key_stride, QpElts elts, unsigned n_rot, unsigned n_items,
                                                                 u64 p_special, const LimbConst* __restrict__ lcs, int log2n) {
    constexpr int L = LD + 1;
    const QpGeo geo = QpMap::geo(log2n, 1);
    const QpWork wk = QpMap::decode(blockIdx.x, geo, (unsigned)L, n_rot, n_items);
    if (!wk.live) return;
    const int limb = wk.limb;
    const unsigned rot = wk.rot, token = wk.token;
    const unsigned g = elts.v[rot];
    const LimbConst lc = lcs[limb];
    const size_t N = geo.n;
    const QpPair pm = QpMap::pair_map(g, wk.sseg, threadIdx.x, geo);
    if (!pm.ok) return;
    const unsigned mo = pm.out, ms = pm.src;
    const bool sw = pm.swap;
    const size_t item = (size_t)rot * n_items + token;
    const U64x2* dig = reinterpret_cast<const U64x2*>(digits + ((size_t)token * LD * L + limb) * N) + ms;      // digit j at + j L N words
    const U64x2* evk = reinterpret_cast<const U64x2*>(keys + (size_t)rot * key_stride + (size_t)limb * N) + mo;  // key (j, comp) at + (j 2 + comp) L N words
    const size_t tile = (size_t)L * N / 2;   // in 16-byte units
    U64x2 x[LD], e0[LD], e1[LD], c0{0, 0};
    const bool data_limb = limb < LD;
    if (data_limb) c0 = (reinterpret_cast<const U64x2*>(xntt + ((size_t)token * 2 * LD + limb) * N))[ms];
#pragma unroll
    for (int j = 0; j < LD; ++j) {
        x[j] = dig[(size_t)j * tile];
        e0[j] = evk[(size_t)(2 * j) * tile];
        e1[j] = evk[(size_t)(2 * j + 1) * tile];
    }
    typedef FoldArith::Dot30 Dot;
    typedef FoldArith::Half30 Half;
    static_assert(LD + 1 <= FoldArith::kDot30Period, "one fold per accumulator");
    Dot s0[2] = {Dot{0, 0, 0}, Dot{0, 0, 0}}, s1[2] = {Dot{0, 0, 0}, Dot{0, 0, 0}};
    if (data_limb) {   // P perm_g(NTT(c0)) on the data limbs
        const Half hp = FoldArith::split30(FoldArith::canon(p_special, lc));
        FoldArith::dot30_mac(s0[0], FoldArith::split30(sw ? c0.b : c0.a), hp);
        FoldArith::dot30_mac(s0[1], FoldArith::split30(sw ? c0.a : c0.b), hp);
    }
#pragma unroll
    for (int j = 0; j < LD; ++j) {
        const Half xa = FoldArith::split30(sw ? x[j].b : x[j].a), xb = FoldArith::split30(sw ? x[j].a : x[j].b);
        FoldArith::dot30_mac(s0[0], xa, FoldArith::split30(e0[j].a));
        FoldArith::dot30_mac(s0[1], xb, FoldArith::split30(e0[j].b));
        FoldArith::dot30_mac(s1[0], xa, FoldArith::split30(e1[j].a));
        FoldArith::dot30_mac(s1[1], xb, FoldArith::split30(e1[j].b));
    }
    U64x2 r0, r1;
    r0.a = FoldArith::canon_small(FoldArith::dot30_fold(s0[0], 0, lc), lc); r0.b = FoldArith::canon_small(FoldArith::dot30_fold(s0[1], 0, lc), lc);
    r1.a = FoldArith::canon_small(FoldArith::dot30_fold(s1[0], 0, lc), lc); r1.b = FoldArith::canon_small(FoldArith::dot30_fold(s1[1], 0, lc), lc);
    st_vec<true>(reinterpret_cast<U64x2*>(out + ((item * 2 + 0) * L + limb) * N) + mo, r0);
    st_vec<true>(reinterpret_cast<U64x2*>(out + ((item * 2 + 1) * L + limb) * N) + mo, r1);
}

}  // namespace dpfhe
