// kernels_keyswitch.h - streaming (HBM-bound) kernels of key switching: the rescales (every one of them is first of all key switching's division
// by P), digit lifting, and - above N = 8192, where the fused relin_kernel of kernels.h stops - the key inner product and add-back that
// cabi_keyswitch.hip composes with the batched transforms (key_switch_composed, key_products_composed; results equal the fused kernels':
// tests/test_gpu_parity.py).  One workgroup per 512-word chunk of one residue polynomial, 16 bytes per lane, all words canonical in and out.
// Included by cabi_keyswitch.hip only.  No reference counterpart.
#pragma once
#include <hip/hip_runtime.h>

#include "fused_rescale.h"
#include "modarith.h"
#include "workmap.h"

namespace dpfhe {

// (the streaming kernels below take their work in 512-word chunks of a residue polynomial: workmap.h chunks_of, chunk_work)

// N1 (second half): rescale / modulus switch to the next level, coefficient domain.
//   out_i = ((in_i + h) - ((in_last + h) mod q_last)) * q_last^-1   (mod q_i),  h = floor(q_last / 2),  i < L-1
// i.e. round(x / q_last) of the CRT-composed value, limb by limb (no big integers): fused_rescale.h rescale_word.  HBM-bound.
// (RescaleConst: devtables.h)

// `addend` (optional) is the last step of hybrid key switching: polynomial p = 2*b + comp of the rescaled pair gets
// component comp of ciphertext b of `addend` ([batch][add_in_comps][L-1][N]) added when bit comp of add_mask is set.
template <class Arith>
__global__ __launch_bounds__(256) void rescale_kernel(u64* out, const u64* in, const u64* addend, int add_in_comps, int add_mask,
                                                      const LimbConst* lcs, const RescaleConst* rcs, int n_limbs, int n, int chunks) {
    const int Lo = n_limbs - 1;
    const ChunkWork wk = chunk_work(blockIdx.x, chunks, Lo);
    const int chunk = wk.chunk, limb = wk.limb;
    const size_t poly = wk.poly;
    const int w0 = chunk * 512 + threadIdx.x * 2;
    if (w0 >= n) return;
    const LimbConst lc = lcs[limb];
    const RescaleConst rc = rcs[limb];
    const U64x2 x = *reinterpret_cast<const U64x2*>(in + (poly * n_limbs + limb) * n + w0);
    const U64x2 last = *reinterpret_cast<const U64x2*>(in + (poly * n_limbs + Lo) * n + w0);
    U64x2 r{rescale_word<Arith>(x.a, last.a, lc, rc), rescale_word<Arith>(x.b, last.b, lc, rc)};
    if (addend && ((add_mask >> (poly & 1)) & 1)) {
        const size_t ap = (poly >> 1) * (size_t)add_in_comps + (poly & 1);
        const U64x2 ad = *reinterpret_cast<const U64x2*>(addend + (ap * Lo + limb) * n + w0);
        r.a = add_mod(r.a, ad.a, lc.q);
        r.b = add_mod(r.b, ad.b, lc.q);
    }
    *reinterpret_cast<U64x2*>(out + (poly * Lo + limb) * n + w0) = r;
}

// N3 (round 3, deferred divide-by-P): the last step of a baby-step / giant-step sum whose key-switched terms were summed over Q P.
//   out[b][comp][i] = round(in[b][comp] / P)_i  +  sum_{a < n_add} addends[a][b][0][i]   (comp 0)
//                                               +  addends[0][b][1][i]                    (comp 1)
// in: [batch][2][L][N] (coefficient domain, Q P), addends: [n_add][batch][2][Ld][N] (the rotated inner sums: item 0 is the
// un-rotated one and keeps both components, of the others only c0 survives - their c1 went through the key switch), out:
// [batch][2][Ld][N].  One pass; the rounding is orc_rescale's.
template <class Arith>
__global__ __launch_bounds__(256) void rescale_bsgs_kernel(u64* out, const u64* in, const u64* addends, size_t n_add, size_t batch, const LimbConst* lcs,
                                                           const RescaleConst* rcs, int n_limbs, int n, int chunks) {
    const int Lo = n_limbs - 1;
    const ChunkWork wk = chunk_work(blockIdx.x, chunks, Lo);
    const int chunk = wk.chunk, limb = wk.limb;
    const size_t poly = wk.poly;   // = b * 2 + comp
    const int w0 = chunk * 512 + threadIdx.x * 2;
    if (w0 >= n) return;
    const LimbConst lc = lcs[limb];
    const RescaleConst rc = rcs[limb];
    const U64x2 x = *reinterpret_cast<const U64x2*>(in + (poly * n_limbs + limb) * n + w0);
    const U64x2 last = *reinterpret_cast<const U64x2*>(in + (poly * n_limbs + Lo) * n + w0);
    U64x2 r{rescale_word<Arith>(x.a, last.a, lc, rc), rescale_word<Arith>(x.b, last.b, lc, rc)};
    const size_t terms = (poly & 1) ? (n_add ? 1 : 0) : n_add;
    const u64* ap = addends + (poly * Lo + limb) * n + w0;
    const size_t astride = batch * 2 * Lo * (size_t)n;
    size_t a = 0;
    for (; a + 4 <= terms; a += 4) {
        U64x2 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const U64x2*>(ap + (a + u) * astride);
#pragma unroll
        for (int u = 0; u < 4; ++u) { r.a = add_mod(r.a, v[u].a, lc.q); r.b = add_mod(r.b, v[u].b, lc.q); }
    }
    for (; a < terms; ++a) {
        const U64x2 v = *reinterpret_cast<const U64x2*>(ap + a * astride);
        r.a = add_mod(r.a, v.a, lc.q); r.b = add_mod(r.b, v.b, lc.q);
    }
    *reinterpret_cast<U64x2*>(out + (poly * Lo + limb) * n + w0) = r;
}

// The last pass of a relinearised product that is rescaled at once (fused_rescale.h (a)): divide the key-switched sums by P, add (c0, c1), divide by the
// last data prime.  work: [batch][2][L][N] over Q P, in3: [batch][3][Ld][N] (components 0 and 1 are read), out: [batch][2][Ld-1][N].  Per (polynomial,
// kept limb, chunk): five 16-byte loads per lane (the rows of limb Ld-1 and of P are shared by the Ld-1 workgroups of a polynomial's chunk: re-read
// from cache) and one store.  lcs / rcp: the extended context's limb and rescale constants (relative to P), rcq: [Ld-1] relative to q_{Ld-1}.
template <class Arith>
__global__ __launch_bounds__(256) void relin_rescale_kernel(u64* out, const u64* __restrict__ work, const u64* __restrict__ in3, const LimbConst* lcs,
                                                            const RescaleConst* rcp, const RescaleConst* rcq, int n_limbs, int n, int chunks) {
    const int Ld = n_limbs - 1, Lo = Ld - 1;
    const ChunkWork wk = chunk_work(blockIdx.x, chunks, Lo);
    const int limb = wk.limb;
    const size_t poly = wk.poly;   // = b * 2 + comp
    const int w0 = wk.chunk * 512 + threadIdx.x * 2;
    if (w0 >= n) return;
    const RelinRescaleConsts k{lcs[limb], lcs[Lo], rcp[limb], rcp[Lo], rcq[limb]};
    const u64* wp = work + poly * n_limbs * (size_t)n + w0;
    const u64* cp = in3 + ((poly >> 1) * 3 + (poly & 1)) * Ld * (size_t)n + w0;
    const U64x2 wi = *reinterpret_cast<const U64x2*>(wp + (size_t)limb * n);
    const U64x2 wl = *reinterpret_cast<const U64x2*>(wp + (size_t)Lo * n);
    const U64x2 wP = *reinterpret_cast<const U64x2*>(wp + (size_t)Ld * n);
    const U64x2 ci = *reinterpret_cast<const U64x2*>(cp + (size_t)limb * n);
    const U64x2 cl = *reinterpret_cast<const U64x2*>(cp + (size_t)Lo * n);
    *reinterpret_cast<U64x2*>(out + (poly * Lo + limb) * n + w0) =
        U64x2{relin_rescale_word<Arith>(wi.a, wl.a, wP.a, ci.a, cl.a, k), relin_rescale_word<Arith>(wi.b, wl.b, wP.b, ci.b, cl.b, k)};
}

// Scalar linear combination of K ciphertexts per item, a constant on X^0 of component 0, and the rescale (fused_rescale.h (b)):
//   out[t][c] = round((sum_{k<K} w_k x[k][t][c] + [c = 0] w_K) / q_{L-1}).   x: [K][batch][2][L][N], w: [K + 1][L], out: [batch][2][L-1][N].
// Per (polynomial, kept limb, chunk): 2 K 16-byte loads per lane (limb i and the last limb of every term, four terms in flight) and one store; the
// weights are workgroup-uniform (scalar loads).
template <class Arith>
__global__ __launch_bounds__(256) void lincomb_rescale_kernel(u64* out, const u64* __restrict__ x, const u64* __restrict__ w, const LimbConst* lcs,
                                                              const RescaleConst* rcs, int n_limbs, int n, int chunks, int n_terms, size_t batch) {
    const int Lo = n_limbs - 1;
    const ChunkWork wk = chunk_work(blockIdx.x, chunks, Lo);
    const int limb = wk.limb;
    const size_t poly = wk.poly;   // = t * 2 + c
    const int w0 = wk.chunk * 512 + threadIdx.x * 2;
    if (w0 >= n) return;
    const LimbConst lc = lcs[limb], lcl = lcs[Lo];
    const size_t term = batch * 2 * n_limbs * (size_t)n;
    const u64* xi = x + (poly * n_limbs + limb) * n + w0;
    const u64* xl = x + (poly * n_limbs + Lo) * n + w0;
    LazySum si[2] = {{0, 0}, {0, 0}}, sl[2] = {{0, 0}, {0, 0}};
    int k = 0;
    for (; k + 4 <= n_terms; k += 4) {
        U64x2 vi[4], vl[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            vi[u] = *reinterpret_cast<const U64x2*>(xi + (k + u) * term);
            vl[u] = *reinterpret_cast<const U64x2*>(xl + (k + u) * term);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const u64 wi = w[(k + u) * n_limbs + limb], wl = w[(k + u) * n_limbs + Lo];
            lazy_mac(si[0], wi, vi[u].a); lazy_mac(si[1], wi, vi[u].b);
            lazy_mac(sl[0], wl, vl[u].a); lazy_mac(sl[1], wl, vl[u].b);
        }
    }
    for (; k < n_terms; ++k) {
        const U64x2 vi = *reinterpret_cast<const U64x2*>(xi + k * term);
        const U64x2 vl = *reinterpret_cast<const U64x2*>(xl + k * term);
        const u64 wi = w[k * n_limbs + limb], wl = w[k * n_limbs + Lo];
        lazy_mac(si[0], wi, vi.a); lazy_mac(si[1], wi, vi.b);
        lazy_mac(sl[0], wl, vl.a); lazy_mac(sl[1], wl, vl.b);
    }
    if (!(poly & 1) && w0 == 0) { lazy_add(si[0], w[n_terms * n_limbs + limb]); lazy_add(sl[0], w[n_terms * n_limbs + Lo]); }
    const RescaleConst rc = rcs[limb];
    *reinterpret_cast<U64x2*>(out + (poly * Lo + limb) * n + w0) =
        U64x2{rescale_word<Arith>(lazy_reduce<Arith>(si[0], lc), lazy_reduce<Arith>(sl[0], lcl), lc, rc),
              rescale_word<Arith>(lazy_reduce<Arith>(si[1], lc), lazy_reduce<Arith>(sl[1], lcl), lc, rc)};
}

// The last pass of a relinearised product with a scalar linear combination of K <= 15 other ciphertexts and a constant, rescaled at once (fused_rescale.h (c)):
//   out[t][c] = round((w_0 t[t][c] + sum_{k<K} w_{1+k} z_k[t][c] + [c = 0] w_{K+1}) / q_{Ld-1}),   t = (c0, c1) + round(work / P)  (never written).
// work, in3, out, lcs, rcp, rcq as in relin_rescale_kernel; w: [K + 2][Ld]; term k: [batch][2][limbs[k]][N], limbs[k] >= Ld, of which rows `limb` and Ld-1
// are read in place.  The term pointers and their limb counts travel in the kernel arguments (nothing uploaded per call).  Per (polynomial, kept limb,
// chunk): the five 16-byte loads of relin_rescale_kernel, 2 K more (four terms in flight) and one store; the weights are workgroup-uniform (scalar loads).
struct LincombTerms {
    const u64* z[kRelinLincombMaxTerms];
    unsigned limbs[kRelinLincombMaxTerms];
};
template <class Arith>
__global__ __launch_bounds__(256) void relin_lincomb_rescale_kernel(u64* out, const u64* __restrict__ work, const u64* __restrict__ in3, const LincombTerms terms,
                                                                    const u64* __restrict__ w, const LimbConst* lcs, const RescaleConst* rcp,
                                                                    const RescaleConst* rcq, int n_limbs, int n, int chunks, int n_terms) {
    const int Ld = n_limbs - 1, Lo = Ld - 1;
    const ChunkWork wk = chunk_work(blockIdx.x, chunks, Lo);
    const int limb = wk.limb;
    const size_t poly = wk.poly;   // = b * 2 + comp
    const int w0 = wk.chunk * 512 + threadIdx.x * 2;
    if (w0 >= n) return;
    const RelinRescaleConsts k{lcs[limb], lcs[Lo], rcp[limb], rcp[Lo], rcq[limb]};
    const u64* wp = work + poly * n_limbs * (size_t)n + w0;
    const u64* cp = in3 + ((poly >> 1) * 3 + (poly & 1)) * Ld * (size_t)n + w0;
    const U64x2 wi = *reinterpret_cast<const U64x2*>(wp + (size_t)limb * n);
    const U64x2 wl = *reinterpret_cast<const U64x2*>(wp + (size_t)Lo * n);
    const U64x2 wP = *reinterpret_cast<const U64x2*>(wp + (size_t)Ld * n);
    const U64x2 ci = *reinterpret_cast<const U64x2*>(cp + (size_t)limb * n);
    const U64x2 cl = *reinterpret_cast<const U64x2*>(cp + (size_t)Lo * n);
    LazySum si[2] = {{0, 0}, {0, 0}}, sl[2] = {{0, 0}, {0, 0}};
    const u64* wt = w + Ld;   // the terms' rows
    auto row = [&](int t, int l) { return terms.z[t] + (poly * terms.limbs[t] + (size_t)l) * n + w0; };
    int t = 0;
    for (; t + 4 <= n_terms; t += 4) {
        U64x2 vi[4], vl[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            vi[u] = *reinterpret_cast<const U64x2*>(row(t + u, limb));
            vl[u] = *reinterpret_cast<const U64x2*>(row(t + u, Lo));
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const u64 a = wt[(t + u) * Ld + limb], b = wt[(t + u) * Ld + Lo];
            lazy_mac(si[0], a, vi[u].a); lazy_mac(si[1], a, vi[u].b);
            lazy_mac(sl[0], b, vl[u].a); lazy_mac(sl[1], b, vl[u].b);
        }
    }
    for (; t < n_terms; ++t) {
        const U64x2 vi = *reinterpret_cast<const U64x2*>(row(t, limb));
        const U64x2 vl = *reinterpret_cast<const U64x2*>(row(t, Lo));
        const u64 a = wt[t * Ld + limb], b = wt[t * Ld + Lo];
        lazy_mac(si[0], a, vi.a); lazy_mac(si[1], a, vi.b);
        lazy_mac(sl[0], b, vl.a); lazy_mac(sl[1], b, vl.b);
    }
    if (!(poly & 1) && w0 == 0) { lazy_add(si[0], wt[n_terms * Ld + limb]); lazy_add(sl[0], wt[n_terms * Ld + Lo]); }
    const u64 pi = w[limb], pl = w[Lo];
    *reinterpret_cast<U64x2*>(out + (poly * Lo + limb) * n + w0) =
        U64x2{relin_lincomb_rescale_word<Arith>(wi.a, wl.a, wP.a, ci.a, cl.a, pi, pl, si[0], sl[0], k),
              relin_lincomb_rescale_word<Arith>(wi.b, wl.b, wP.b, ci.b, cl.b, pi, pl, si[1], sl[1], k)};
}

// (the exact base extension / scale-and-round kernels live in kernels_bx.h: one kernel per source-limb count, compiled in their own
// translation units k_bx_fold.hip / k_bx_shoup.hip)

// N3, hoisted rotations: digit j of the key-switched component (limb j of c1, coefficient domain, values < q_j) lifted to every
// limb i of the extended basis: out[j][i][k] = c1[j][k] mod q_i (canonical).  One workgroup per (digit, limb, 512-word chunk).
template <class Arith>
// Several input ciphertexts: item t reads c1 + t * in_item_stride and writes out + t * (n_limbs - 1) * n_limbs * n.
__global__ __launch_bounds__(256) void lift_digits_kernel(u64* out, const u64* c1, size_t in_item_stride, const LimbConst* lcs, int n_limbs, int n, int chunks) {
    const int chunk = (int)(blockIdx.x % chunks);
    const int limb = (int)((blockIdx.x / chunks) % n_limbs);
    const size_t dg = blockIdx.x / chunks / n_limbs, item = dg / (unsigned)(n_limbs - 1), digit = dg % (unsigned)(n_limbs - 1);
    c1 += item * in_item_stride;
    out += item * (size_t)(n_limbs - 1) * n_limbs * n;
    const int w0 = chunk * 512 + threadIdx.x * 2;
    if (w0 >= n) return;
    const LimbConst lc = lcs[limb];
    const U64x2 v = *reinterpret_cast<const U64x2*>(c1 + digit * n + w0);
    U64x2 r;
    r.a = Arith::kFold ? FoldArith::canon(v.a, lc) : ShoupArith::mul_var(v.a, 1, lc);
    r.b = Arith::kFold ? FoldArith::canon(v.b, lc) : ShoupArith::mul_var(v.b, 1, lc);
    *reinterpret_cast<U64x2*>(out + (digit * n_limbs + limb) * n + w0) = r;
}

// RNS digits of the key-switched component, lifted to every limb: out[item][j][i][k] = src[item][j][k] mod q_i  (src = component
// `comp` of an `in_comps`-component ciphertext, coefficient domain, limb j holds values < q_j).  out: [batch][L][L][N].
template <class Arith>
__global__ __launch_bounds__(256) void lift_rns_digits_kernel(u64* __restrict__ out, const u64* __restrict__ in, int in_comps, int comp, const LimbConst* lcs,
                                                              int n_limbs, int n, int chunks) {
    const ChunkWork wk = chunk_work(blockIdx.x, chunks, n_limbs);   // poly = (item, digit)
    const int chunk = wk.chunk, limb = wk.limb;
    const size_t dg = wk.poly, item = dg / (unsigned)n_limbs, digit = dg % (unsigned)n_limbs;
    const int w0 = chunk * 512 + threadIdx.x * 2;
    if (w0 >= n) return;
    const LimbConst lc = lcs[limb];
    const U64x2 v = *reinterpret_cast<const U64x2*>(in + (((item * in_comps + comp) * n_limbs) + digit) * n + w0);
    U64x2 r;
    if ((int)digit == limb) r = v;   // already canonical modulo its own prime
    else {
        r.a = Arith::kFold ? FoldArith::canon(v.a, lc) : ShoupArith::mul_var(v.a, 1, lc);
        r.b = Arith::kFold ? FoldArith::canon(v.b, lc) : ShoupArith::mul_var(v.b, 1, lc);
    }
    *reinterpret_cast<U64x2*>(out + ((item * n_limbs + digit) * n_limbs + limb) * n + w0) = r;
}

// acc[item][c][i] = sum_{j < n_digits} x[item][j][i] (.) evk[j][c][i], c = 0, 1 (NTT domain; x: [batch][n_digits][L][N], evk: [n_digits][2][L][N];
// its tiles are re-read from L2).  acc: [batch][2][L][N].  n_digits = L (RNS-digit keys) or L - 1 (hybrid keys: the last limb is the special prime,
// the sum is divided by it afterwards).  Per-item keys (round 5: the batched rotations and the giant steps of a packed layer above N = 8192):
// item i of this launch uses the key at evk + ((item0 + i) / key_group) * key_stride; key_stride = 0 is one key for the whole batch.
template <class Arith>
__global__ __launch_bounds__(256) void key_inner_product_kernel(u64* __restrict__ acc, const u64* __restrict__ x, const u64* __restrict__ evk, const LimbConst* lcs,
                                                                int n_digits, int n_limbs, int n, int chunks, size_t key_stride = 0, unsigned key_group = 1,
                                                                unsigned item0 = 0) {
    const ChunkWork wk = chunk_work(blockIdx.x, chunks, n_limbs);
    const int chunk = wk.chunk, limb = wk.limb;
    const size_t item = wk.poly;
    const int w0 = chunk * 512 + threadIdx.x * 2;
    if (w0 >= n) return;
    const LimbConst lc = lcs[limb];
    evk += ((item + item0) / key_group) * key_stride;
    U64x2 s0{0, 0}, s1{0, 0};
#pragma unroll 2
    for (int j = 0; j < n_digits; ++j) {
        const U64x2 d = *reinterpret_cast<const U64x2*>(x + ((item * n_digits + j) * n_limbs + limb) * n + w0);
        const U64x2 k0 = *reinterpret_cast<const U64x2*>(evk + (((size_t)j * 2 + 0) * n_limbs + limb) * n + w0);
        const U64x2 k1 = *reinterpret_cast<const U64x2*>(evk + (((size_t)j * 2 + 1) * n_limbs + limb) * n + w0);
        s0.a = add_mod(s0.a, Arith::mul_var(d.a, k0.a, lc), lc.q); s0.b = add_mod(s0.b, Arith::mul_var(d.b, k0.b, lc), lc.q);
        s1.a = add_mod(s1.a, Arith::mul_var(d.a, k1.a, lc), lc.q); s1.b = add_mod(s1.b, Arith::mul_var(d.b, k1.b, lc), lc.q);
    }
    *reinterpret_cast<U64x2*>(acc + ((item * 2 + 0) * n_limbs + limb) * n + w0) = s0;
    *reinterpret_cast<U64x2*>(acc + ((item * 2 + 1) * n_limbs + limb) * n + w0) = s1;
}

// out2[item][c] += in[item][c] for the components c whose bit is set in `mask` (in: [batch][in_comps][L][N], coefficient domain)
__global__ __launch_bounds__(256) void add_back_kernel(u64* __restrict__ out2, const u64* __restrict__ in, int in_comps, int mask, const LimbConst* lcs, int n_limbs,
                                                       int n, int chunks) {
    const int chunk = (int)(blockIdx.x % chunks);
    const int limb = (int)((blockIdx.x / chunks) % n_limbs);
    const size_t pc = blockIdx.x / chunks / n_limbs, item = pc >> 1;
    const int comp = (int)(pc & 1);
    const int w0 = chunk * 512 + threadIdx.x * 2;
    if (w0 >= n || !((mask >> comp) & 1)) return;
    const u64 q = lcs[limb].q;
    U64x2* o = reinterpret_cast<U64x2*>(out2 + ((item * 2 + comp) * n_limbs + limb) * n + w0);
    const U64x2 v = *reinterpret_cast<const U64x2*>(in + ((item * in_comps + comp) * n_limbs + limb) * n + w0);
    U64x2 r = *o;
    r.a = add_mod(r.a, v.a, q); r.b = add_mod(r.b, v.b, q);
    *o = r;
}

}  // namespace dpfhe
