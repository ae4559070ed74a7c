// fused_rescale.h - the one-pass rescales of the approximate (CKKS-style) family's activations: a relinearised product that drops P and the last
// data prime together, a scalar linear combination of ciphertexts with a constant that drops the last prime, and the two in one (a Newton or Horner step).
//
//   rescale step (kernels_keyswitch.h rescale_kernel):  R(x, last; q_last)_i = ((x_i + h) - ((last + h) mod q_last)) q_last^-1  mod q_i,  h = floor(q_last / 2)
//   = round(X / q_last) mod q_i of the value X the limbs hold.  Every step is modular and local to the coefficient, so two of them chain without a
//   round trip through memory as long as the intermediate word of the NEXT divisor's limb is carried along:
//
//   (a) last pass of dpfhe_relinearize_rescale_hybrid.  work: the key-switched sums over Q P, (c0, c1): the product's first two components, Ld data limbs.
//         t_i    = R(work_i,    work_P; P)_i    + c_i       mod q_i         (what dpfhe_relinearize_hybrid writes on limb i)
//         t_last = R(work_last, work_P; P)_last + c_last    mod q_{Ld-1}    (... on the last data limb)
//         out_i  = R(t_i, t_last; q_{Ld-1})_i                                (what dpfhe_rescale makes of them), i < Ld - 1
//   (b) dpfhe_lincomb_rescale.  s_l = sum_{k<K} w_k,l x_k,l + [constant word] w_K,l  mod q_l  on limb i and on the last limb, then out_i = R(s_i, s_last; q_{L-1})_i.
//       Canonical words are below 2^60, so K + 1 <= 17 products sum below 17 2^120 < 2^125: one 128-bit lazy sum per word, reduced once.
//   (c) last pass of dpfhe_relinearize_lincomb_rescale_hybrid: (a)'s t_i and t_last are never written; they enter (b)'s lazy sums as one more product, ahead of
//       K <= 15 addends z_k read on limbs i and Ld-1 of whatever level they live on (the first Ld limbs of a longer chain ARE the level drop):
//         s_l   = w_0,l t_l + sum_{k<K} w_1+k,l z_k,l + [constant word] w_K+1,l   mod q_l,   l in {i, Ld-1}
//         out_i = R(s_i, s_last; q_{Ld-1})_i,   i < Ld - 1
//       At most 16 products and the constant: (b)'s bound.  With K = 0, w_0 = 1 and no constant this is (a); in general it is dpfhe_relinearize_hybrid's words
//       followed by (b) on the data limbs over [t, z_0, ...].
//
// All results are canonical residues, so the words do not depend on how a policy reduces: Arith::kFold picks FoldArith's folds, anything else the
// generic 128-bit Barrett products, as in every other streaming kernel (cabi.h with_ctx_arith).
//
// Shared by the device kernels (kernels_keyswitch.h: every rescale there, plain or fused, is rescale_word) and the host twins below
// (dpfhe_relinearize_rescale_pass_host, dpfhe_lincomb_rescale_host, dpfhe_relinearize_lincomb_rescale_pass_host): one statement of the arithmetic.  No HIP in here.
#pragma once
#include <stddef.h>

#include "devtables.h"

namespace dpfhe {

constexpr size_t kLincombMaxTerms = 16;
constexpr size_t kRelinLincombMaxTerms = kLincombMaxTerms - 1;   // (c): the product takes one of the 16 places

// x mod q_i for a canonical word of ANOTHER limb (x < 2^60)
template <class Arith>
DPF_HD u64 to_limb(u64 x, const LimbConst& lc) {
    if (Arith::kFold) return FoldArith::canon(x, lc);
    return ShoupArith::mul_var(x, 1, lc);
}

// one rescale step on limb i: x canonical mod q_i, last canonical mod rc.q_last
template <class Arith>
DPF_HD u64 rescale_word(u64 x, u64 last, const LimbConst& lc, const RescaleConst& rc) {
    const u64 t = csub(last + rc.h, rc.q_last);                    // (last + h) mod q_last
    const u64 d = sub_mod(add_mod(x, rc.h_mod, lc.q), to_limb<Arith>(t, lc), lc.q);
    return Arith::mul_var(d, rc.inv, lc);
}

// (a): the constants of one kept limb i and of the last data limb, both relative to P (the extended context's own table), and of limb i relative to
// the last data prime (the second table)
struct RelinRescaleConsts {
    LimbConst lc_i, lc_last;
    RescaleConst p_i, p_last, q_i;
};
template <class Arith>
DPF_HD u64 relin_rescale_word(u64 work_i, u64 work_last, u64 work_p, u64 c_i, u64 c_last, const RelinRescaleConsts& k) {
    const u64 t_i = add_mod(rescale_word<Arith>(work_i, work_p, k.lc_i, k.p_i), c_i, k.lc_i.q);
    const u64 t_last = add_mod(rescale_word<Arith>(work_last, work_p, k.lc_last, k.p_last), c_last, k.lc_last.q);
    return rescale_word<Arith>(t_i, t_last, k.lc_i, k.q_i);
}

// (b): the lazy sum of products of canonical words
struct LazySum {
    u64 lo, hi;
};
DPF_HD void lazy_mac(LazySum& s, u64 a, u64 b) {
    const u64 lo = a * b, hi = mulhi64(a, b);
    s.lo += lo;
    s.hi += hi + (s.lo < lo);
}
DPF_HD void lazy_add(LazySum& s, u64 a) {
    s.lo += a;
    s.hi += (s.lo < a);
}
// hi 2^64 + lo mod q, canonical; hi < 2^61 (at most 17 products of words below 2^60)
template <class Arith>
DPF_HD u64 lazy_reduce(const LazySum& s, const LimbConst& lc) {
    if (Arith::kFold) {   // hi (2^64 mod q) + lo, both folded below 2^60 + 2^53
        const u64 h = FoldArith::mul60_full(s.hi, lc.two64, (u32)lc.d);
        return FoldArith::canon(h + FoldArith::reduce(s.lo, lc), lc);
    }
    return add_mod(ShoupArith::mul_var(s.hi, lc.two64, lc), ShoupArith::mul_var(s.lo, 1, lc), lc.q);
}

// (c): si / sl are the lazy sums of the addends (and of the constant word) on limb i and on the last data limb; the relinearised product joins them with its
// weight on either limb before the one reduction
template <class Arith>
DPF_HD u64 relin_lincomb_rescale_word(u64 work_i, u64 work_last, u64 work_p, u64 c_i, u64 c_last, u64 w_i, u64 w_last, LazySum si, LazySum sl,
                                      const RelinRescaleConsts& k) {
    const u64 t_i = add_mod(rescale_word<Arith>(work_i, work_p, k.lc_i, k.p_i), c_i, k.lc_i.q);
    const u64 t_last = add_mod(rescale_word<Arith>(work_last, work_p, k.lc_last, k.p_last), c_last, k.lc_last.q);
    lazy_mac(si, w_i, t_i);
    lazy_mac(sl, w_last, t_last);
    return rescale_word<Arith>(lazy_reduce<Arith>(si, k.lc_i), lazy_reduce<Arith>(sl, k.lc_last), k.lc_i, k.q_i);
}

// the rescale constants of limbs [0, last) relative to limb `last` (ctx_tables.h fills the context's own table the same way); the moduli pairwise coprime
// primes or not, q_last^-1 comes from `inv(q_last mod q_i, q_i)`
template <class Inv>
inline void fill_rescale_consts(RescaleConst* r, const u64* moduli, size_t last, Inv inv) {
    const u64 ql = moduli[last], hh = ql / 2;
    for (size_t l = 0; l < last; ++l) r[l] = RescaleConst{hh % moduli[l], inv(ql % moduli[l], moduli[l]), ql, hh};
}

// ---- host twins: the same words, one coefficient at a time -----------------------------------------------------------------------------------------
// (a)  work: [batch][2][L][N] over Q P, in3: [batch][3][Ld][N], out: [batch][2][Ld-1][N];  lc: [L], rc_p: [L-1] relative to P, rc_q: [Ld-1] relative to q_{Ld-1}
template <class Arith>
inline void relin_rescale_pass_host(size_t n, size_t L, const LimbConst* lc, const RescaleConst* rc_p, const RescaleConst* rc_q, u64* out, const u64* work,
                                    const u64* in3, size_t batch) {
    const size_t Ld = L - 1, Lo = Ld - 1;
    for (size_t p = 0; p < 2 * batch; ++p)
        for (size_t i = 0; i < Lo; ++i) {
            const RelinRescaleConsts k{lc[i], lc[Lo], rc_p[i], rc_p[Lo], rc_q[i]};
            const u64* w = work + p * L * n;
            const u64* c = in3 + ((p >> 1) * 3 + (p & 1)) * Ld * n;
            for (size_t j = 0; j < n; ++j)
                out[(p * Lo + i) * n + j] = relin_rescale_word<Arith>(w[i * n + j], w[Lo * n + j], w[Ld * n + j], c[i * n + j], c[Lo * n + j], k);
        }
}

// (b)  x: [K][batch][2][L][N], w: [K + 1][L], out: [batch][2][L-1][N];  lc: [L], rc: [L-1] relative to q_{L-1}
template <class Arith>
inline void lincomb_rescale_host(size_t n, size_t L, const LimbConst* lc, const RescaleConst* rc, u64* out, const u64* x, const u64* w, size_t K, size_t batch) {
    const size_t Lo = L - 1, term = batch * 2 * L * n;
    for (size_t p = 0; p < 2 * batch; ++p)
        for (size_t i = 0; i < Lo; ++i)
            for (size_t j = 0; j < n; ++j) {
                LazySum si{0, 0}, sl{0, 0};
                for (size_t k = 0; k < K; ++k) {
                    lazy_mac(si, w[k * L + i], x[k * term + (p * L + i) * n + j]);
                    lazy_mac(sl, w[k * L + Lo], x[k * term + (p * L + Lo) * n + j]);
                }
                if (!(p & 1) && j == 0) { lazy_add(si, w[K * L + i]); lazy_add(sl, w[K * L + Lo]); }
                out[(p * Lo + i) * n + j] = rescale_word<Arith>(lazy_reduce<Arith>(si, lc[i]), lazy_reduce<Arith>(sl, lc[Lo]), lc[i], rc[i]);
            }
}

// (c)  work, in3, out, lc, rc_p, rc_q as in (a);  terms: K pointers, term k [batch][2][term_limbs[k]][N] of which the first Ld limbs are read;  w: [K + 2][Ld]
template <class Arith>
inline void relin_lincomb_rescale_pass_host(size_t n, size_t L, const LimbConst* lc, const RescaleConst* rc_p, const RescaleConst* rc_q, u64* out, const u64* work,
                                            const u64* in3, const u64* const* terms, const unsigned* term_limbs, size_t K, const u64* w, size_t batch) {
    const size_t Ld = L - 1, Lo = Ld - 1;
    for (size_t p = 0; p < 2 * batch; ++p)
        for (size_t i = 0; i < Lo; ++i) {
            const RelinRescaleConsts k{lc[i], lc[Lo], rc_p[i], rc_p[Lo], rc_q[i]};
            const u64* wk = work + p * L * n;
            const u64* c = in3 + ((p >> 1) * 3 + (p & 1)) * Ld * n;
            for (size_t j = 0; j < n; ++j) {
                LazySum si{0, 0}, sl{0, 0};
                for (size_t t = 0; t < K; ++t) {
                    const u64* z = terms[t] + p * term_limbs[t] * n + j;
                    lazy_mac(si, w[(1 + t) * Ld + i], z[i * n]);
                    lazy_mac(sl, w[(1 + t) * Ld + Lo], z[Lo * n]);
                }
                if (!(p & 1) && j == 0) { lazy_add(si, w[(K + 1) * Ld + i]); lazy_add(sl, w[(K + 1) * Ld + Lo]); }
                out[(p * Lo + i) * n + j] = relin_lincomb_rescale_word<Arith>(wk[i * n + j], wk[Lo * n + j], wk[Ld * n + j], c[i * n + j], c[Lo * n + j], w[i], w[Lo], si, sl, k);
            }
        }
}

}  // namespace dpfhe
