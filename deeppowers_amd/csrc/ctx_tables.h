// ctx_tables.h - host-side construction of the table blobs of a context: every byte the kernels read through
// DevTables / MixedTables (devtables.h).  Plain C++17, no HIP: dpfhe_ctx_create (cabi_ctx.hip) uploads these blobs
// and tools/emulate.cpp runs the kernels' per-thread code on them, so the CPU proofs cover the shipped arrangement.
#pragma once
#include <cstring>
#include <vector>

#include "devtables.h"
#include "ntt_core.h"
#include "ntt_quarters.h"
#include "tables.h"

namespace dpfhe {

// ---- one packing routine -------------------------------------------------------------------------------------------
// every class's twiddle is 16 bytes, so the per-limb slots of all tables share one stride and one builder serves every class
static_assert(sizeof(TwShoup) == 16 && sizeof(TwFold) == 16 && sizeof(TwF64) == 16, "the twiddle slots of every class share one stride");
struct alignas(16) TwBytes { u64 lo, hi; };   // a twiddle as stored, whichever class reads it
constexpr size_t kTwSize = sizeof(TwBytes);

template <class Tw> inline TwBytes tw_bytes(const Tw& t) { static_assert(sizeof(Tw) == sizeof(TwBytes), "slot size"); TwBytes r; std::memcpy(&r, &t, sizeof r); return r; }
// the twiddle of w (< q) in the format of class k
inline TwBytes class_tw(LimbClass k, u64 w, u64 q) {
    if (k == kClassFold) return tw_bytes(h_tw_fold(w, q));
    if (k == kClassFoldScaled) return tw_bytes(h_tw_fold_scaled(w, q, fold_scaled_shift(q)));
    if (k == kClassF64 || k == kClassF64Wide) return tw_bytes(h_make_tw<TwF64>(w, q));
    return tw_bytes(h_make_tw<TwShoup>(w, q));
}
inline InvLast<TwBytes> class_last(LimbClass k, u64 w_last, u64 w_ninv, u64 q) { return InvLast<TwBytes>{class_tw(k, w_last, q), class_tw(k, w_ninv, q)}; }
// one 2^logn_tab-point table at dst, in the layout kernel geometry (logn_tab, loge) reads (tables.h permute_window0)
inline void pack_table(unsigned char* dst, const std::vector<u64>& words, LimbClass k, u64 q, int logn_tab, int loge) {
    std::vector<TwBytes> t(words.size());
    for (size_t i = 0; i < words.size(); ++i) t[i] = class_tw(k, words[i], q);
    permute_window0(t, logn_tab, loge, geo_perm_stages(logn_tab, loge));
    std::memcpy(dst, t.data(), t.size() * kTwSize);
}
// the 2^log_n1 sub-tree tables of one limb (tables.h subtree_table), [r][N >> log_n1] at dst, each in the layout of geometry (log2n - log_n1, loge)
inline void pack_subtrees(unsigned char* dst, const std::vector<u64>& table, LimbClass k, u64 q, int log2n, int log_n1, int loge) {
    const size_t n2 = (size_t)1 << (log2n - log_n1);
    for (size_t r = 0; r < (size_t)1 << log_n1; ++r) pack_table(dst + r * n2 * kTwSize, subtree_table(table, log2n, log_n1, r), k, q, log2n - log_n1, loge);
}

// ---- the class blob ------------------------------------------------------------------------------------------------
// Tables of a context with per-limb arithmetic classes (round 6): ONE blob, LimbConst[L] | fwd | inv | last[L] | last2[L], every per-limb slot in the
// format of that limb's class.  The classes' DevTables are typed views of the same blob, each with its own active-limb map.  Single-kernel transforms
// only (log2 N <= 14).
struct MixedLayout { size_t o_lc, o_fwd, o_inv, o_last, o_last2, total; };
inline MixedLayout mixed_layout(int log2n, size_t L) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t n = (size_t)1 << log2n, tab = L * n * kTwSize;
    MixedLayout m;
    m.o_lc = 0; m.o_fwd = up(L * sizeof(LimbConst)); m.o_inv = up(m.o_fwd + tab);
    m.o_last = up(m.o_inv + tab); m.o_last2 = up(m.o_last + L * 32); m.total = up(m.o_last2 + L * 32);
    return m;
}
// limb_cls[l]: the LimbClass limb l runs on (dpfhe_ctx_create: tables.h limb_class of its prime; the emulator: the policy under test)
inline std::vector<unsigned char> build_class_blob(int log2n, const std::vector<HostLimbTables>& ht, const unsigned char* limb_cls) {
    const size_t L = ht.size(), slot = ((size_t)1 << log2n) * kTwSize;
    const MixedLayout m = mixed_layout(log2n, L);
    std::vector<unsigned char> blob(m.total, 0);
    for (size_t l = 0; l < L; ++l) {
        const HostLimbTables& t = ht[l];
        const LimbClass cls = (LimbClass)limb_cls[l];
        const u64 q = t.lc.q;
        const LimbConst lc = limb_const_of_class(t.lc, cls);
        std::memcpy(&blob[m.o_lc + l * sizeof(LimbConst)], &lc, sizeof(LimbConst));
        pack_table(&blob[m.o_fwd + l * slot], t.rp, cls, q, log2n, kLoge);
        pack_table(&blob[m.o_inv + l * slot], t.irp, cls, q, log2n, kLoge);
        reinterpret_cast<InvLast<TwBytes>*>(&blob[m.o_last])[l] = class_last(cls, t.w_last, t.lc.ninv, q);
        // products of two scaled words carry s = 2^(60-k) twice: their inverse transform ends on twiddles with s^-1 folded in (DevTables::last2)
        const u64 sinv = cls == kClassFoldScaled ? h_powmod((1ull << fold_scaled_shift(q)) % q, q - 2, q) : 1;
        reinterpret_cast<InvLast<TwBytes>*>(&blob[m.o_last2])[l] = class_last(cls, h_mulmod(t.w_last, sinv, q), h_mulmod(t.lc.ninv, sinv, q), q);
    }
    return blob;
}
template <class Arith>
inline DevTables<Arith> mixed_view(const unsigned char* b, const MixedLayout& m, size_t L) {
    typedef typename Arith::Tw Tw;
    DevTables<Arith> tb{};
    tb.lc = reinterpret_cast<const LimbConst*>(b + m.o_lc);
    tb.fwd = reinterpret_cast<const Tw*>(b + m.o_fwd); tb.inv = reinterpret_cast<const Tw*>(b + m.o_inv);
    tb.last = reinterpret_cast<const InvLast<Tw>*>(b + m.o_last);
    tb.last2 = reinterpret_cast<const InvLast<Tw>*>(b + m.o_last2);
    tb.n_sub = 1;
    tb.n_limbs = (int)L;
    return tb;
}
// Which contexts have a class blob, and on which classes: L <= 16, 8 <= log2 N <= 14, not all-fold, and at least one limb with a faster class than the
// generic policy.  Fills limb_cls[0 .. L) when it returns true.
inline bool ctx_limb_classes(int log2n, const std::vector<HostLimbTables>& ht, bool fold, unsigned char limb_cls[16]) {
    if (fold || ht.size() > 16 || log2n < 8 || log2n > 14) return false;
    bool any_fast = false;
    for (size_t l = 0; l < ht.size(); ++l) { limb_cls[l] = (unsigned char)limb_class(ht[l].lc.q); any_fast = any_fast || limb_cls[l] != kClassShoup; }
    return any_fast;
}

// ---- the lazy-multiply blob ----------------------------------------------------------------------------------------
// Round 11: the fused multiply of the pinned primes at N = 4096 runs its transforms on twiddles split at bit 29 (FoldArith::mul_tw29_add, NttBody's
// LAZY29 plans).  Those tables live in a blob of their own - fwd29 | inv29 | last29, [L] slots with only the fold limbs' filled - next
// to the context-wide blob and the class blob, which stay byte for byte what they were.  Built for every context at log2 N = 12 in which a limb runs on
// FoldArith: the all-fold contexts, and the fold limbs of a context with per-limb classes (they launch the same kernel).
constexpr int kLazy29Log2N = 12;
struct Lazy29Layout { size_t o_fwd, o_inv, o_last, total; };
inline Lazy29Layout lazy29_layout(size_t L) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t tab = L * ((size_t)1 << kLazy29Log2N) * kTwSize;
    Lazy29Layout m;
    m.o_fwd = 0; m.o_inv = up(tab); m.o_last = up(m.o_inv + tab); m.total = up(m.o_last + L * 2 * kTwSize);
    return m;
}
// fold_limb[l]: limb l runs on FoldArith.  Returns an empty blob when the context has no use for one.
inline std::vector<unsigned char> build_lazy29_blob(int log2n, const std::vector<HostLimbTables>& ht, const std::vector<bool>& fold_limb) {
    bool any = false;
    for (size_t l = 0; l < ht.size(); ++l) any = any || fold_limb[l];
    if (log2n != kLazy29Log2N || !any) return {};
    const size_t L = ht.size(), n = (size_t)1 << log2n;
    const Lazy29Layout m = lazy29_layout(L);
    std::vector<unsigned char> blob(m.total, 0);
    auto pack29 = [&](size_t off, const std::vector<u64>& words, u64 q) {
        std::vector<TwBytes> t(words.size());
        for (size_t i = 0; i < words.size(); ++i) t[i] = tw_bytes(h_tw_fold29(words[i], q));
        permute_window0(t, log2n, kLoge, geo_perm_stages(log2n, kLoge));
        std::memcpy(&blob[off], t.data(), t.size() * kTwSize);
    };
    for (size_t l = 0; l < L; ++l) {
        if (!fold_limb[l]) continue;
        const HostLimbTables& t = ht[l];
        const u64 q = t.lc.q;
        pack29(m.o_fwd + l * n * kTwSize, t.rp, q);
        pack29(m.o_inv + l * n * kTwSize, t.irp, q);
        reinterpret_cast<InvLast<TwBytes>*>(&blob[m.o_last])[l] = InvLast<TwBytes>{tw_bytes(h_tw_fold29(t.w_last, q)), tw_bytes(h_tw_fold29(t.lc.ninv, q))};
    }
    return blob;
}
inline void lazy29_view(DevTables<FoldArith>& tb, const unsigned char* d, const Lazy29Layout& m) {
    tb.fwd29 = reinterpret_cast<const TwFold*>(d + m.o_fwd); tb.inv29 = reinterpret_cast<const TwFold*>(d + m.o_inv);
    tb.last29 = reinterpret_cast<const InvLast<TwFold>*>(d + m.o_last);
}

// ---- the context-wide blob -----------------------------------------------------------------------------------------
// Tables of the context-wide arithmetic (FoldArith or ShoupArith, every limb): ONE blob of 256-byte aligned sections.  One twiddle table pair
// (fwd | inv), in the layout every kernel reads (devtables.h kLoge).  Split transforms (N > 16384) store, per limb, n_sub tables of N2 points (sub-trees of the full table) plus the top-stage twiddles.  FoldArith at N = 8192 / 16384 adds the "halves" /
// "quarters" tables next to the one-piece ones (ntt_halves.h / ntt_quarters.h; the fused kernels keep the one-piece layout); elsewhere their offsets are
// the end of the blob and their pointers stay null.
struct CtxLayout {
    int log_n1, log_n2;
    size_t n_sub, n2;
    bool split, halves, quarters;
    size_t o_lc, o_fwd, o_inv, o_last, o_top_fwd, o_top_inv, o_top_last, o_resc, o_hfwd, o_hinv, o_htop_fwd, o_htop_last,
           o_qfwd, o_qinv, o_qtop_fwd, o_qtop_inv, o_qtop_last, total;
};
inline CtxLayout ctx_layout(int log2n, size_t L, bool fold) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    CtxLayout m;
    m.log_n1 = split_log_n1(log2n); m.log_n2 = log2n - m.log_n1;
    m.n_sub = (size_t)1 << m.log_n1; m.n2 = (size_t)1 << m.log_n2;
    m.split = m.log_n1 > 0;
    m.halves = log2n == 13 && fold;     // the halves tables (launch.h): large batched transforms at N = 8192
    m.quarters = log2n == 14 && fold;   // four sub-tree tables per limb + the column stages' twiddles
    const size_t n_sub = m.n_sub, tab = L * ((size_t)1 << log2n) * kTwSize;
    m.o_lc = 0; m.o_fwd = up(m.o_lc + L * sizeof(LimbConst)); m.o_inv = up(m.o_fwd + tab);
    m.o_last = up(m.o_inv + tab); m.o_top_fwd = up(m.o_last + L * n_sub * 2 * kTwSize); m.o_top_inv = up(m.o_top_fwd + L * n_sub * kTwSize);
    m.o_top_last = up(m.o_top_inv + L * n_sub * kTwSize); m.o_resc = up(m.o_top_last + L * 2 * kTwSize);
    const bool h = m.halves, qu = m.quarters;
    m.o_hfwd = up(m.o_resc + L * sizeof(RescaleConst)); m.o_hinv = h ? up(m.o_hfwd + tab) : m.o_hfwd; m.o_htop_fwd = h ? up(m.o_hinv + tab) : m.o_hfwd;
    m.o_htop_last = h ? up(m.o_htop_fwd + L * kTwSize) : m.o_hfwd;
    const size_t o_q0 = h ? up(m.o_htop_last + L * 2 * kTwSize) : m.o_hfwd;
    m.o_qfwd = o_q0; m.o_qinv = qu ? up(m.o_qfwd + tab) : o_q0; m.o_qtop_fwd = qu ? up(m.o_qinv + tab) : o_q0;
    m.o_qtop_inv = qu ? up(m.o_qtop_fwd + L * sizeof(QuartersTop)) : o_q0; m.o_qtop_last = qu ? up(m.o_qtop_inv + L * 2 * kTwSize) : o_q0;
    m.total = qu ? up(m.o_qtop_last + L * 2 * kTwSize) : o_q0;
    return m;
}
// `fold`: every limb is a pinned 2^60 - d prime and the tables are FoldArith's; otherwise ShoupArith's
inline std::vector<unsigned char> build_ctx_blob(int log2n, const std::vector<HostLimbTables>& ht, bool fold) {
    const size_t L = ht.size(), n = (size_t)1 << log2n;
    const CtxLayout lay = ctx_layout(log2n, L, fold);
    const size_t n_sub = lay.n_sub, n2 = lay.n2;
    const LimbClass k = fold ? kClassFold : kClassShoup;
    std::vector<unsigned char> blob(lay.total, 0);
    auto tws = [&](size_t off) { return reinterpret_cast<TwBytes*>(&blob[off]); };
    auto lasts = [&](size_t off) { return reinterpret_cast<InvLast<TwBytes>*>(&blob[off]); };
    for (size_t l = 0; l < L; ++l) {
        const HostLimbTables& t = ht[l];
        const u64 q = t.lc.q;
        std::memcpy(&blob[lay.o_lc + l * sizeof(LimbConst)], &t.lc, sizeof(LimbConst));
        if (!lay.split) {
            pack_table(&blob[lay.o_fwd + l * n * kTwSize], t.rp, k, q, log2n, kLoge);
            pack_table(&blob[lay.o_inv + l * n * kTwSize], t.irp, k, q, log2n, kLoge);
            lasts(lay.o_last)[l] = class_last(k, t.w_last, t.lc.ninv, q);
            if (lay.quarters) {
                pack_subtrees(&blob[lay.o_qfwd + l * n * kTwSize], t.rp, k, q, 14, 2, 4);
                pack_subtrees(&blob[lay.o_qinv + l * n * kTwSize], t.irp, k, q, 14, 2, 4);
                reinterpret_cast<QuartersTop*>(&blob[lay.o_qtop_fwd])[l] = QuartersTop{h_tw_fold(t.rp[1], q), h_tw_fold(t.rp[2], q), h_tw_fold(t.rp[3], q)};
                for (size_t i = 0; i < 2; ++i) tws(lay.o_qtop_inv)[2 * l + i] = class_tw(k, t.irp[2 + i], q);
                lasts(lay.o_qtop_last)[l] = lasts(lay.o_last)[l];
            }
            if (lay.halves) {
                pack_subtrees(&blob[lay.o_hfwd + l * n * kTwSize], t.rp, k, q, 13, 1, 4);
                pack_subtrees(&blob[lay.o_hinv + l * n * kTwSize], t.irp, k, q, 13, 1, 4);
                tws(lay.o_htop_fwd)[l] = class_tw(k, t.rp[1], q);
                lasts(lay.o_htop_last)[l] = lasts(lay.o_last)[l];   // the column stage IS the one-piece transform's last stage
            }
        } else {
            pack_subtrees(&blob[lay.o_fwd + l * n * kTwSize], t.rp, k, q, log2n, lay.log_n1, kLoge);
            pack_subtrees(&blob[lay.o_inv + l * n * kTwSize], t.irp, k, q, log2n, lay.log_n1, kLoge);
            // generic primes: no N^-1 inside a block.  FoldArith: the block's last stage divides its sums by N2 exactly (FoldArith::mul_ninv),
            // so its differences carry N2^-1 in their twiddle; the column stage then multiplies by N1^-1 (top_last below)
            const u64 n2inv = fold ? h_powmod((u64)n2 % q, q - 2, q) : 1;
            for (size_t r = 0; r < n_sub; ++r)   // (entry 1 of sub-tree r's table: tables.h subtree_table)
                lasts(lay.o_last)[l * n_sub + r] = class_last(k, h_mulmod(t.irp[n_sub + r], n2inv, q), 1, q);
            for (size_t i = 1; i < n_sub; ++i) { tws(lay.o_top_fwd)[l * n_sub + i] = class_tw(k, t.rp[i], q); tws(lay.o_top_inv)[l * n_sub + i] = class_tw(k, t.irp[i], q); }
            // FoldArith sub-transforms divide by their own length N2 in their last stage (ntt_core.h: FoldArith::mul_ninv, exact division), so the
            // column stage multiplies by N1^-1 = N^-1 N2 only; generic-prime sub-transforms multiply by 1 there and the column stage by N^-1
            const u64 up = fold ? (u64)n2 % q : 1;
            lasts(lay.o_top_last)[l] = class_last(k, h_mulmod(t.w_last, up, q), h_mulmod(t.lc.ninv, up, q), q);
        }
    }
    // rescale constants relative to the LAST prime (used only when L >= 2)
    const u64 ql = ht[L - 1].lc.q, hh = ql / 2;
    RescaleConst* r = reinterpret_cast<RescaleConst*>(&blob[lay.o_resc]);
    for (size_t l = 0; l + 1 < L; ++l) {
        const u64 q = ht[l].lc.q;
        r[l].h_mod = hh % q; r[l].inv = h_powmod(ql % q, q - 2, q); r[l].q_last = ql; r[l].h = hh;
    }
    return blob;
}
template <class Arith>
inline DevTables<Arith> ctx_view(const unsigned char* d, const CtxLayout& m, size_t L) {
    typedef typename Arith::Tw Tw;
    DevTables<Arith> tb{};
    tb.lc = reinterpret_cast<const LimbConst*>(d + m.o_lc);
    tb.fwd = reinterpret_cast<const Tw*>(d + m.o_fwd); tb.inv = reinterpret_cast<const Tw*>(d + m.o_inv);
    tb.last = reinterpret_cast<const InvLast<Tw>*>(d + m.o_last);
    tb.top_fwd = reinterpret_cast<const Tw*>(d + m.o_top_fwd); tb.top_inv = reinterpret_cast<const Tw*>(d + m.o_top_inv);
    tb.top_last = reinterpret_cast<const InvLast<Tw>*>(d + m.o_top_last);
    tb.n_sub = (int)m.n_sub;
    tb.n_limbs = (int)L;
    if (m.quarters) {
        tb.qfwd = reinterpret_cast<const Tw*>(d + m.o_qfwd); tb.qinv = reinterpret_cast<const Tw*>(d + m.o_qinv);
        tb.qtop_fwd = reinterpret_cast<const QuartersTop*>(d + m.o_qtop_fwd); tb.qtop_inv = reinterpret_cast<const Tw*>(d + m.o_qtop_inv);
        tb.qtop_last = reinterpret_cast<const InvLast<Tw>*>(d + m.o_qtop_last);
    }
    if (m.halves) {
        tb.hfwd = reinterpret_cast<const Tw*>(d + m.o_hfwd); tb.hinv = reinterpret_cast<const Tw*>(d + m.o_hinv);
        tb.htop_fwd = reinterpret_cast<const Tw*>(d + m.o_htop_fwd); tb.htop_last = reinterpret_cast<const InvLast<Tw>*>(d + m.o_htop_last);
    }
    return tb;
}

}  // namespace dpfhe
