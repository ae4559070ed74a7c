// emulate.cpp - CPU emulation of the HIP NTT kernels (TEST INFRASTRUCTURE).
//
// Runs the exact per-thread code of deeppowers_amd/csrc/ntt_core.h for every thread id of one
// workgroup, step by step between barriers, with LDS as a plain array.  tests/test_emulated_kernels.py
// compares the result with the oracle, so index/twiddle/padding/bound-plan logic is proven on the CPU
// before any GPU minute is spent.  Built by tests (g++), never shipped, never on the product path.
#define DPFHE_EMU_CHECK 1
#include <cstring>
#include <vector>

#include "../deeppowers_amd/csrc/ctx_tables.h"
#include "../deeppowers_amd/csrc/ntt_halves.h"
#include "../deeppowers_amd/csrc/ntt_top.h"

namespace dpfhe { long g_emu_overflows = 0; }
using namespace dpfhe;
extern "C" long emu_overflows() { return g_emu_overflows; }
// modarith.h DPFHE_EMU_NOTE: per site (EmuSite, in declaration order) bit i = the i-th remainder-edge value has been returned, bit 31 = the site was reached
extern "C" void emu_notes_reset() { std::memset(g_emu_notes, 0, sizeof g_emu_notes); }
extern "C" int emu_notes_get(unsigned* out, int cap) {
    for (int i = 0; i < kEmuSiteCount && i < cap; ++i) out[i] = g_emu_notes[i];
    return kEmuSiteCount;
}

// ---- the tables the emulated kernels read ----------------------------------------------------------------------------
// Built by ctx_tables.h, the code dpfhe_ctx_create uploads from, and read through the same DevTables views with the kernels' own indexing
// (limb and sub-tree strides included); the single-prime entry points below are the n_limbs = 1 case.
template <class Arith> static bool class_ok(u64 q) {
    if (Arith::kFold) return fold_eligible(q);
    if constexpr (Arith::kF64) return q < (1ull << Arith::kMaxBits);
    if (Arith::kFoldCore) return fold_scaled_shift(q) != 0;
    return true;
}
template <class Arith> static constexpr LimbClass class_of() {
    if constexpr (Arith::kF64) return Arith::kMaxBits == F64Arith::kMaxBits ? kClassF64 : kClassF64Wide;
    else return Arith::kFold ? kClassFold : Arith::kFoldCore ? kClassFoldScaled : kClassShoup;
}
// fn(Arith{}) on the policy of class `arith` (tables.h LimbClass)
template <class Fn> static int with_arith(int arith, Fn fn) {
    switch (arith) {
        case kClassShoup: return fn(ShoupArith{});
        case kClassFold: return fn(FoldArith{});
        case kClassF64: return fn(F64Arith{});
        case kClassFoldScaled: return fn(FoldScaledArith{});
        case kClassF64Wide: return fn(F64WideArith{});
        default: return -1;
    }
}

template <class Arith> struct Tables {
    std::vector<unsigned char> blob;   // the bytes a context would upload
    DevTables<Arith> tb{};             // the kernels' view of them, over this host copy
};
static int limb_tables(int log2n, int n_limbs, const u64* moduli, const u64* psi, std::vector<HostLimbTables>& ht) {
    ht.resize((size_t)n_limbs);
    for (int l = 0; l < n_limbs; ++l) if (int rc = build_limb_tables(log2n, moduli[l], psi[l], ht[(size_t)l])) return rc;
    return 0;
}
// the class blob with limb l on class limb_cls[l], seen as Arith's (DevTables of a context with per-limb classes: dpfhe_ctx::cls_*)
template <class Arith>
static void class_tables(int log2n, const std::vector<HostLimbTables>& ht, const unsigned char* limb_cls, Tables<Arith>& t) {
    t.blob = build_class_blob(log2n, ht, limb_cls);
    t.tb = mixed_view<Arith>(t.blob.data(), mixed_layout(log2n, ht.size()), ht.size());
}
// The tables of a context that runs EVERY limb on Arith - the policy under test, whatever tables.h limb_class would choose: the context-wide blob for
// FoldArith / ShoupArith, the class blob for the other classes.  2000: a prime the policy does not take.
template <class Arith>
static int policy_tables(int log2n, const std::vector<HostLimbTables>& ht, Tables<Arith>& t) {
    for (const HostLimbTables& h : ht) if (!class_ok<Arith>(h.lc.q)) return 2000;
    if constexpr (class_of<Arith>() == kClassFold || class_of<Arith>() == kClassShoup) {
        t.blob = build_ctx_blob(log2n, ht, Arith::kFold);
        t.tb = ctx_view<Arith>(t.blob.data(), ctx_layout(log2n, ht.size(), Arith::kFold), ht.size());
    } else class_tables<Arith>(log2n, ht, std::vector<unsigned char>(ht.size(), (unsigned char)class_of<Arith>()).data(), t);
    return 0;
}
template <class Arith>
static int policy_tables(int log2n, u64 q, u64 psi, Tables<Arith>& t) {
    std::vector<HostLimbTables> ht;
    if (int rc = limb_tables(log2n, 1, &q, &psi, ht)) return rc;
    return policy_tables<Arith>(log2n, ht, t);
}
// Forms the library does not ship - a geometry other than LOGE = 4, a ring below N = 256, the halves form on ShoupArith: one limb's tables through the
// shared packing routines (ctx_tables.h pack_table / pack_subtrees), in the sections a context would have.  log_n1 = 1: the halves tables.
template <class Arith>
static int unshipped_tables(int log2n, int loge, int log_n1, u64 q, u64 psi, Tables<Arith>& t) {
    typedef typename Arith::Tw Tw;
    HostLimbTables h;
    if (int rc = build_limb_tables(log2n, q, psi, h)) return rc;
    if (!class_ok<Arith>(q)) return 2000;
    const LimbClass k = class_of<Arith>();
    struct Rest { TwBytes top; InvLast<TwBytes> last; LimbConst lc; };   // what follows the two tables: htop_fwd, last = htop_last, the limb constants
    const size_t tab = ((size_t)1 << log2n) * sizeof(TwBytes);
    t.blob.assign(2 * tab + sizeof(Rest), 0);
    unsigned char* b = t.blob.data();
    if (log_n1) { pack_subtrees(b, h.rp, k, q, log2n, log_n1, loge); pack_subtrees(b + tab, h.irp, k, q, log2n, log_n1, loge); }
    else { pack_table(b, h.rp, k, q, log2n, loge); pack_table(b + tab, h.irp, k, q, log2n, loge); }
    Rest* r = reinterpret_cast<Rest*>(b + 2 * tab);
    *r = Rest{class_tw(k, h.rp[1], q), class_last(k, h.w_last, h.lc.ninv, q), limb_const_of_class(h.lc, k)};
    t.tb.fwd = t.tb.hfwd = reinterpret_cast<const Tw*>(b); t.tb.inv = t.tb.hinv = reinterpret_cast<const Tw*>(b + tab);
    t.tb.htop_fwd = reinterpret_cast<const Tw*>(&r->top);
    t.tb.last = t.tb.htop_last = reinterpret_cast<const InvLast<Tw>*>(&r->last);
    t.tb.lc = &r->lc;
    t.tb.n_sub = t.tb.n_limbs = 1;
    return 0;
}

// Exchanges are run the way the kernels synchronise them: the all-to-all exchange as "all threads write, barrier, all
// threads read"; a wave-local exchange (Geo::exch_wave_local) one WAVE at a time - write then read - in DESCENDING wave
// order, with no barrier, so a word that had to cross waves, or a region that another wave's exchange clobbers, shows up
// as a mismatch against the oracle (emu_check_lds_regions below proves the address sets disjoint as well).
template <class B, int P, int SIDE_W, int SIDE_R, bool FWD>
static void emu_exchange(std::vector<u64>& regs, std::vector<u64>& lds) {
    constexpr int E = B::E, T = B::T;
    auto X = [&](int tid) -> u64(&)[E] { return *reinterpret_cast<u64(*)[E]>(&regs[(size_t)tid * E]); };
    if (!B::G::exch_wave_local(P)) {
        for (int tid = 0; tid < T; ++tid) B::template lds_write<P, SIDE_W, FWD>(tid, X(tid), lds.data());
        for (int tid = 0; tid < T; ++tid) B::template lds_read<P, SIDE_R, FWD>(tid, X(tid), lds.data());
        return;
    }
    for (int w = (T + 63) / 64 - 1; w >= 0; --w) {
        const int t0 = w * 64, t1 = (t0 + 64 < T) ? t0 + 64 : T;
        for (int tid = t0; tid < t1; ++tid) B::template lds_write<P, SIDE_W, FWD>(tid, X(tid), lds.data());
        for (int tid = t0; tid < t1; ++tid) B::template lds_read<P, SIDE_R, FWD>(tid, X(tid), lds.data());
    }
}

template <class B, int P>
struct FwdSteps {
    static void run(std::vector<u64>& regs, std::vector<u64>& lds, const typename B::Tw* tw, const LimbConst& lc) {
        constexpr int E = B::E, T = B::T;
        auto X = [&](int tid) -> u64(&)[E] { return *reinterpret_cast<u64(*)[E]>(&regs[(size_t)tid * E]); };
        for (int tid = 0; tid < T; ++tid) B::template fwd_phase<P>(tid, X(tid), tw, lc);
        if constexpr (P + 1 < B::NPH) {
            emu_exchange<B, P, P, P + 1, true>(regs, lds);
            FwdSteps<B, P + 1>::run(regs, lds, tw, lc);
        }
    }
};

template <class B, int P, int IN>
struct InvSteps {
    static void run(std::vector<u64>& regs, std::vector<u64>& lds, const typename B::Tw* tw, const typename B::Tw& wl,
                    const typename B::Tw& wn, const LimbConst& lc) {
        constexpr int E = B::E, T = B::T;
        auto X = [&](int tid) -> u64(&)[E] { return *reinterpret_cast<u64(*)[E]>(&regs[(size_t)tid * E]); };
        for (int tid = 0; tid < T; ++tid) B::template inv_phase<P, IN>(tid, X(tid), tw, wl, wn, lc);
        if constexpr (P > 0) {
            emu_exchange<B, P - 1, P, P - 1, false>(regs, lds);
            InvSteps<B, P - 1, IN>::run(regs, lds, tw, wl, wn, lc);
        }
    }
};

// The barrier-free protocol rests on address-set facts; check them exhaustively for one geometry.  For every exchange X
// (forward and inverse direction) let W(X, w) / R(X, w) be the LDS words wave w writes / reads.  Returns 0 when
//   (1) wave-local X:  R(X, w) is a subset of W(X, w), and W(X, w) lies inside wave w's region [w S, (w+1) S)  (S = kWaveStride);
//   (2) the all-to-all exchange, forward direction: every wave READS only its own region (so later wave-local writes need no
//       barrier), inverse direction: every wave WRITES only its own region (so no barrier is needed before it);
//   (3) every address map is injective and inside the buffer.
// A negative return value names the failed check.
template <class B, int P>
static int check_exchanges() {
    constexpr int E = B::E, T = B::T, S = B::G::kWaveStride, W = B::G::kWaves;
    const int words = B::G::lds_words();
    for (int fwd = 0; fwd < 2; ++fwd) {
        std::vector<int> owner_w(words, -1), seen(words, 0);
        // write side / read side register mappings of exchange P in this direction
        for (int pass = 0; pass < 2; ++pass) {   // 0: writes, 1: reads
            std::fill(seen.begin(), seen.end(), 0);
            for (int tid = 0; tid < T; ++tid) {
                const int w = tid / 64;
                for (int k = 0; k < E; ++k) {
                    int a;
                    if (fwd) a = pass == 0 ? B::template xaddr<P, P, true>(tid, k) : B::template xaddr<P, P + 1, true>(tid, k);
                    else a = pass == 0 ? B::template xaddr<P, P + 1, false>(tid, k) : B::template xaddr<P, P, false>(tid, k);
                    if (a < 0 || a >= words) return -3;
                    if (seen[a]++) return -3;                       // injective
                    const bool own = a >= w * S && a < (w + 1) * S;
                    if (B::G::exch_wave_local(P)) {
                        if (!own) return -1;
                        if (pass == 0) owner_w[a] = w; else if (owner_w[a] != w) return -1;
                    } else {
                        // forward: the LAST cross-wave exchange is read inside the own region (the wave-local exchanges that follow
                        // need no barrier); inverse: the FIRST one met (highest index) is written inside the own region
                        if (fwd && pass == 1 && !own && P == B::G::highest_cross_wave_exchange()) return -2;
                        if (!fwd && pass == 0 && !own && P == B::G::highest_cross_wave_exchange()) return -2;
                        if (pass == 0) owner_w[a] = w; else if (owner_w[a] < 0) return -3;   // every word read was written
                    }
                }
            }
        }
    }
    (void)W;
    if constexpr (P + 2 < B::NPH) return check_exchanges<B, P + 1>();
    return 0;
}
template <int LOGN, int LOGE>
static int check_geo() {
    typedef NttBody<FoldArith, LOGN, LOGE> B;
    if constexpr (B::NPH >= 2) {
        // cross-wave exchanges come first (forward order): everything after the last of them stays inside a wave
        for (int p = 0; p + 1 < B::NPH; ++p) if (!B::G::exch_wave_local(p) && p > B::G::highest_cross_wave_exchange()) return -4;
        // the kLdsIO rows of a wave lie in its region
        for (int tid = 0; tid < B::T; ++tid) {
            const int r = B::G::lds_row(tid), w = tid / 64;
            if (r < w * B::G::kWaveStride || r + B::E + 2 > (w + 1) * B::G::kWaveStride) return -5;
        }
        return check_exchanges<B, 0>();
    }
    return 0;
}

// ---- one workgroup's transforms --------------------------------------------------------------------------------------
template <class B> static u64 (&regs_of(std::vector<u64>& r, int tid))[B::E] { return *reinterpret_cast<u64(*)[B::E]>(&r[(size_t)tid * B::E]); }
// forward chain of body B on table `tw` from coefficients `in` (in == out is fine: every word is loaded before the first store)
template <class B>
static void block_fwd(const typename B::Tw* tw, const LimbConst& lc, const u64* in, u64* out) {
    std::vector<u64> regs((size_t)B::T * B::E), lds(B::G::lds_words(), 0xDEADBEEFDEADBEEFull);
    for (int tid = 0; tid < B::T; ++tid) B::load_top(tid, regs_of<B>(regs, tid), in);
    FwdSteps<B, 0>::run(regs, lds, tw, lc);
    for (int tid = 0; tid < B::T; ++tid) { B::fwd_canon(regs_of<B>(regs, tid), lc); B::store_bot(tid, regs_of<B>(regs, tid), out); }
}
template <class B>
static void block_inv(const typename B::Tw* tw, const InvLast<typename B::Tw>& last, const LimbConst& lc, const u64* in, u64* out) {
    std::vector<u64> regs((size_t)B::T * B::E), lds(B::G::lds_words(), 0xDEADBEEFDEADBEEFull);
    for (int tid = 0; tid < B::T; ++tid) B::load_bot(tid, regs_of<B>(regs, tid), in);
    InvSteps<B, B::NPH - 1, kUnit>::run(regs, lds, tw, last.w_last, last.w_ninv, lc);
    for (int tid = 0; tid < B::T; ++tid) { B::inv_canon(regs_of<B>(regs, tid), lc); B::store_top(tid, regs_of<B>(regs, tid), out); }
}
// kernels.h ntt_fwd_kernel / ntt_inv_kernel for block `sub` of a polynomial of limb `limb`
template <class Arith, int LOGN, int LOGE>
static void emu_ntt_block(const DevTables<Arith>& tb, int limb, int sub, int inverse, const u64* in, u64* out) {
    typedef NttBody<Arith, LOGN, LOGE> B;
    const size_t slot = (size_t)limb * tb.n_sub + sub;
    if (!inverse) block_fwd<B>(tb.fwd + slot * B::G::N, tb.lc[limb], in, out);
    else block_inv<B>(tb.inv + slot * B::G::N, tb.last[slot], tb.lc[limb], in, out);
}

// Split transform (N = 2^15, 2^16) as launch_impl.h launch_ntt_split runs it: ntt_top.h column stages (ntt_top_kernel) + N1 4096-point kernels on the
// context's sub-tree tables.
template <class Arith, int LOG_N1>
static void emu_split(const DevTables<Arith>& tb, int limb, int inverse, const u64* in, u64* out) {
    constexpr int LN2 = kSplitLog2N2, N1 = 1 << LOG_N1, N2 = 1 << LN2;
    const LimbConst lc = tb.lc[limb];
    auto columns = [&](const u64* src) {
        for (size_t c = 0; c < (size_t)N2; ++c) {
            u64 x[N1];
            for (int r = 0; r < N1; ++r) x[r] = src[(size_t)r * N2 + c];
            if (!inverse) top_forward<Arith, LOG_N1>(x, tb.top_fwd + (size_t)limb * N1, lc);
            else top_inverse<Arith, LOG_N1>(x, tb.top_inv + (size_t)limb * N1, tb.top_last[limb], lc);
            for (int r = 0; r < N1; ++r) out[(size_t)r * N2 + c] = x[r];
        }
    };
    auto blocks = [&](const u64* src) { for (int r = 0; r < N1; ++r) emu_ntt_block<Arith, LN2, 4>(tb, limb, r, inverse, src + (size_t)r * N2, out + (size_t)r * N2); };
    if (!inverse) { columns(in); blocks(out); } else { blocks(in); columns(out); }
}

// launch.h launch_ntt for a small batch: the one-piece kernel of the ring degree, the split transform from N = 2^15 (FoldArith / ShoupArith)
template <class Arith>
static int emu_launch_ntt(int log2n, const DevTables<Arith>& tb, int limb, int inverse, const u64* in, u64* out) {
#define CASE(LN) if (log2n == LN) { emu_ntt_block<Arith, LN, 4>(tb, limb, 0, inverse, in, out); return 0; }
    CASE(8) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14)
#undef CASE
    if constexpr (class_of<Arith>() == kClassFold || class_of<Arith>() == kClassShoup) {
        if (log2n == 15) { emu_split<Arith, 3>(tb, limb, inverse, in, out); return 0; }
        if (log2n == 16) { emu_split<Arith, 4>(tb, limb, inverse, in, out); return 0; }
    }
    return -1;
}

// N = 8192 as a column stage in registers + two 4096-point sub-transforms through ONE LDS buffer (ntt_halves.h; kernels_halves.h runs exactly these steps
// on the device): 256 emulated threads hold lo / hi, the sub-transforms run on the context's halves tables (sub-trees rooted at nodes 2 and 3).
template <class Arith>
static void emu_halves(const DevTables<Arith>& tb, int limb, int inverse, const u64* in, u64* out) {
    typedef Halves13<Arith> H;
    typedef typename H::B B;
    constexpr int T = B::T, N = H::N, N2 = H::N2;
    const LimbConst lc = tb.lc[limb];
    std::vector<u64> r[2], lds(B::G::lds_words(), 0xDEADBEEFDEADBEEFull);   // lo, hi
    for (auto& v : r) v.assign((size_t)T * B::E, 0);
    auto X = [](std::vector<u64>& v, int tid) -> u64(&)[B::E] { return regs_of<B>(v, tid); };
    if (!inverse) {
        const typename B::Tw* tw = tb.hfwd + (size_t)limb * N;     // [limb][half][N2]
        const typename B::Tw wtop = tb.htop_fwd[limb];
        for (int tid = 0; tid < T; ++tid) { B::load_top(tid, X(r[0], tid), in); B::load_top(tid, X(r[1], tid), in + N2); H::fwd_column(X(r[0], tid), X(r[1], tid), wtop, lc); }
        for (int i = 0; i < 2; ++i) {
            FwdSteps<B, 0>::run(r[i], lds, tw + (size_t)i * N2, lc);
            for (int tid = 0; tid < T; ++tid) { B::fwd_canon(X(r[i], tid), lc); B::store_bot(tid, X(r[i], tid), out + (size_t)i * N2); }
        }
    } else {
        const typename B::Tw* tw = tb.hinv + (size_t)limb * N;
        const InvLast<typename B::Tw> last = tb.htop_last[limb];
        for (int i = 0; i < 2; ++i) {
            for (int tid = 0; tid < T; ++tid) B::load_bot(tid, X(r[i], tid), in + (size_t)i * N2);
            InvSteps<B, B::NPH - 1, kUnit>::run(r[i], lds, tw + (size_t)i * N2, last.w_last, last.w_ninv, lc);
        }
        for (int tid = 0; tid < T; ++tid) {
            H::inv_column(X(r[0], tid), X(r[1], tid), last, lc);
            for (int i = 0; i < 2; ++i) { B::inv_canon(X(r[i], tid), lc); B::store_top(tid, X(r[i], tid), out + (size_t)i * N2); }
        }
    }
}
// N = 16384 as two column stages in registers + four 4096-point sub-transforms through ONE LDS buffer (ntt_quarters.h; kernels_quarters.h runs exactly these
// steps on the device): 256 emulated threads hold q0..q3, the sub-transforms run on the context's quarters tables (sub-trees rooted at nodes 4..7).  FoldArith.
static void emu_quarters(const DevTables<FoldArith>& tb, int limb, int inverse, const u64* in, u64* out) {
    typedef Quarters14 Q;
    typedef Q::B B;
    constexpr int T = B::T, N = Q::N, N2 = Q::N2;
    const LimbConst lc = tb.lc[limb];
    std::vector<u64> r[4], lds(B::G::lds_words(), 0xDEADBEEFDEADBEEFull);
    for (auto& v : r) v.assign((size_t)T * B::E, 0);
    auto X = [](std::vector<u64>& v, int tid) -> u64(&)[B::E] { return regs_of<B>(v, tid); };
    if (!inverse) {
        const TwFold* tw = tb.qfwd + (size_t)limb * N;     // [limb][quarter][N2]
        const QuartersTop top = tb.qtop_fwd[limb];
        for (int tid = 0; tid < T; ++tid) {
            for (int i = 0; i < 4; ++i) B::load_top(tid, X(r[i], tid), in + (size_t)i * N2);
            Q::fwd_columns(X(r[0], tid), X(r[1], tid), X(r[2], tid), X(r[3], tid), top, lc);
        }
        for (int i = 0; i < 4; ++i) {
            FwdSteps<B, 0>::run(r[i], lds, tw + (size_t)i * N2, lc);
            for (int tid = 0; tid < T; ++tid) { B::fwd_canon(X(r[i], tid), lc); B::store_bot(tid, X(r[i], tid), out + (size_t)i * N2); }
        }
    } else {
        const TwFold* tw = tb.qinv + (size_t)limb * N;
        const InvLast<TwFold> last = tb.qtop_last[limb];
        const TwFold wi2 = tb.qtop_inv[2 * limb], wi3 = tb.qtop_inv[2 * limb + 1];
        for (int i = 0; i < 4; ++i) {
            for (int tid = 0; tid < T; ++tid) B::load_bot(tid, X(r[i], tid), in + (size_t)i * N2);
            InvSteps<B, B::NPH - 1, kUnit>::run(r[i], lds, tw + (size_t)i * N2, last.w_last, last.w_ninv, lc);
        }
        for (int tid = 0; tid < T; ++tid) {
            Q::inv_columns(X(r[0], tid), X(r[1], tid), X(r[2], tid), X(r[3], tid), wi2, wi3, last, lc);
            for (int i = 0; i < 4; ++i) { B::inv_canon(X(r[i], tid), lc); B::store_top(tid, X(r[i], tid), out + (size_t)i * N2); }
        }
    }
}

// ---- a whole context ---------------------------------------------------------------------------------------------------
// What dpfhe_ctx_create decides for (log2n, moduli, psi) - fold or generic, per-limb classes or not - through the calls it makes.
struct CtxChoice { std::vector<HostLimbTables> ht; bool fold = true, classes = false; unsigned char limb_cls[16] = {}; };
static int ctx_choice(int log2n, int n_limbs, const u64* moduli, const u64* psi, CtxChoice& c) {
    if (log2n < 8 || log2n > kMaxLog2N || n_limbs < 1 || n_limbs > 1024) return 2000;
    if (int rc = limb_tables(log2n, n_limbs, moduli, psi, c.ht)) return rc;
    for (int l = 0; l < n_limbs; ++l) { if (!h_is_prime(moduli[l])) return 2000; c.fold = c.fold && fold_eligible(moduli[l]); }
    c.classes = ctx_limb_classes(log2n, c.ht, c.fold, c.limb_cls);
    return 0;
}
// One polynomial of limb `limb` through a transform of a context of n_limbs limbs.  form 0: what the library launches for a small batch (one-piece, or
// split from N = 2^15; on the limb's own class when the context has classes); 1: the halves form; 2: the quarters form (2000 where the context has no such
// tables); 3: form 0 on the GENERIC context-wide tables, as a context with one non-fold limb holds them for every limb.
enum { kFormLaunch = 0, kFormHalves = 1, kFormQuarters = 2, kFormGeneric = 3 };
extern "C" int emu_ctx_ntt(int log2n, int n_limbs, const u64* moduli, const u64* psi, int limb, int form, int inverse, const u64* in, u64* out) {
    CtxChoice c;
    if (int rc = ctx_choice(log2n, n_limbs, moduli, psi, c)) return rc;
    if (limb < 0 || limb >= n_limbs || form < kFormLaunch || form > kFormGeneric) return 2000;
    if (form == kFormLaunch && c.classes)
        return with_arith(c.limb_cls[limb], [&](auto a) {
            Tables<decltype(a)> t;
            class_tables(log2n, c.ht, c.limb_cls, t);
            return emu_launch_ntt(log2n, t.tb, limb, inverse, in, out);
        });
    if (form == kFormGeneric || (form == kFormLaunch && !c.fold)) {
        Tables<ShoupArith> t;
        if (int rc = policy_tables(log2n, c.ht, t)) return rc;
        return emu_launch_ntt(log2n, t.tb, limb, inverse, in, out);
    }
    Tables<FoldArith> t;
    if (int rc = policy_tables(log2n, c.ht, t)) return rc;   // (2000: halves / quarters of a context that is not all-fold)
    if (form == kFormLaunch) return emu_launch_ntt(log2n, t.tb, limb, inverse, in, out);
    if (form == kFormHalves ? !t.tb.hfwd : !t.tb.qfwd) return 2000;
    if (form == kFormHalves) emu_halves(t.tb, limb, inverse, in, out); else emu_quarters(t.tb, limb, inverse, in, out);
    return 0;
}
// out = sigma_g(INTT(in)) at N = 2^15, 2^16 as launch_impl.h launch_ntt_inv_galois_split runs it: kernels.h ntt_inv_galois_sub_kernel's per-thread code for every
// sub-block (galois_sub_block -> gather_plan -> stage_load / stage_write / gather_read through the wave's LDS rows, one wave at a time: the rows are
// wave-private), then ntt_top.h's column stages.  -7: a staged load would leave the source sub-block, or a wave's threads disagree on their source region
// (the kernel takes it from its first lane).
template <class Arith, int LOG_N1>
static int emu_split_inv_galois(const DevTables<Arith>& tb, int limb, unsigned g, const u64* in, u64* out) {
    typedef NttBody<Arith, kSplitLog2N2, 4> B;
    constexpr int N1 = 1 << LOG_N1, N2 = B::G::N, T = B::T, E = B::E;
    static_assert(B::kLdsIO, "the kernel's gather path");
    const LimbConst lc = tb.lc[limb];
    std::vector<u64> mid((size_t)N1 * N2);
    for (int b = 0; b < N1; ++b) {
        const GaloisSub gs = galois_sub_block<LOG_N1>(g, (unsigned)b, kSplitLog2N2);
        if (gs.block >= (unsigned)N1) return -7;
        const size_t slot = (size_t)limb * N1 + (size_t)b;
        const u64* src = in + (size_t)gs.block * N2;
        std::vector<u64> regs((size_t)T * E), lds(B::G::lds_words(), 0xDEADBEEFDEADBEEFull);
        std::vector<unsigned> addr((size_t)T * E);
        auto A = [&](int tid) -> unsigned(&)[E] { return *reinterpret_cast<unsigned(*)[E]>(&addr[(size_t)tid * E]); };
        for (int w = T / 64 - 1; w >= 0; --w) {
            long shift0 = 0;
            for (int tid = w * 64; tid < (w + 1) * 64; ++tid) {
                const long shift = B::gather_plan(tid, g, gs.h, A(tid));
                if (tid == w * 64) shift0 = shift;
                const long first = (long)w * 64 * E + shift;   // the wave's staged words: [first, first + 64 E) of the source sub-block
                if (shift != shift0 || first < 0 || first + 64 * E > N2) return -7;
                u64 v[E];
                B::stage_load(tid, v, src + shift);
                B::stage_write(tid, v, lds.data());
            }
            for (int tid = w * 64; tid < (w + 1) * 64; ++tid) B::gather_read(regs_of<B>(regs, tid), lds.data(), A(tid));
        }
        const InvLast<typename B::Tw> last = tb.last[slot];
        InvSteps<B, B::NPH - 1, kUnit>::run(regs, lds, tb.inv + slot * N2, last.w_last, last.w_ninv, lc);
        for (int tid = 0; tid < T; ++tid) { B::inv_canon(regs_of<B>(regs, tid), lc); B::store_top(tid, regs_of<B>(regs, tid), mid.data() + (size_t)b * N2); }
    }
    for (size_t c = 0; c < (size_t)N2; ++c) {
        u64 x[N1];
        for (int r = 0; r < N1; ++r) x[r] = mid[(size_t)r * N2 + c];
        top_inverse<Arith, LOG_N1>(x, tb.top_inv + (size_t)limb * N1, tb.top_last[limb], lc);
        for (int r = 0; r < N1; ++r) out[(size_t)r * N2 + c] = x[r];
    }
    return 0;
}
// One polynomial of limb `limb` of a context of n_limbs limbs through dpfhe_ntt_inv_galois at log2n = 15, 16.  form kFormLaunch: the context's own
// tables (fold or generic); kFormGeneric: the generic tables whatever the primes.  g odd, < 2N.  in != out.
extern "C" int emu_ctx_ntt_inv_galois(int log2n, int n_limbs, const u64* moduli, const u64* psi, int limb, int form, unsigned g, const u64* in, u64* out) {
    CtxChoice c;
    if (int rc = ctx_choice(log2n, n_limbs, moduli, psi, c)) return rc;
    if (limb < 0 || limb >= n_limbs || (form != kFormLaunch && form != kFormGeneric) || !(g & 1u) || g >= (2u << log2n) || in == out) return 2000;
    if (log2n != 15 && log2n != 16) return -1;
    auto run = [&](auto a) {
        Tables<decltype(a)> t;
        if (int rc = policy_tables(log2n, c.ht, t)) return rc;
        return log2n == 15 ? emu_split_inv_galois<decltype(a), 3>(t.tb, limb, g, in, out) : emu_split_inv_galois<decltype(a), 4>(t.tb, limb, g, in, out);
    };
    if (form == kFormGeneric || !c.fold) return run(ShoupArith{});
    return run(FoldArith{});
}
// ---- the Galois gather alone: which word does every output position read? ------------------------------------------------------------------------------
// The kernels' own gather_plan / stage_load / stage_write / gather_read on the words in[i] = first + i of one N-word block, wave by wave as above (the
// kernel stages from its FIRST lane's region), with no transform behind them: out[p] = the word position p receives.  -7: a wave's staged range leaves
// [0, N) of the block, its lanes disagree on the shift, or an LDS address leaves the workgroup's rows.
template <class B>
static int emu_gather_block(unsigned g, unsigned h, u64 first, long long* out) {
    constexpr int N = B::G::N, T = B::T, E = B::E;
    static_assert(B::kLdsIO, "the kernels' gather path");
    std::vector<u64> in((size_t)N), lds(B::G::lds_words(), 0xDEADBEEFDEADBEEFull);
    for (int i = 0; i < N; ++i) in[(size_t)i] = first + (u64)i;
    std::vector<unsigned> addr((size_t)64 * E);
    auto A = [&](int lane) -> unsigned(&)[E] { return *reinterpret_cast<unsigned(*)[E]>(&addr[(size_t)lane * E]); };
    for (int w = T / 64 - 1; w >= 0; --w) {
        long shift0 = 0;
        for (int tid = w * 64; tid < (w + 1) * 64; ++tid) {
            const long shift = B::gather_plan(tid, g, h, A(tid & 63));
            if (tid == w * 64) shift0 = shift;
            const long lo = (long)w * 64 * E + shift;
            if (shift != shift0 || lo < 0 || lo + 64 * E > N) return -7;
            for (int k = 0; k < E; ++k) if (A(tid & 63)[k] >= (unsigned)B::G::lds_words()) return -7;
            u64 v[E];
            B::stage_load(tid, v, in.data() + shift0);
            B::stage_write(tid, v, lds.data());
        }
        for (int tid = w * 64; tid < (w + 1) * 64; ++tid) {
            u64 x[E];
            B::gather_read(x, lds.data(), A(tid & 63));
            for (int k = 0; k < E; ++k) out[(size_t)tid * E + k] = (long long)x[k];
        }
    }
    return 0;
}
// kernels.h ntt_inv_galois_kernel's gather at N = 1024 ... 16384: h = (g - 1) / 2.  out[p], p < N: the source position.  -1: no such kernel.
extern "C" int emu_gather_map(int log2n, unsigned g, long long* out) {
    const unsigned h = (g - 1u) >> 1;
    switch (log2n) {
        case 10: return emu_gather_block<NttBody<FoldArith, 10, kLoge>>(g, h, 0, out);
        case 11: return emu_gather_block<NttBody<FoldArith, 11, kLoge>>(g, h, 0, out);
        case 12: return emu_gather_block<NttBody<FoldArith, 12, kLoge>>(g, h, 0, out);
        case 13: return emu_gather_block<NttBody<FoldArith, 13, kLoge>>(g, h, 0, out);
        case 14: return emu_gather_block<NttBody<FoldArith, 14, kLoge>>(g, h, 0, out);
        default: return -1;
    }
}
// kernels.h ntt_inv_galois_sub_kernel's gather at N = 32768, 65536: sub-block b reads sub-block blocks[b] (galois_sub_block) with that block's h.
// out[b N2 + k] = blocks[b] N2 + the index read inside it.
template <int LOG_N1>
static int emu_gather_split(unsigned g, long long* out, long long* blocks) {
    typedef NttBody<FoldArith, kSplitLog2N2, 4> B;
    for (unsigned b = 0; b < (1u << LOG_N1); ++b) {
        const GaloisSub gs = galois_sub_block<LOG_N1>(g, b, kSplitLog2N2);
        blocks[b] = (long long)gs.block;
        if (gs.block >= (1u << LOG_N1)) return -7;
        if (int rc = emu_gather_block<B>(g, gs.h, (u64)gs.block * B::G::N, out + (size_t)b * B::G::N)) return rc;
    }
    return 0;
}
extern "C" int emu_gather_map_split(int log2n, unsigned g, long long* out, long long* blocks) {
    if (log2n == 15) return emu_gather_split<3>(g, out, blocks);
    if (log2n == 16) return emu_gather_split<4>(g, out, blocks);
    return -1;
}

// The bytes dpfhe_ctx_create would upload: which = 0 the context-wide blob, 1 the class blob, 2 the lazy-multiply blob (log2 N = 12 with a fold limb).  Returns the size (0: the context has no class blob), or
// -2000 for parameters a context rejects; copies the bytes when out holds at least that many, and the LimbClass per limb into limb_cls (n_limbs <= 16).
extern "C" long emu_ctx_blob(int log2n, int n_limbs, const u64* moduli, const u64* psi, int which, unsigned char* out, size_t cap, unsigned char* limb_cls) {
    CtxChoice c;
    if (ctx_choice(log2n, n_limbs, moduli, psi, c)) return -2000;
    std::vector<unsigned char> blob;
    if (!which) blob = build_ctx_blob(log2n, c.ht, c.fold);
    else if (which == 1) { if (c.classes) blob = build_class_blob(log2n, c.ht, c.limb_cls); }
    else {   // 2: the lazy-multiply blob, as dpfhe_ctx_create calls for it
        std::vector<bool> fold_limb((size_t)n_limbs);
        for (int l = 0; l < n_limbs; ++l) fold_limb[(size_t)l] = c.fold || (c.classes && c.limb_cls[l] == kClassFold);
        blob = build_lazy29_blob(log2n, c.ht, fold_limb);
    }
    if (limb_cls && n_limbs <= 16) std::memcpy(limb_cls, c.limb_cls, (size_t)n_limbs);
    if (out && cap >= blob.size()) std::memcpy(out, blob.data(), blob.size());
    return (long)blob.size();
}

// ---- the single-prime entry points: a context of one limb, on the policy the caller names ----------------------------------
// arith: 0 Shoup, 1 Fold, 2 F64, 3 FoldScaled, 4 F64Wide (tables.h LimbClass).  `in`/`out` must be 16-byte aligned.  returns 0, 2000 bad args, -1 unsupported geometry
extern "C" int emu_ntt(int arith, int log2n, int loge, int inverse, u64 q, u64 psi, const u64* in, u64* out) {
    return with_arith(arith, [&](auto a) {
        typedef decltype(a) Arith;
        Tables<Arith> t;
        if (log2n >= 8 && log2n <= 14 && log2n != 9 && loge == kLoge) {
            if (int rc = policy_tables<Arith>(log2n, q, psi, t)) return rc;
            return emu_launch_ntt<Arith>(log2n, t.tb, 0, inverse, in, out);
        }
#define CASE(LN, LE)                                                                 \
        if (log2n == LN && loge == LE) {                                             \
            if (int rc = unshipped_tables<Arith>(LN, LE, 0, q, psi, t)) return rc;   \
            emu_ntt_block<Arith, LN, LE>(t.tb, 0, 0, inverse, in, out);              \
            return 0;                                                                \
        }
        CASE(13, 5) CASE(14, 5) CASE(12, 3) CASE(12, 5) CASE(6, 3)
#undef CASE
        return -1;
    });
}
// (a fold prime alone is an all-fold context; arith = 0 runs it on the generic tables)
extern "C" int emu_ntt_split(int arith, int log2n, int inverse, u64 q, u64 psi, const u64* in, u64* out) {
    if (log2n != 15 && log2n != 16) return -1;
    if (arith && !fold_eligible(q)) return 2000;
    return emu_ctx_ntt(log2n, 1, &q, &psi, 0, arith ? kFormLaunch : kFormGeneric, inverse, in, out);
}
// the halves form ships for FoldArith contexts only: ShoupArith runs it on tables packed here
extern "C" int emu_ntt_halves(int arith, int inverse, u64 q, u64 psi, const u64* in, u64* out) {
    if (arith) return emu_ctx_ntt(13, 1, &q, &psi, 0, kFormHalves, inverse, in, out);
    Tables<ShoupArith> t;
    if (int rc = unshipped_tables(13, 4, 1, q, psi, t)) return rc;
    emu_halves(t.tb, 0, inverse, in, out);
    return 0;
}
extern "C" int emu_ntt_quarters(int inverse, u64 q, u64 psi, const u64* in, u64* out) { return emu_ctx_ntt(14, 1, &q, &psi, 0, kFormQuarters, inverse, in, out); }

// Forward transform of words that are only known to be below 2^60 (the digits of a key switch are canonical for ANOTHER limb): NttBody's
// FWD_IN = kRedB plans, which relin_kernel / relin_shared_kernel rely on to skip the canonicalisation.  FoldArith only.
extern "C" int emu_ntt_fwd_any60(int log2n, u64 q, u64 psi, const u64* in, u64* out) {
    Tables<FoldArith> t;
    if (int rc = policy_tables(log2n, q, psi, t)) return rc;
#define CASE(LN) if (log2n == LN) { block_fwd<NttBody<FoldArith, LN, kLoge, 0, kRedB>>(t.tb.fwd, t.tb.lc[0], in, out); return 0; }
    CASE(8) CASE(10) CASE(12) CASE(13)
#undef CASE
    return -1;
}

// ---- the fused multiply -------------------------------------------------------------------------------------------------
// One limb's (c0, c1, c2) through the fused ct x ct kernels' data paths (coefficient domain in and out), with the same per-thread transform code and the
// same dyadic sequence, on the context's tables (DevTables::fwd / inv).
//   LAZY (kernels.h ct_mul_quad_kernel / ct_mul_dual_kernel - the paired kernel computes the same values, two transforms at a time): lazy forward outputs,
//     NttBody::tensor (fold policies turn b0, b1 into twiddles on the fly), the inverse of register-resident products - so the bound plans and the relaxed
//     mul60 precondition (lazy forward outputs < 14 q times partially reduced b-side factors) are checked with the wrap-around / precondition counters armed;
//   otherwise (ct_mul_kernel, any policy): four forward transforms to canonical words, Arith::mul_var products, three inverse transforms.
//   LAZY29 (ct_mul_quad_kernel at N = 4096 on the pinned primes): the same with NttBody's LAZY29 plans on the context's bit-29 tables (ctx_tables.h
//     build_lazy29_blob); out_ntt: the products as DPFHE_OUT_NTT stores them (canonical, forward-output order), no inverse transforms.
template <class Arith, int LOGN, bool LAZY, bool LAZY29 = false>
static int emu_ct_mul_path(u64 q, u64 psi, const u64* a0, const u64* a1, const u64* b0, const u64* b1, u64* out3, bool out_ntt = false) {
    typedef NttBody<Arith, LOGN, kLoge, 0, kUnit, false, LAZY29> B;
    typedef NttBody<Arith, LOGN, kLoge, 0, kUnit, LAZY, LAZY29> BI;
    Tables<Arith> t;
    if (int rc = policy_tables(LOGN, q, psi, t)) return rc;
    constexpr int T = B::T, N = B::G::N, limb = 0;
    static_assert(!LAZY || !Arith::kFoldCore || B::kFwdOutBound <= (LAZY29 ? kWord : kLimitPartner), "lazy forward outputs must satisfy mul60's bound");
    // FoldScaledArith: lazy products carry the scale twice; the inverse's last stage folds one s^-1 in (DevTables::last2)
    constexpr bool kScaledProducts = LAZY && Arith::kFoldCore && !Arith::kFold;
    const LimbConst lc = t.tb.lc[limb];
    std::vector<unsigned char> blob29;
    if constexpr (LAZY29) {
        std::vector<HostLimbTables> ht;
        if (int rc = limb_tables(LOGN, 1, &q, &psi, ht)) return rc;
        blob29 = build_lazy29_blob(LOGN, ht, std::vector<bool>(1, true));
        if (blob29.empty()) return -1;
        lazy29_view(t.tb, blob29.data(), lazy29_layout(1));
    }
    const InvLast<typename B::Tw> last = LAZY29 ? t.tb.last29[limb] : kScaledProducts ? t.tb.last2[limb] : t.tb.last[limb];
    const typename B::Tw *twf = (LAZY29 ? t.tb.fwd29 : t.tb.fwd) + (size_t)limb * N, *twi = (LAZY29 ? t.tb.inv29 : t.tb.inv) + (size_t)limb * N;
    std::vector<u64> lds(B::G::lds_words());
    auto fwd = [&](const u64* src, bool partner) {
        std::vector<u64> regs((size_t)T * B::E);
        for (int tid = 0; tid < T; ++tid) B::load_top(tid, regs_of<B>(regs, tid), src);
        FwdSteps<B, 0>::run(regs, lds, twf, lc);
        for (int tid = 0; tid < T; ++tid) {
            if constexpr (!LAZY) B::fwd_canon(regs_of<B>(regs, tid), lc);
            else if (partner) B::prod_partner(regs_of<B>(regs, tid), lc);
        }
        return regs;
    };
    auto inv = [&](std::vector<u64> regs, u64* dst) {
        InvSteps<BI, B::NPH - 1, LAZY ? B::kProdInvIn : kUnit>::run(regs, lds, twi, last.w_last, last.w_ninv, lc);
        for (int tid = 0; tid < T; ++tid) { B::inv_canon(regs_of<B>(regs, tid), lc); B::store_top(tid, regs_of<B>(regs, tid), dst); }
    };
    std::vector<u64> S0 = fwd(a0, false), S1 = fwd(b0, true), S2 = fwd(b1, true), S3 = fwd(a1, false), c0((size_t)N), c1((size_t)N), c2((size_t)N);
    for (int i = 0; i < N; ++i) {
        if constexpr (LAZY) B::tensor(S0[i], S3[i], S1[i], S2[i], c0[i], c1[i], c2[i], lc);
        else { c0[i] = Arith::mul_var(S0[i], S1[i], lc); c1[i] = add_mod(Arith::mul_var(S0[i], S2[i], lc), Arith::mul_var(S3[i], S1[i], lc), lc.q); c2[i] = Arith::mul_var(S3[i], S2[i], lc); }
    }
    if (out_ntt) {
        if constexpr (LAZY && Arith::kFold) {
            std::vector<u64>* c[3] = {&c0, &c1, &c2};
            for (int j = 0; j < 3; ++j)
                for (int tid = 0; tid < T; ++tid) {
                    u64(&r)[B::E] = regs_of<B>(*c[j], tid);
                    for (int k = 0; k < B::E; ++k) r[k] = FoldArith::canon_small(r[k], lc);
                    B::store_bot(tid, r, out3 + (size_t)j * N);
                }
            return 0;
        }
        return -1;
    }
    inv(c0, out3);
    inv(c1, out3 + N);
    inv(c2, out3 + 2 * N);
    return 0;
}
// ct_mul_quad_kernel<FoldArith, 12, 4> as shipped: the lazy body on the bit-29 blob, coefficient-domain or NTT-domain output
extern "C" int emu_ct_mul_lazy29(u64 q, u64 psi, int out_ntt, const u64* a0, const u64* a1, const u64* b0, const u64* b1, u64* out3) {
    if (!fold_eligible(q)) return 2000;
    return emu_ct_mul_path<FoldArith, 12, true, true>(q, psi, a0, a1, b0, b1, out3, out_ntt != 0);
}
// FoldArith::mul_tw29_add on the twiddle tables.h makes of w: the UNREDUCED word, through the very code the kernels run
extern "C" u64 emu_fold_tw29(u64 d, u64 y, u64 w, u64 addend) {
    LimbConst lc{};
    lc.q = (1ull << 60) - d; lc.d = d;
    return FoldArith::mul_tw29_add(y, h_tw_fold29(w, lc.q), lc, addend);
}
// The lazy plans of the N = 4096 geometry, one phase at a time (forward: phase p of the chain; inverse: phase p of the walk back, inputs below in_bound).
// Forward rows [u][k]: red_a, K; inverse rows [u][k]: red, off.  tail[0 .. 16) = red_end, tail[16] = out_bound, tail[17] = n_red, tail[18 .. 34) = out (forward).
extern "C" int emu_lazy29_plan(int inverse, int phase, int in_bound, int* flags, int* consts, int* tail) {
    typedef NttBody<FoldArith, 12, kLoge, 0, kUnit, true, true> B;
    if (phase < 0 || phase >= B::NPH) return 2000;
    const Phase ph = B::G::phase(phase);
    if (!inverse) {
        const Ctf29Plan<4> p = make_ctf29_plan<4>(ph.b - ph.c + ph.r - 1, ph.r, in_bound, phase == B::NPH - 1 ? kWord : kCtf29Mid);
        for (int u = 0; u < 4; ++u) for (int k = 0; k < 16; ++k) { flags[u * 16 + k] = p.red_a[u][k]; consts[u * 16 + k] = p.K[u][k]; }
        for (int k = 0; k < 16; ++k) { tail[k] = p.red_end[k]; tail[18 + k] = p.out[k]; }
        tail[16] = p.out_bound; tail[17] = p.n_red;
    } else {
        const Gs29Plan<4> p = make_gs29_plan<4>(ph.b - ph.c, ph.r, in_bound, phase == 0 ? 3 * kUnit / 2 : kGs29Mid, phase == 0, 12);
        for (int u = 0; u < 4; ++u) for (int k = 0; k < 16; ++k) { flags[u * 16 + k] = p.red[u][k]; consts[u * 16 + k] = p.off[u][k]; }
        for (int k = 0; k < 16; ++k) tail[k] = p.red_end[k];
        tail[16] = p.out_bound; tail[17] = p.n_red;
    }
    return 0;
}
// FoldArith::mul_tw29_add_uniform with the multiple k q on board: the UNREDUCED word (its assertions check the chain and the residue in 128-bit arithmetic)
extern "C" u64 emu_fold_tw29_uniform(u64 d, u64 y, u64 w, u64 k) {
    LimbConst lc{};
    lc.q = (1ull << 60) - d; lc.d = d;
    return FoldArith::mul_tw29_add_uniform(y, h_tw_fold29(w, lc.q), lc, k * lc.q);
}
// Where the inverse butterflies' multiples of q come from (ntt_core.h Gs29Ride, derived from the plan of the same phase and input bound): ride[u][kk] in
// flags[u * 16 + kk]; returns the number of products that carry their next butterfly's multiple, or -2000.
extern "C" int emu_gs29_ride(int phase, int in_bound, int* flags) {
    typedef NttBody<FoldArith, 12, kLoge, 0, kUnit, true, true> B;
    if (phase < 0 || phase >= B::NPH) return -2000;
    const Phase ph = B::G::phase(phase);
    const int cap = phase == 0 ? 3 * kUnit / 2 : kGs29Mid;
    const Gs29Plan<4> p = make_gs29_plan<4>(ph.b - ph.c, ph.r, in_bound, cap, phase == 0, 12);
    const Gs29Ride<4> rd = make_gs29_ride<4>(p, ph.b - ph.c, ph.r, in_bound, cap, phase == 0, 12);
    for (int u = 0; u < 4; ++u) for (int k = 0; k < 16; ++k) flags[u * 16 + k] = rd.ride[u][k];
    return rd.n_ride;
}
// the tables the shipped body compiles in, phase by phase: ride[phase][u][kk] in flags[phase * 64 + u * 16 + kk]; returns their total per transform and thread
extern "C" int emu_gs29_ride_shipped(int* flags) {
    typedef NttBody<FoldArith, 12, kLoge, 0, kUnit, true, true> BI;
    constexpr int IN = BI::kProdInvIn;
    const Gs29Ride<4> rd[3] = {BI::gs29_ride<0, IN>(), BI::gs29_ride<1, IN>(), BI::gs29_ride<2, IN>()};
    int n = 0;
    for (int p = 0; p < 3; ++p) { n += rd[p].n_ride; for (int u = 0; u < 4; ++u) for (int k = 0; k < 16; ++k) flags[p * 64 + u * 16 + k] = rd[p].ride[u][k]; }
    return n;
}
// One thread's lazy inverse phase (NttBody::inv_phase_lazy29, the code the kernel runs) on the caller's 16 words and twiddles, under the shipped plan of
// that phase and either its shipped derived table (ride_flags == nullptr) or the caller's - a multiple folded where the bounds have no room must trip the
// armed assertions.  w[u * 8 + j]: the twiddle (a residue below q) of stage u, butterfly group j; w_last: the last stage's.  q = 2^60 - d, any fold modulus.
template <int P>
static void emu_gs29_phase_p(u64 q, const int* ride_flags, const u64* w, u64 w_last, u64 (&x)[16]) {
    typedef NttBody<FoldArith, 12, kLoge, 0, kUnit, true, true> BI;
    constexpr int IN = BI::kProdInvIn;
    const Gs29Plan<4> plan = BI::gs29_plan<P, IN>();
    Gs29Ride<4> rd = BI::gs29_ride<P, IN>();
    if (ride_flags) for (int u = 0; u < 4; ++u) for (int k = 0; k < 16; ++k) rd.ride[u][k] = ride_flags[u * 16 + k] != 0;
    LimbConst lc{};
    lc.q = q; lc.d = (1ull << 60) - q;
    typename BI::TwRegs twr;
    for (int u = 0; u < 4; ++u) for (int j = 0; j < 8; ++j) twr[u][j] = h_tw_fold29(w[u * 8 + j], q);
    BI::inv_phase_lazy29<P>(x, twr, h_tw_fold29(w_last, q), lc, plan, rd);
}
extern "C" int emu_gs29_phase(int phase, u64 q, const int* ride_flags, const u64* w, u64 w_last, u64* x16) {
    if (!fold_eligible(q) || !(q & 1)) return 2000;
    u64(&x)[16] = *reinterpret_cast<u64(*)[16]>(x16);
    if (phase == 0) emu_gs29_phase_p<0>(q, ride_flags, w, w_last, x);
    else if (phase == 1) emu_gs29_phase_p<1>(q, ride_flags, w, w_last, x);
    else if (phase == 2) emu_gs29_phase_p<2>(q, ride_flags, w, w_last, x);
    else return 2000;
    return 0;
}
// what the shipped body compiles in: reductions per transform and thread, forward and inverse, and the hand-over bounds the phases were planned with
extern "C" void emu_lazy29_totals(int* out) {
    typedef NttBody<FoldArith, 12, kLoge, 0, kUnit, false, true> B;
    typedef NttBody<FoldArith, 12, kLoge, 0, kUnit, true, true> BI;
    out[0] = B::lazy_fwd_reductions<>(); out[1] = BI::lazy_inv_reductions<B::kProdInvIn>();
    out[2] = B::ctf29_plan<0>().out_bound; out[3] = B::ctf29_plan<1>().out_bound; out[4] = B::ctf29_plan<2>().out_bound;
    out[5] = kCtf29Mid; out[6] = kGs29Mid; out[7] = B::kProdInvIn;
}
template <bool LAZY>
static int emu_ct_mul_any(int arith, int log2n, u64 q, u64 psi, const u64* a0, const u64* a1, const u64* b0, const u64* b1, u64* out3) {
    return with_arith(arith, [&](auto a) {
        typedef decltype(a) Arith;
#define CASE(LN) if (log2n == LN) return emu_ct_mul_path<Arith, LN, LAZY>(q, psi, a0, a1, b0, b1, out3);
        if constexpr (LAZY ? Arith::kFoldCore || Arith::kF64 : !Arith::kFold) { CASE(8) CASE(10) CASE(12) CASE(13) }   // (ShoupArith has no lazy products; FoldArith always uses them)
#undef CASE
        return -1;
    });
}
// the generic path of the classes (arith 0 Shoup, 2 F64, 3 FoldScaled, 4 F64Wide), their lazy-product path (1 Fold, 2, 3, 4), and the pinned primes' multiply
extern "C" int emu_ct_mul_class(int arith, int log2n, u64 q, u64 psi, const u64* a0, const u64* a1, const u64* b0, const u64* b1, u64* out3) {
    return emu_ct_mul_any<false>(arith, log2n, q, psi, a0, a1, b0, b1, out3);
}
extern "C" int emu_ct_mul_lazy_class(int arith, int log2n, u64 q, u64 psi, const u64* a0, const u64* a1, const u64* b0, const u64* b1, u64* out3) {
    return emu_ct_mul_any<true>(arith, log2n, q, psi, a0, a1, b0, b1, out3);
}
extern "C" int emu_ct_mul(int log2n, u64 q, u64 psi, const u64* a0, const u64* a1, const u64* b0, const u64* b1, u64* out3) {
    if (log2n == 12) return fold_eligible(q) ? emu_ct_mul_path<FoldArith, 12, true, true>(q, psi, a0, a1, b0, b1, out3) : 2000;   // the quad form's lazy body (emu_ct_mul_lazy_class runs the paired form's)
    return emu_ct_mul_any<true>(kClassFold, log2n, q, psi, a0, a1, b0, b1, out3);
}

extern "C" int emu_check_lds_regions(int log2n, int loge) {
#define CASE(LN, LE) if (log2n == LN && loge == LE) return check_geo<LN, LE>();
    CASE(8, 4) CASE(9, 4) CASE(10, 4) CASE(11, 4) CASE(12, 4) CASE(13, 4) CASE(14, 4) CASE(13, 5) CASE(14, 5) CASE(12, 3) CASE(12, 5)
#undef CASE
    return -100;
}

extern "C" int emu_lds_words(int log2n, int loge) {
    if (log2n == 12 && loge == 4) return Geo<12, 4>::lds_words();
    if (log2n == 13 && loge == 5) return Geo<13, 5>::lds_words();
    if (log2n == 10 && loge == 4) return Geo<10, 4>::lds_words();
    return -1;
}

// FoldArith::prod_tw / mul_ptw_add (variable x variable products through the twiddle chain): addend + y b mod q through the very code the
// kernels run, canonicalised; d is passed so that the scaled-fold moduli (q' = 2^60 - d, not prime) can be checked as well.
extern "C" u64 emu_fold_ptw(u64 d, u64 y, u64 b, u64 addend) {
    LimbConst lc{};
    lc.q = (1ull << 60) - d; lc.d = d;
    return FoldArith::canon(FoldArith::mul_ptw_add(y, FoldArith::prod_tw(b, lc), lc, addend), lc);
}

// FoldArith::dot30_* (the plaintext matvec's column accumulators): dot product of canonical residues through the very code
// the kernel runs (fold every kDot30Period terms, the running word riding in column 0), against 128-bit arithmetic.
extern "C" u64 emu_dot30(u64 q, const u64* a, const u64* b, size_t n) {
    LimbConst lc{};
    lc.q = q; lc.d = (1ull << 60) - q;
    FoldArith::Dot30 acc{0, 0, 0};
    int since = 0;
    for (size_t i = 0; i < n; ++i) {
        FoldArith::dot30_mac(acc, FoldArith::split30(a[i]), FoldArith::split30(b[i]));
        if (++since == FoldArith::kDot30Period) { acc = FoldArith::Dot30{FoldArith::dot30_fold0(acc, lc), 0, 0}; since = 0; }
    }
    return FoldArith::canon_small(since ? FoldArith::dot30_fold0(acc, lc) : acc.s0, lc);
}
