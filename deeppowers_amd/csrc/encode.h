// encode.h - slot encoding over Z_t (include/dpfhe.h "slot encoding"): the inverse negacyclic transform in 32-bit words, then centre and lift.
//
//   t prime, t < 2^32, t = 1 mod 2N; zeta a primitive 2N-th root of unity mod t.  Slot i sits at the position p = brv((e - 1) / 2) of a vector a
//   (e = 3^i mod 2N for row 0, 2N - 3^i for row 1: a[p] = m(zeta^e)), and the message polynomial is the inverse transform of a:
//   Gentleman-Sande butterflies (u, v) -> (u + v, (u - v) w), level `lg` pairing words 2^lg apart with w = zeta^-brv(block) for the block
//   j >> (lg + 1) of its pair, levels lg = 0 ... log2 N - 1, then N^-1 (folded into the last level's two multipliers).
//   Every word stays canonical in [0, t): t may lie one below 2^32, so there is no room for a lazy [0, 2t) representation in 32 bits.  Products are
//   Shoup products with a 32-bit quotient estimate; the remainder x w - floor(x w' / 2^32) t lies in [0, 2t) and is taken in 64 bits, so the
//   arithmetic is exact for every prime below 2^32.
//   Several levels run per pass over the vector: a group of 2^R words 2^lg0 apart is loaded once and goes through R levels in registers.
//
// Shared by the device kernels (k_encode.hip) and the host twin (dpfhe_encode_slots_host): the host walks the groups of a pass one after the other
// through the same functions, so one statement of the arithmetic serves both.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include <vector>

#include "modarith.h"
#include "tables.h"

namespace dpfhe {

constexpr u32 kEncRadixLog = 3;   // levels per pass

struct EncTw {
    u32 w;    // a power of zeta^-1 mod t (or N^-1 times one)
    u32 wq;   // floor(w 2^32 / t)
};

struct EncLimb {
    u64 q;
    u64 mu;   // floor(2^64 / q)
};

// what a launch needs of (N, t): entry m + i of `tw` is zeta^-brv(i) for the 2 m blocks of the level with m pairs of blocks (m a power of two, i < m);
// entry 0 is N^-1 and entry N is N^-1 zeta^-(N/2): the last level's two multipliers.  src[p] is the slot whose value position p holds.
struct EncodeTables {
    const EncTw* tw;      // N + 1 entries
    const u32* src;       // N entries
    const EncLimb* limb;  // n_limbs entries
    u32 t, half;          // half = (t - 1) / 2: a > half means the centred value is a - t
    u32 log2n, n_limbs;
};

DPF_HD u32 enc_add(u32 a, u32 b, u32 t) {
    const u32 s = a + b;
    return (s < a || s >= t) ? s - t : s;   // a wrapped sum is >= 2^32 > t: the subtraction wraps back
}
DPF_HD u32 enc_sub(u32 a, u32 b, u32 t) { return a >= b ? a - b : a - b + t; }
DPF_HD u32 enc_mul(u32 x, EncTw w, u32 t) {
    const u32 q = (u32)(((u64)x * w.wq) >> 32);
    const u64 r = (u64)x * w.w - (u64)q * t;   // in [0, 2t): below 2^33
    return (u32)(r >= t ? r - t : r);
}
DPF_HD EncTw enc_tw(u64 w, u64 t) { return EncTw{(u32)w, (u32)((w << 32) / t)}; }
// a slot value as the transform takes it: values >= t are reduced
DPF_HD u32 enc_slot(u32 v, u32 t) { return v >= t ? v % t : v; }

// R levels lg0 ... lg0 + R - 1 on the 2^R words x[k] = a[j0 + (k << lg0)] of one group; LAST: level lg0 + R - 1 is the transform's last (log2 N - 1)
template <int R, bool LAST>
DPF_HD void enc_group(u32 (&x)[1 << R], u32 j0, u32 lg0, u32 log2n, const EncTw* __restrict__ tw, u32 t) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const u32 lg = lg0 + r;
#pragma unroll
        for (int k = 0; k < (1 << R); ++k) {
            if (k & (1 << r)) continue;
            const u32 u = x[k], v = x[k | (1 << r)];
            if (LAST && r == R - 1) {
                x[k] = enc_mul(enc_add(u, v, t), tw[0], t);
                x[k | (1 << r)] = enc_mul(enc_sub(u, v, t), tw[1u << log2n], t);
            } else {
                const u32 j = j0 + ((u32)k << lg0);
                x[k] = enc_add(u, v, t);
                x[k | (1 << r)] = enc_mul(enc_sub(u, v, t), tw[(1u << (log2n - 1 - lg)) + (j >> (lg + 1))], t);
            }
        }
    }
}

// group g of the pass that starts at level lg0, on a vector in memory (LDS on the device, an array on the host) whose word 0 is position `base`
template <int R, bool LAST>
DPF_HD void enc_group_mem(u32* a, u32 g, u32 base, u32 lg0, u32 log2n, const EncTw* __restrict__ tw, u32 t) {
    const u32 lo = g & ((1u << lg0) - 1u);
    const u32 p0 = ((g >> lg0) << (lg0 + R)) + lo;
    u32 x[1 << R];
#pragma unroll
    for (int k = 0; k < (1 << R); ++k) x[k] = a[p0 + ((u32)k << lg0)];
    enc_group<R, LAST>(x, base + p0, lg0, log2n, tw, t);
#pragma unroll
    for (int k = 0; k < (1 << R); ++k) a[p0 + ((u32)k << lg0)] = x[k];
}


// the centred value of a in [0, t) mod q, canonical: what lift_signed makes of it.  q may be smaller than t.
DPF_HD u64 enc_lift(u32 a, u32 t, u32 half, const EncLimb& l) {
    const bool neg = a > half;
    u64 x = neg ? t - a : a;   // |c|
    if (!(l.q >> 32)) x = csub(x - mulhi64(x, l.mu) * l.q, l.q);   // (a limb of 32 bits or more already exceeds |c|)
    return neg && x ? l.q - x : x;
}

// ---- the lane's steps of the LDS kernel between two barriers: k_encode.hip runs them on the device, tools/emulate_encode.cpp lane by lane on the CPU.
// `a` holds the C = 2^log2c words of the chunk that starts at position `base` (the whole vector when C = N); lane `tid` of T.
#if defined(__HIPCC__)
typedef u32 enc_u32x4 __attribute__((ext_vector_type(4)));
#else
struct alignas(16) enc_u32x4 { u32 x, y, z, w; };
#endif

// levels 0 ... 2 (log2c >= 8: never the last pass) on 8 adjacent words gathered straight from the slot vector v
DPF_HD void enc_lane_first_pass(u32* a, const u32* __restrict__ v, u32 tid, u32 T, u32 base, u32 C, const EncodeTables& tb) {
    for (u32 g = tid; g < (C >> kEncRadixLog); g += T) {
        const u32 p0 = g << kEncRadixLog;
        const enc_u32x4 s0 = *reinterpret_cast<const enc_u32x4*>(tb.src + base + p0), s1 = *reinterpret_cast<const enc_u32x4*>(tb.src + base + p0 + 4);
        u32 x[8] = {enc_slot(v[s0.x], tb.t), enc_slot(v[s0.y], tb.t), enc_slot(v[s0.z], tb.t), enc_slot(v[s0.w], tb.t),
                    enc_slot(v[s1.x], tb.t), enc_slot(v[s1.y], tb.t), enc_slot(v[s1.z], tb.t), enc_slot(v[s1.w], tb.t)};
        enc_group<3, false>(x, base + p0, 0, tb.log2n, tb.tw, tb.t);
        *reinterpret_cast<enc_u32x4*>(a + p0) = enc_u32x4{x[0], x[1], x[2], x[3]};
        *reinterpret_cast<enc_u32x4*>(a + p0 + 4) = enc_u32x4{x[4], x[5], x[6], x[7]};
    }
}
// levels lg0 ... lg0 + 2, not the last pass
DPF_HD void enc_lane_mid_pass(u32* a, u32 tid, u32 T, u32 base, u32 C, u32 lg0, const EncodeTables& tb) {
    for (u32 g = tid; g < (C >> kEncRadixLog); g += T) enc_group_mem<3, false>(a, g, base, lg0, tb.log2n, tb.tw, tb.t);
}
// the chunk's last pass: the 1 ... 3 levels from lg0 to log2c - 1; WHOLE: they end the transform (N^-1 folded in)
template <bool WHOLE>
DPF_HD void enc_lane_last_pass(u32* a, u32 tid, u32 T, u32 base, u32 log2c, u32 lg0, const EncodeTables& tb) {
    const u32 C = 1u << log2c;
    switch (log2c - lg0) {
    case 1: for (u32 g = tid; g < (C >> 1); g += T) enc_group_mem<1, WHOLE>(a, g, base, lg0, tb.log2n, tb.tw, tb.t); break;
    case 2: for (u32 g = tid; g < (C >> 2); g += T) enc_group_mem<2, WHOLE>(a, g, base, lg0, tb.log2n, tb.tw, tb.t); break;
    default: for (u32 g = tid; g < (C >> 3); g += T) enc_group_mem<3, WHOLE>(a, g, base, lg0, tb.log2n, tb.tw, tb.t); break;
    }
}
// coefficients k, k + 1 (k even) of one item: the plain words, or their residues on every limb row (16-byte stores)
DPF_HD void enc_store_pair(u64* item_out, size_t k, u32 a0, u32 a1, bool plain, const EncodeTables& tb) {
    if (plain) {
        *reinterpret_cast<u64x2_t*>(item_out + k) = u64x2_t{a0, a1};
        return;
    }
    const size_t n = (size_t)1 << tb.log2n;
    for (u32 l = 0; l < tb.n_limbs; ++l) {
        const EncLimb lim = tb.limb[l];
        *reinterpret_cast<u64x2_t*>(item_out + l * n + k) = u64x2_t{enc_lift(a0, tb.t, tb.half, lim), enc_lift(a1, tb.t, tb.half, lim)};
    }
}
// the lane's pairs of the chunk: WHOLE the output rows, otherwise the chunk's words parked in row 0 of the item's output
template <bool WHOLE>
DPF_HD void enc_lane_store(u64* item_out, const u32* a, u32 tid, u32 T, u32 base, u32 C, bool plain, const EncodeTables& tb) {
    for (u32 p = 2 * tid; p < C; p += 2 * T) {
        if (WHOLE) enc_store_pair(item_out, p, a[p], a[p + 1], plain, tb);
        else *reinterpret_cast<u64x2_t*>(item_out + base + p) = u64x2_t{a[p], a[p + 1]};
    }
}
// the second kernel of N = 32768 / 65536: the last R = log2 N - log2c levels on the 2^R words 2^log2c apart of columns k, k + 1 (k even), read from row 0
template <int R>
DPF_HD void enc_lane_tail(u64* item_out, u32 k, u32 log2c, bool plain, const EncodeTables& tb) {
    u32 x0[1 << R], x1[1 << R];
#pragma unroll
    for (int c = 0; c < (1 << R); ++c) {
        const u64x2_t w = *reinterpret_cast<const u64x2_t*>(item_out + k + ((size_t)c << log2c));
        x0[c] = (u32)w.x;
        x1[c] = (u32)w.y;
    }
    enc_group<R, true>(x0, k, log2c, tb.log2n, tb.tw, tb.t);
    enc_group<R, true>(x1, k + 1, log2c, tb.log2n, tb.tw, tb.t);
#pragma unroll
    for (int c = 0; c < (1 << R); ++c) enc_store_pair(item_out, k + ((size_t)c << log2c), x0[c], x1[c], plain, tb);
}

// ---- host: the tables of (N, t) from the definition (t already known to be a prime = 1 mod 2N below 2^32); false if t has no primitive 2N-th root
struct EncodeHostTables {
    std::vector<EncTw> tw;
    std::vector<u32> src;
    std::vector<EncLimb> limb;
    u64 zeta = 0;
    EncodeTables view(u32 log2n, u64 t) const { return EncodeTables{tw.data(), src.data(), limb.data(), (u32)t, (u32)((t - 1) / 2), log2n, (u32)limb.size()}; }
};
inline bool enc_host_tables(u32 log2_n, u64 t, const u64* moduli, u32 n_limbs, EncodeHostTables& h) {
    const u64 n = (u64)1 << log2_n;
    u64 zeta = 0;
    for (u64 g = 2; g < t && !zeta; ++g) {   // zeta = g^((t-1)/2N) has order exactly 2N iff zeta^N = -1
        const u64 z = h_powmod(g, (t - 1) / (2 * n), t);
        if (h_powmod(z, n, t) == t - 1) zeta = z;
    }
    if (!zeta) return false;
    h.zeta = zeta;
    auto brv = [&](u32 x) { u32 r = 0; for (u32 i = 0; i < log2_n; ++i) { r = (r << 1) | (x & 1); x >>= 1; } return r; };
    const u64 izeta = h_powmod(zeta, t - 2, t), n_inv = h_powmod(n % t, t - 2, t);
    h.tw.assign(n + 1, EncTw{0, 0});
    u64 ipw = 1;
    for (u64 i = 0; i < n; ++i) {            // entry brv(i) = zeta^-i (brv over log2 N bits): the order the levels read them in
        h.tw[brv((u32)i)] = enc_tw(ipw, t);
        ipw = h_mulmod(ipw, izeta, t);
    }
    h.tw[n] = enc_tw(h_mulmod(n_inv, h.tw[1].w, t), t);
    h.tw[0] = enc_tw(n_inv, t);
    h.src.assign(n, 0);
    u64 e = 1;
    for (u64 i = 0; i < n / 2; ++i) {
        h.src[brv((u32)((e - 1) / 2))] = (u32)i;                      // zeta^(3^i)
        h.src[brv((u32)((2 * n - e - 1) / 2))] = (u32)(n / 2 + i);    // zeta^(-3^i)
        e = e * 3 % (2 * n);
    }
    h.limb.resize(n_limbs);
    for (u32 l = 0; l < n_limbs; ++l) h.limb[l] = EncLimb{moduli[l], ~(u64)0 / moduli[l]};   // = floor(2^64 / q): q is odd, never a power of two
    return true;
}

#if defined(__HIPCC__)
// host twin of the device launch (k_encode.hip launch_encode_slots), tables in host memory
void encode_slots_host(u64* out, const u32* slots, size_t items, bool plain, const EncodeTables& tb);
#endif

}  // namespace dpfhe
