// cencode.h - complex slot encoding (include/dpfhe.h "complex slot encoding"): the half-size inverse transform in FP64, then scale, round and lift.
//
//   N = 2^log2n, n = N / 2, xi = exp(i pi / N).  With c_j = m_j + i m_(j+n) (j < n) one has c(xi^e) = m(xi^e) for every e = 1 mod 4 (xi^(e n) = i),
//   and those n points e = 4 r + 1 carry z_i (i even, e = 3^i) and conj(z_i) (i odd, e = 2N - 3^i).  So c is the polynomial of degree < n mod
//   X^n - i with these values: position p = brv((e - 1) / 4) (brv over log2 n bits) of a vector a holds the value at xi^e, and c is its inverse
//   transform: Gentleman-Sande butterflies (u, v) -> (u + v, (u - v) w), level `lg` pairing words h = 2^lg apart with w = xi^-(h (1 + 4 brv(block)))
//   for the block j >> (lg + 1) of its pair, levels lg = 0 ... log2 n - 1, then Delta / n (a multiplication of both outputs of the last level).
//   Several levels run per pass over the vector: a group of 2^R words 2^lg0 apart is loaded once and goes through R levels in registers.
//   Every operation is an IEEE add, multiply or rint on doubles in a fixed order (no fma, no contraction: -ffp-contract=off), the twiddles come from
//   one table built on the host, so the device kernels (k_cencode.hip), the host twin and tools/emulate_cencode.cpp give the same words.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include <cmath>
#include <cstdint>
#include <vector>

#include "modarith.h"

namespace dpfhe {

constexpr u32 kCencRadixLog = 3;        // levels per pass
constexpr u32 kCencConj = 0x80000000u;  // src entry: the position holds the conjugate of the slot
constexpr double kCencClamp = 4611686018427387904.0;   // 2^62

#if defined(__HIPCC__)
typedef double cenc_f64x2 __attribute__((ext_vector_type(2)));
typedef u32 cenc_u32x4 __attribute__((ext_vector_type(4)));
#else
struct alignas(16) cenc_f64x2 { double x, y; };
struct alignas(16) cenc_u32x4 { u32 x, y, z, w; };
#endif

struct CencLimb {
    u64 q;
    u64 mu;   // floor(2^64 / q)
};

// what a launch needs of N: entry m + b of `tw` (x = re, y = im) is xi^-(h (1 + 4 brv(b))), h = n / 2m, for block b of the level with m blocks (m a power
// of two, brv over log2 m bits); entry 0 is unused.  src[p] is the slot whose value position p holds, with kCencConj set where it is the conjugate.
struct CencodeTables {
    const cenc_f64x2* tw;   // n entries
    const u32* src;         // n entries
    const CencLimb* limb;   // n_limbs entries
    u32 log2n, n_limbs;     // log2n = log2 N (the transform has log2n - 1 levels)
};

DPF_HD cenc_f64x2 cenc_add(cenc_f64x2 a, cenc_f64x2 b) { return cenc_f64x2{a.x + b.x, a.y + b.y}; }
DPF_HD cenc_f64x2 cenc_sub(cenc_f64x2 a, cenc_f64x2 b) { return cenc_f64x2{a.x - b.x, a.y - b.y}; }
DPF_HD cenc_f64x2 cenc_mul(cenc_f64x2 a, cenc_f64x2 w) { return cenc_f64x2{a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }
DPF_HD cenc_f64x2 cenc_scale(cenc_f64x2 a, double s) { return cenc_f64x2{a.x * s, a.y * s}; }

// the slot of position `s` (a src entry) of one vector: (re, im) pairs, or REAL doubles
DPF_HD cenc_f64x2 cenc_slot(const double* __restrict__ v, u32 s, bool real) {
    const u32 i = s & ~kCencConj;
    if (real) return cenc_f64x2{v[i], 0.0};
    const cenc_f64x2 z = *reinterpret_cast<const cenc_f64x2*>(v + 2 * (size_t)i);
    return (s & kCencConj) ? cenc_f64x2{z.x, -z.y} : z;
}

// the integer a transformed value y stands for: NaN -> 0, clamp to [-2^62, 2^62], ties to even
DPF_HD int64_t cenc_round(double y) {
    if (y != y) return 0;
    y = y < -kCencClamp ? -kCencClamp : (y > kCencClamp ? kCencClamp : y);
    return (int64_t)__builtin_rint(y);
}
// c mod q, canonical (|c| <= 2^62, q odd in [3, 2^60])
DPF_HD u64 cenc_lift(int64_t c, const CencLimb& l) {
    const bool neg = c < 0;
    const u64 a = neg ? (u64)0 - (u64)c : (u64)c;
    const u64 x = csub(a - mulhi64(a, l.mu) * l.q, l.q);   // the quotient estimate is short by at most 1
    return neg && x ? l.q - x : x;
}

// R levels lg0 ... lg0 + R - 1 on the 2^R words x[k] = a[j0 + (k << lg0)] of one group; LAST: level lg0 + R - 1 is the transform's last (log2 n - 1) and
// both its outputs are multiplied by `scale` (Delta / n)
template <int R, bool LAST>
DPF_HD void cenc_group(cenc_f64x2 (&x)[1 << R], u32 j0, u32 lg0, u32 log2h, const cenc_f64x2* __restrict__ tw, double scale) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const u32 lg = lg0 + r;
#pragma unroll
        for (int k = 0; k < (1 << R); ++k) {
            if (k & (1 << r)) continue;
            const cenc_f64x2 u = x[k], v = x[k | (1 << r)];
            const u32 j = j0 + ((u32)k << lg0);
            const cenc_f64x2 s = cenc_add(u, v), d = cenc_mul(cenc_sub(u, v), tw[(1u << (log2h - 1 - lg)) + (j >> (lg + 1))]);
            if (LAST && r == R - 1) {
                x[k] = cenc_scale(s, scale);
                x[k | (1 << r)] = cenc_scale(d, scale);
            } else {
                x[k] = s;
                x[k | (1 << r)] = d;
            }
        }
    }
}

// group g of the pass that starts at level lg0, on a vector in memory (LDS on the device, an array on the host) whose word 0 is position `base`
template <int R, bool LAST>
DPF_HD void cenc_group_mem(cenc_f64x2* a, u32 g, u32 base, u32 lg0, u32 log2h, const cenc_f64x2* __restrict__ tw, double scale) {
    const u32 lo = g & ((1u << lg0) - 1u);
    const u32 p0 = ((g >> lg0) << (lg0 + R)) + lo;
    cenc_f64x2 x[1 << R];
#pragma unroll
    for (int k = 0; k < (1 << R); ++k) x[k] = a[p0 + ((u32)k << lg0)];
    cenc_group<R, LAST>(x, base + p0, lg0, log2h, tw, scale);
#pragma unroll
    for (int k = 0; k < (1 << R); ++k) a[p0 + ((u32)k << lg0)] = x[k];
}

// ---- the lane's steps of the LDS kernel between two barriers: k_cencode.hip runs them on the device, tools/emulate_cencode.cpp lane by lane on the CPU.
// `a` holds the C = 2^log2c complex words of the chunk that starts at position `base` (the whole vector when C = n); lane `tid` of T.

// levels 0 ... 2 (log2c >= 7: never the last pass) on 8 adjacent words gathered straight from the slot vector v
DPF_HD void cenc_lane_first_pass(cenc_f64x2* a, const double* __restrict__ v, bool real, u32 tid, u32 T, u32 base, u32 C, const CencodeTables& tb) {
    for (u32 g = tid; g < (C >> kCencRadixLog); g += T) {
        const u32 p0 = g << kCencRadixLog;
        const cenc_u32x4 s0 = *reinterpret_cast<const cenc_u32x4*>(tb.src + base + p0), s1 = *reinterpret_cast<const cenc_u32x4*>(tb.src + base + p0 + 4);
        cenc_f64x2 x[8] = {cenc_slot(v, s0.x, real), cenc_slot(v, s0.y, real), cenc_slot(v, s0.z, real), cenc_slot(v, s0.w, real),
                           cenc_slot(v, s1.x, real), cenc_slot(v, s1.y, real), cenc_slot(v, s1.z, real), cenc_slot(v, s1.w, real)};
        cenc_group<3, false>(x, base + p0, 0, tb.log2n - 1, tb.tw, 0.0);
#pragma unroll
        for (int k = 0; k < 8; ++k) a[p0 + k] = x[k];
    }
}
// levels lg0 ... lg0 + 2, not the last pass
DPF_HD void cenc_lane_mid_pass(cenc_f64x2* a, u32 tid, u32 T, u32 base, u32 C, u32 lg0, const CencodeTables& tb) {
    for (u32 g = tid; g < (C >> kCencRadixLog); g += T) cenc_group_mem<3, false>(a, g, base, lg0, tb.log2n - 1, tb.tw, 0.0);
}
// the chunk's last pass: the 1 ... 3 levels from lg0 to log2c - 1; WHOLE: they end the transform (scale folded in)
template <bool WHOLE>
DPF_HD void cenc_lane_last_pass(cenc_f64x2* a, u32 tid, u32 T, u32 base, u32 log2c, u32 lg0, double scale, const CencodeTables& tb) {
    const u32 C = 1u << log2c, log2h = tb.log2n - 1;
    switch (log2c - lg0) {
    case 1: for (u32 g = tid; g < (C >> 1); g += T) cenc_group_mem<1, WHOLE>(a, g, base, lg0, log2h, tb.tw, scale); break;
    case 2: for (u32 g = tid; g < (C >> 2); g += T) cenc_group_mem<2, WHOLE>(a, g, base, lg0, log2h, tb.tw, scale); break;
    default: for (u32 g = tid; g < (C >> 3); g += T) cenc_group_mem<3, WHOLE>(a, g, base, lg0, log2h, tb.tw, scale); break;
    }
}
// coefficients j, j + 1 (from the real parts) and j + n, j + n + 1 (from the imaginary parts) of one item, j even: the plain words (two's complement), or
// their residues on every limb row (16-byte stores)
DPF_HD void cenc_store_pair(u64* item_out, size_t j, cenc_f64x2 c0, cenc_f64x2 c1, bool plain, const CencodeTables& tb) {
    const size_t n = (size_t)1 << tb.log2n, h = n >> 1;
    const int64_t r0 = cenc_round(c0.x), r1 = cenc_round(c1.x), i0 = cenc_round(c0.y), i1 = cenc_round(c1.y);
    if (plain) {
        *reinterpret_cast<u64x2_t*>(item_out + j) = u64x2_t{(u64)r0, (u64)r1};
        *reinterpret_cast<u64x2_t*>(item_out + h + j) = u64x2_t{(u64)i0, (u64)i1};
        return;
    }
    for (u32 l = 0; l < tb.n_limbs; ++l) {
        const CencLimb lim = tb.limb[l];
        *reinterpret_cast<u64x2_t*>(item_out + l * n + j) = u64x2_t{cenc_lift(r0, lim), cenc_lift(r1, lim)};
        *reinterpret_cast<u64x2_t*>(item_out + l * n + h + j) = u64x2_t{cenc_lift(i0, lim), cenc_lift(i1, lim)};
    }
}
// the lane's pairs of the chunk: WHOLE the output rows; otherwise the chunk's words parked in row 0 of the item's output, real parts at words j, imaginary
// parts at words n + j - the very words the second kernel's lane of columns j, j + 1 will overwrite with coefficients j and n + j
template <bool WHOLE>
DPF_HD void cenc_lane_store(u64* item_out, const cenc_f64x2* a, u32 tid, u32 T, u32 base, u32 C, bool plain, const CencodeTables& tb) {
    const size_t h = (size_t)1 << (tb.log2n - 1);
    for (u32 p = 2 * tid; p < C; p += 2 * T) {
        const cenc_f64x2 c0 = a[p], c1 = a[p + 1];
        if (WHOLE) cenc_store_pair(item_out, p, c0, c1, plain, tb);
        else {
            double* park = reinterpret_cast<double*>(item_out);
            *reinterpret_cast<cenc_f64x2*>(park + base + p) = cenc_f64x2{c0.x, c1.x};
            *reinterpret_cast<cenc_f64x2*>(park + h + base + p) = cenc_f64x2{c0.y, c1.y};
        }
    }
}
// the second kernel of N = 32768 / 65536: the last R = log2 n - log2c levels on the 2^R words 2^log2c apart of columns k, k + 1 (k even), read from row 0
template <int R>
DPF_HD void cenc_lane_tail(u64* item_out, u32 k, u32 log2c, double scale, bool plain, const CencodeTables& tb) {
    const size_t h = (size_t)1 << (tb.log2n - 1);
    const double* park = reinterpret_cast<const double*>(item_out);
    cenc_f64x2 x0[1 << R], x1[1 << R];
#pragma unroll
    for (int c = 0; c < (1 << R); ++c) {
        const size_t j = k + ((size_t)c << log2c);
        const cenc_f64x2 re = *reinterpret_cast<const cenc_f64x2*>(park + j), im = *reinterpret_cast<const cenc_f64x2*>(park + h + j);
        x0[c] = cenc_f64x2{re.x, im.x};
        x1[c] = cenc_f64x2{re.y, im.y};
    }
    cenc_group<R, true>(x0, k, log2c, tb.log2n - 1, tb.tw, scale);
    cenc_group<R, true>(x1, k + 1, log2c, tb.log2n - 1, tb.tw, scale);
#pragma unroll
    for (int c = 0; c < (1 << R); ++c) cenc_store_pair(item_out, k + ((size_t)c << log2c), x0[c], x1[c], plain, tb);
}

// ---- host: the tables of N from the definition
// xi^e, e in [0, 2N): cos and sin of an angle in [0, pi/4] in extended precision, placed by the octant, so each component is the correctly rounded value
// (to within 2^-11 ulp of double rounding) and the axis points are exact
inline cenc_f64x2 cenc_root(u64 e, u32 log2_n) {
    const u64 n = (u64)1 << (log2_n - 1);   // a quarter turn
    const u64 quad = (e / n) & 3, rem = e % n;
    const bool swap = rem > n / 2;
    const long double pi = 3.14159265358979323846264338327950288L;
    const long double ang = pi * (long double)(swap ? n - rem : rem) / (long double)(2 * n);
    double c = (double)cosl(ang), s = (double)sinl(ang);
    if (swap) { const double t = c; c = s; s = t; }
    switch (quad) {
    case 0: return cenc_f64x2{c, s};
    case 1: return cenc_f64x2{-s, c};
    case 2: return cenc_f64x2{-c, -s};
    default: return cenc_f64x2{s, -c};
    }
}
struct CencodeHostTables {
    std::vector<cenc_f64x2> tw;
    std::vector<u32> src;
    std::vector<CencLimb> limb;
    CencodeTables view(u32 log2n) const { return CencodeTables{tw.data(), src.data(), limb.data(), log2n, (u32)limb.size()}; }
};
inline void cenc_host_tables(u32 log2_n, const u64* moduli, u32 n_limbs, CencodeHostTables& t) {
    const u64 n2 = (u64)2 << log2_n, h = (u64)1 << (log2_n - 1);
    const u32 bits = log2_n - 1;
    auto brv = [](u64 x, u32 b) { u64 r = 0; for (u32 i = 0; i < b; ++i) { r = (r << 1) | (x & 1); x >>= 1; } return r; };
    t.tw.assign(h, cenc_f64x2{0.0, 0.0});
    for (u32 d = 0; d < bits; ++d) {
        const u64 m = (u64)1 << d, step = h / (2 * m);
        for (u64 b = 0; b < m; ++b) t.tw[m + b] = cenc_root((n2 - step * (1 + 4 * brv(b, d)) % n2) % n2, log2_n);
    }
    t.src.assign(h, 0);
    u64 e = 1;
    for (u64 i = 0; i < h; ++i) {
        if (i & 1) t.src[brv((n2 - e - 1) / 4, bits)] = (u32)i | kCencConj;   // xi^(-3^i) carries conj(z_i)
        else t.src[brv((e - 1) / 4, bits)] = (u32)i;                          // xi^(3^i) carries z_i
        e = e * 3 % n2;
    }
    t.limb.resize(n_limbs);
    for (u32 l = 0; l < n_limbs; ++l) t.limb[l] = CencLimb{moduli[l], ~(u64)0 / moduli[l]};   // = floor(2^64 / q): q is odd, never a power of two
}

#if defined(__HIPCC__)
// host twin of the device launch (k_cencode.hip launch_encode_complex), tables in host memory
void encode_complex_host(u64* out, const double* slots, size_t items, double scale_over_n, bool real, bool plain, const CencodeTables& tb);
// z_i = m(xi^(3^i)) / scale from centred coefficients ([items][N]); real: the real parts only
void decode_complex_host(double* slots_out, const int64_t* coeffs, size_t items, double scale, bool real, u32 log2_n);
#endif

}  // namespace dpfhe
