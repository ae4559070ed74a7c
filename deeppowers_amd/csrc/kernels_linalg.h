// kernels_linalg.h - streaming (HBM-bound) kernels of the linear algebra: A7 ct x pt matvec, A8 shard-local reduce.
// Included by cabi_linalg.hip only.  No reference counterpart.
#pragma once
#include <hip/hip_runtime.h>

#include "modarith.h"
#include "reduce_thin.h"
#include "workmap.h"

namespace dpfhe {

// (the streaming kernels below take their work in 512-word chunks of a residue polynomial: workmap.h chunks_of, chunk_work)

// ------------------------------------------------------------------------------------------------
// A8: out[c][l][:] = sum_i in[i][c][l][:]  (HBM-bound: one read per term).
// grid (residue-poly chunks, splits): each workgroup reduces its share of the batch to a canonical partial
// and adds it into `out` (zeroed by the caller on the same stream) with 64-bit atomics - at most 15
// partials < q < 2^60 per word, so the lazy sum cannot wrap.  reduce_final_kernel then canonicalises.
// No workspace, no per-call allocation.
// ------------------------------------------------------------------------------------------------
constexpr int kReduceSplits = 15;

// Work item = (512-word chunk of a residue polynomial, batch split); a workgroup walks the items with stride gridDim.x,
// so the launch size caps how much of the chip (and of the HBM bandwidth) the reduction takes at once.
__global__ __launch_bounds__(256) void reduce_partial_kernel(u64* out, const u64* in, const LimbConst* lcs, int n_limbs, int n, int chunks,
                                                             size_t count, size_t words_per_item, unsigned poly_chunks, unsigned nsplit) {
    for (unsigned work = blockIdx.x; work < poly_chunks * nsplit; work += gridDim.x) {
        const unsigned pc = work % poly_chunks;
        const size_t split = work / poly_chunks;
        const size_t p = pc / (unsigned)chunks;  // residue polynomial within one item
        const int w = (int)(pc % (unsigned)chunks) * 512 + threadIdx.x * 2;
        if (w >= n) continue;
        const u64 q = lcs[p % (size_t)n_limbs].q;
        const size_t lo = count * split / nsplit, hi = count * (split + 1) / nsplit;
        const u64* src = in + p * n + w;
        u64 s0 = 0, s1 = 0;
        size_t it = lo;
        for (; it + 4 <= hi; it += 4) {
            U64x2 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                v[u] = *reinterpret_cast<const U64x2*>(src + (it + u) * words_per_item);   // (non-temporal loads measured no faster here: plain)
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) { s0 = csub(s0 + v[u].a, q); s1 = csub(s1 + v[u].b, q); }
        }
        for (; it < hi; ++it) {
            const U64x2 v = *reinterpret_cast<const U64x2*>(src + it * words_per_item);
            s0 = csub(s0 + v.a, q); s1 = csub(s1 + v.b, q);
        }
        if (hi > lo) {
            atomicAdd(reinterpret_cast<unsigned long long*>(out + p * n + w), (unsigned long long)s0);
            atomicAdd(reinterpret_cast<unsigned long long*>(out + p * n + w + 1), (unsigned long long)s1);
        }
    }
}

// The same partial sums for the sharded multiply's batches (FoldArith limbs, count > 512), built to run BESIDE the fused multiply
// instead of in its place: ct_mul_quad_kernel holds 2 x 240 of a SIMD lane's 512 registers, so a kernel of at most 32 registers, no
// LDS and ONE workgroup per CU (the launcher's grid) is the only shape whose waves fit next to both multiply workgroups of a CU
// (tests/test_reduce_thin_budget.py holds both budgets).  The lazy sums of reduce_thin.h are what make
// 32 registers enough: five 16-byte loads in flight, two accumulators, one lane offset; everything else is wave-uniform.
// Same work items, same atomics into the zeroed `out`, same reduce_final_kernel behind it.
__global__ __launch_bounds__(256) void reduce_thin_kernel(u64* __restrict__ out, const u64* __restrict__ in, const LimbConst* __restrict__ lcs, unsigned n_limbs,
                                                          unsigned n, unsigned log2_chunks, size_t per, unsigned rem, size_t words_per_item, unsigned poly_chunks,
                                                          unsigned nsplit) {
    // launched with min(256, N / 2) threads: no thread is out of range, so every branch and every address part below is wave-uniform but this one
    const unsigned lane = threadIdx.x * 16u;   // byte offset of the thread's two words inside a 512-word chunk
    // split `s` sums items [s per + min(s, rem), (s + 1) per + min(s + 1, rem)); the workgroup walks (chunk, split) with stride gridDim.x, without a division
    unsigned pc = blockIdx.x % poly_chunks, split = blockIdx.x / poly_chunks;
    while (split < nsplit) {
        const unsigned p = pc >> log2_chunks, w0 = (pc & ((1u << log2_chunks) - 1u)) * 512u;
        const LimbConst lc = lcs[p % n_limbs];
        const size_t lo = split * per + (split < rem ? split : rem), hi = (split + 1) * per + (split + 1 < rem ? split + 1 : rem);
        const u64* src = in + (size_t)p * n + w0;
        // (uniform base in scalar registers) + (the lane's 32-bit offset): a raw buffer load takes exactly that - as pointer arithmetic hipcc builds a 64-bit
        // vector address per load (two registers and a v_lshl_add_u64 each: 48 registers instead of 32)
        const U64x2 sum = thin_sum([&](size_t it) {
            typedef unsigned v4u __attribute__((ext_vector_type(4)));
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<u64*>(src + it * words_per_item), 0, 0x7fffffff, 0x00020000);
            const v4u t = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)lane, 0, 0);
            return U64x2{((u64)t.y << 32) | t.x, ((u64)t.w << 32) | t.z};
        }, lo, hi, lc);
        if (hi > lo) {
            u64* o = reinterpret_cast<u64*>(reinterpret_cast<char*>(out + (size_t)p * n + w0) + lane);
            atomicAdd(reinterpret_cast<unsigned long long*>(o), (unsigned long long)sum.a);
            atomicAdd(reinterpret_cast<unsigned long long*>(o + 1), (unsigned long long)sum.b);
        }
        pc += gridDim.x;
        while (pc >= poly_chunks) { pc -= poly_chunks; ++split; }
    }
}

__global__ __launch_bounds__(256) void reduce_final_kernel(u64* out, const LimbConst* lcs, int n_limbs, int n, int chunks) {
    const size_t p = blockIdx.x / chunks;
    const int w = (int)(blockIdx.x % chunks) * 512 + threadIdx.x * 2;
    if (w >= n) return;
    const u64 q = lcs[p % (size_t)n_limbs].q;
    U64x2* o = reinterpret_cast<U64x2*>(out + p * n + w);
    U64x2 v = *o;  // < 15 q
    v.a = csub(csub(csub(csub(v.a, 8 * q), 4 * q), 2 * q), q);
    v.b = csub(csub(csub(csub(v.b, 8 * q), 4 * q), 2 * q), q);
    *o = v;
}

// ------------------------------------------------------------------------------------------------
// A7: y[i][c][l][:] = sum_j W[i][j][l][:] (.) x[j][c][l][:],  c in {0,1}.  128-bit lazy accumulation,
// one reduction at the end.  One workgroup per (row, limb); W is streamed once (the HBM-bound term),
// x (cols x 2 RNS polys) is re-read by every row through L2 / Infinity Cache.
// ------------------------------------------------------------------------------------------------
struct Acc128 {
    u64 lo, hi;
};
__device__ __forceinline__ void acc_mac(Acc128& acc, u64 a, u64 b) {
    const u64 lo = a * b, hi = mulhi64(a, b);
    acc.lo += lo;
    acc.hi += hi + (acc.lo < lo);
}
template <class Arith>
__device__ __forceinline__ u64 acc_reduce(const Acc128& acc, const LimbConst& lc, u64 two64_mod_q) {
    if (Arith::kFold) {  // hi * 2^64 + lo  =  hi * (2^64 mod q) + lo
        const u64 h = FoldArith::mul60_full(acc.hi, two64_mod_q, (u32)lc.d);  // < 2q
        const u64 l = FoldArith::reduce(acc.lo, lc);                      // < 2q
        return FoldArith::canon(h + l, lc);
    } else {
        const u64 h = ShoupArith::mul_var(acc.hi % lc.q, two64_mod_q, lc);
        return add_mod(h, acc.lo % lc.q, lc.q);
    }
}

// RT rows per workgroup: x_j is loaded once per column and re-used from registers for RT rows, so the
// L2/Infinity-Cache traffic for x drops RT-fold and the W stream (read exactly once) owns the HBM pipe.
// grid = (row tiles * L * chunks); every thread owns 2 consecutive words of RT x 2 output polynomials.
template <class Arith, int RT>
__global__ __launch_bounds__(256) void matvec_kernel(u64* y, const u64* W, const u64* x, const LimbConst* lcs, int n_limbs, int n,
                                                     int chunks, size_t rows, size_t cols) {
    const size_t L = (size_t)n_limbs;
    // XCD-aware block ids (workmap.h MatvecMap): slab p = (limb, chunk) on XCD p mod 8, its row tiles adjacent there - the x tile of
    // a slab is fetched from HBM once and re-read from that XCD's L2 by the other row tiles
    const MatvecWork wk = MatvecMap::decode(blockIdx.x, (unsigned)L, (unsigned)chunks, (unsigned)((rows + RT - 1) / RT), 1u);
    if (!wk.live) return;
    const int chunk = wk.chunk, limb = wk.limb;
    const size_t row0 = (size_t)wk.row_tile * RT;
    const int w0 = chunk * 512 + threadIdx.x * 2;
    if (w0 >= n) return;
    const LimbConst lc = lcs[limb];
    const u64 two64 = lc.two64;
    const size_t wstride = L * n, xstride = 2 * L * n, rstride = cols * L * n;
    Acc128 acc[RT][2][2];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[r][c][0] = acc[r][c][1] = Acc128{0, 0};
    const u64* wp = W + (row0 * cols * L + limb) * n + w0;
    const u64* xp = x + (size_t)limb * n + w0;
    size_t since = 0;
    // (requesting column j + 1 before the products of column j measured SLOWER here - 1.46 against 1.38 ms at configs[2]: the 10 extra registers cost the 4th wave per SIMD - removed)
    U64x2 x0 = *reinterpret_cast<const U64x2*>(xp), x1 = *reinterpret_cast<const U64x2*>(xp + L * n), w[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) w[r] = (row0 + r < rows) ? *reinterpret_cast<const U64x2*>(wp + r * rstride) : U64x2{0, 0};
    for (size_t j = 0; j < cols; ++j) {
        if (j > 0) {
            x0 = *reinterpret_cast<const U64x2*>(xp + j * xstride);
            x1 = *reinterpret_cast<const U64x2*>(xp + j * xstride + L * n);
#pragma unroll
            for (int r = 0; r < RT; ++r) w[r] = (row0 + r < rows) ? *reinterpret_cast<const U64x2*>(wp + r * rstride + j * wstride) : U64x2{0, 0};
        }
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            acc_mac(acc[r][0][0], w[r].a, x0.a); acc_mac(acc[r][0][1], w[r].b, x0.b);
            acc_mac(acc[r][1][0], w[r].a, x1.a); acc_mac(acc[r][1][1], w[r].b, x1.b);
        }
        if (++since == 128) {  // 128 products of < 2^120 stay below 2^128 next to a reduced value
#pragma unroll
            for (int r = 0; r < RT; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int k = 0; k < 2; ++k) acc[r][c][k] = Acc128{acc_reduce<Arith>(acc[r][c][k], lc, two64), 0};
            since = 0;
        }
    }
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        if (row0 + r >= rows) break;
        u64* yp = y + (((row0 + r) * 2) * L + limb) * n + w0;
        *reinterpret_cast<U64x2*>(yp) = U64x2{acc_reduce<Arith>(acc[r][0][0], lc, two64), acc_reduce<Arith>(acc[r][0][1], lc, two64)};
        *reinterpret_cast<U64x2*>(yp + L * n) = U64x2{acc_reduce<Arith>(acc[r][1][0], lc, two64), acc_reduce<Arith>(acc[r][1][1], lc, two64)};
    }
}

// A7 with several right-hand sides (tokens): y[i][t] = sum_j W[i][j] (.) x[j][t], x: [cols][C/2][2][L][N], y: [rows][C/2][2][L][N]; the
// C = 2 * tokens polynomials of a column are just more "components".  A weight tile is loaded once per RT rows and used for all
// tokens: the W stream (the 335 MB of diagonals of a packed GPT-2 layer) is read once per launch instead of once per token.
template <class Arith, int RT, int C>
__global__ __launch_bounds__(256) void matvec_multi_kernel(u64* y, const u64* W, const u64* x, const LimbConst* lcs, int n_limbs, int n,
                                                           int chunks, size_t rows, size_t cols, size_t polys_per_col /* >= C: the full [n_rhs][2] extent */,
                                                           unsigned n_groups, unsigned n_tiles) {
    // `n_groups` groups of C / 2 right-hand sides and all row tiles in ONE launch, block ids laid out for the 8 XCDs (workmap.h MatvecMap):
    // slab p = (limb, chunk of 512 words) lives on XCD p mod 8, and its row tiles x groups are adjacent ids on that XCD.  The G workgroups of a
    // row tile read the same W tile and the R workgroups of a group the same x tile at about the same time: each is fetched from HBM once.
    const size_t L = (size_t)n_limbs;
    const unsigned n_slabs = (unsigned)L * (unsigned)chunks;   // n_tiles = row tiles * slabs
    const MatvecWork wk = MatvecMap::decode(blockIdx.x, (unsigned)L, (unsigned)chunks, n_tiles / n_slabs, n_groups);
    if (!wk.live) return;
    const unsigned group = wk.group;
    const int chunk = wk.chunk, limb = wk.limb;
    const size_t row0 = (size_t)wk.row_tile * RT;
    const int w0 = chunk * 512 + threadIdx.x * 2;
    if (w0 >= n) return;
    x += (size_t)group * C * L * n;
    y += (size_t)group * C * L * n;
    const LimbConst lc = lcs[limb];
    const u64 two64 = lc.two64;
    const size_t wstride = L * n, xstride = polys_per_col * L * n, rstride = cols * L * n;
    Acc128 acc[RT][C][2];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int c = 0; c < C; ++c) acc[r][c][0] = acc[r][c][1] = Acc128{0, 0};
    const u64* wp = W + (row0 * cols * L + limb) * n + w0;
    const u64* xp = x + (size_t)limb * n + w0;
    size_t since = 0;
    // software pipeline: the operands of column j + 1 are requested before the RT * C multiply-accumulates of column j (there are
    // only `cols` = 32 iterations in a packed layer and two waves per SIMD: nothing else hides the HBM latency of the W tiles)
    U64x2 w[RT], xv[C];
#pragma unroll
    for (int r = 0; r < RT; ++r) w[r] = (row0 + r < rows) ? *reinterpret_cast<const U64x2*>(wp + r * rstride) : U64x2{0, 0};
#pragma unroll
    for (int c = 0; c < C; ++c) xv[c] = *reinterpret_cast<const U64x2*>(xp + (size_t)c * L * n);
    for (size_t j = 0; j < cols; ++j) {
        const size_t jn = j + 1 < cols ? j + 1 : j;
        U64x2 wn[RT], xn[C];
#pragma unroll
        for (int r = 0; r < RT; ++r) wn[r] = (row0 + r < rows) ? *reinterpret_cast<const U64x2*>(wp + r * rstride + jn * wstride) : U64x2{0, 0};
#pragma unroll
        for (int c = 0; c < C; ++c) xn[c] = *reinterpret_cast<const U64x2*>(xp + jn * xstride + (size_t)c * L * n);
#pragma unroll
        for (int c = 0; c < C; ++c) {
#pragma unroll
            for (int r = 0; r < RT; ++r) { acc_mac(acc[r][c][0], w[r].a, xv[c].a); acc_mac(acc[r][c][1], w[r].b, xv[c].b); }
        }
#pragma unroll
        for (int r = 0; r < RT; ++r) w[r] = wn[r];
#pragma unroll
        for (int c = 0; c < C; ++c) xv[c] = xn[c];
        if (++since == 128) {
#pragma unroll
            for (int r = 0; r < RT; ++r)
#pragma unroll
                for (int c = 0; c < C; ++c)
#pragma unroll
                    for (int k = 0; k < 2; ++k) acc[r][c][k] = Acc128{acc_reduce<Arith>(acc[r][c][k], lc, two64), 0};
            since = 0;
        }
    }
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        if (row0 + r >= rows) break;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            u64* yp = y + (((row0 + r) * polys_per_col + c) * L + limb) * n + w0;
            *reinterpret_cast<U64x2*>(yp) = U64x2{acc_reduce<Arith>(acc[r][c][0], lc, two64), acc_reduce<Arith>(acc[r][c][1], lc, two64)};
        }
    }
}

// A7 for FoldArith contexts (round 3): the same product with the split-at-bit-30 column accumulators of modarith.h
// (FoldArith::dot30_mac: FOUR multiply-adds per term instead of the 21 instructions of a 128-bit accumulate; one 18-instruction
// fold per 8 columns).  W tile (RT rows) and x tile (C polynomials) of a column are split once and used RT x C times.  Same
// XCD-aware block ids, same software pipeline; WPT words per thread (chunks of 256 WPT words).  Serves dpfhe_matvec_plain
// (C = 2, one group) and dpfhe_matvec_plain_multi.
template <int WPT> struct WordVec;
template <> struct WordVec<1> { u64 v[1]; };
template <> struct __attribute__((aligned(16))) WordVec<2> { u64 v[2]; };
template <int WPT, bool NT = false>
__device__ __forceinline__ WordVec<WPT> load_words(const u64* p, bool in_range) {   // rows beyond the matrix read as zero
    WordVec<WPT> r;
    if (in_range) {
        if (NT) {
#pragma unroll
            for (int k = 0; k < WPT; ++k) r.v[k] = __builtin_nontemporal_load(p + k);
        } else r = *reinterpret_cast<const WordVec<WPT>*>(p);
    } else {
#pragma unroll
        for (int k = 0; k < WPT; ++k) r.v[k] = 0;
    }
    return r;
}

// NTW: the W tiles are read once by ONE workgroup (a single group of right-hand sides) and W does not fit the Infinity Cache: non-temporal loads
// WD: how many columns AHEAD the W words are requested (a register ring of WD x RT words; WD divides the period).  The W stream is the one
// operand that comes from HBM (one workgroup group reads each tile once), x comes from L2: round 4 measured ~3.6 us from issue to first word for
// an HBM burst under load, against ~0.5 us of products per column - one column of lookahead cannot cover it.
// FULL: rows is a multiple of RT and cols a multiple of the period (what a packed layer's products are) - no row predicate on the W loads and no
// ragged last period, i.e. NO control flow inside the period: its 8 columns are one basic block, the double-buffered operands are renamed at
// compile time and the loads of column j + 1 are waited for where column j + 1 first uses them.  With the checks in place every column was its
// own block that ended in register copies of the next operands behind s_waitcnt vmcnt(0): the one-column lookahead the source asks for
// did not exist in the binary.
constexpr int kMatvecFullDepth = 1;   // columns of lookahead of the FULL form (both operands)
template <int RT, int C, int WPT, bool NTW = false, int WD = 1, bool FULL = false>
__global__ __launch_bounds__(256) void matvec_fold_kernel(u64* y, const u64* W, const u64* x, const LimbConst* lcs, int n_limbs, int n,
                                                          int chunks, size_t rows, size_t cols, size_t polys_per_col, unsigned n_groups,
                                                          unsigned n_tiles) {
    typedef WordVec<WPT> V;
    typedef FoldArith::Half30 H;
    constexpr int P = FoldArith::kDot30Period;
    const size_t L = (size_t)n_limbs;
    const unsigned n_slabs = (unsigned)L * (unsigned)chunks;
    const MatvecWork wk = MatvecMap::decode(blockIdx.x, (unsigned)L, (unsigned)chunks, n_tiles / n_slabs, n_groups);
    if (!wk.live) return;
    const unsigned group = wk.group;
    const int chunk = wk.chunk, limb = wk.limb;
    const size_t row0 = (size_t)wk.row_tile * RT;
    const unsigned w0 = (unsigned)(chunk * 256 * WPT + (int)threadIdx.x * WPT);   // the ONLY per-thread part of every address
    if ((int)w0 >= n) return;
    x += (size_t)group * C * L * n;
    y += (size_t)group * C * L * n;
    const LimbConst lc = lcs[limb];
    const size_t wstride = L * n, xstride = polys_per_col * L * n, rstride = cols * L * n;
    // uniform bases (scalar registers, scalar adds) + one 32-bit lane offset: no per-lane 64-bit address arithmetic
    const u64* const wu = W + (row0 * cols * L + limb) * n;
    const u64* const xu = x + (size_t)limb * n;
    // (uniform 64-bit base) + (32-bit BYTE offset of the lane): the shape the global_load "saddr" form takes - base in scalar registers, one
    // 32-bit vector offset shared by every load of the thread; indexing the u64 pointer with w0 instead makes hipcc scale in 64 bits per lane
    // (one v_lshl_add_u64 and a 64-bit vector address per load: 12 % of the kernel's vector instructions)
    auto ld_w = [&](int r, size_t j) { return load_words<WPT, NTW>(&(wu + (r * rstride + j * wstride))[w0], FULL || row0 + r < rows); };
    auto ld_x = [&](int c, size_t j) { return *reinterpret_cast<const V*>(&(xu + (j * xstride + (size_t)c * L * n))[w0]); };
    u64 run[RT][C][WPT];   // folded running words (reduced); the first products of every period chain onto them
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int k = 0; k < WPT; ++k) run[r][c][k] = 0;
    if constexpr (FULL) {
        // Both operands of column j + FD are requested at the top of column j into a register ring of FD columns, and a scheduling barrier
        // closes every column: without it the scheduler pulls the (cheap) splits of the next column's operands up into the current one and
        // the wait for them with it - half a column of lookahead instead of FD columns.
        constexpr int FD = kMatvecFullDepth;
        static_assert(P % FD == 0, "the operand ring must divide the period");
        // Every load of the thread is (uniform 64-bit base) + (ONE 32-bit byte offset of the lane).  Written as pointer arithmetic hipcc folds the lane part
        // into a 64-bit vector base and adds the uniform part per load (one v_lshl_add_u64 and an address register pair each: 12 % of the kernel's vector
        // instructions); a raw buffer load takes the base in scalar registers (the descriptor, rebuilt per load by the scalar unit - W may exceed a 32-bit
        // offset) and the lane offset as is.
        const unsigned b0 = w0 * 8u;
        auto bld = [&](const u64* uniform) {
            V r;
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<u64*>(uniform), 0, 0x7fffffff, 0x00020000);
            if constexpr (WPT == 1) {
                typedef unsigned v2u __attribute__((ext_vector_type(2)));
                const v2u t = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)b0, 0, NTW ? 2 : 0);
                r.v[0] = ((u64)t.y << 32) | t.x;
            } else {
                typedef unsigned v4u __attribute__((ext_vector_type(4)));
                const v4u t = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)b0, 0, NTW ? 2 : 0);
                r.v[0] = ((u64)t.y << 32) | t.x; r.v[1] = ((u64)t.w << 32) | t.z;
            }
            return r;
        };
        auto ld_w = [&](int r, size_t j) { return bld(wu + (r * rstride + j * wstride)); };
        auto ld_x = [&](int c, size_t j) { return bld(xu + (j * xstride + (size_t)c * L * n)); };
        V wr[FD][RT], xr[FD][C];
#pragma unroll
        for (int d = 0; d < FD; ++d) {
            const size_t jd = (size_t)d < cols ? (size_t)d : cols - 1;
#pragma unroll
            for (int r = 0; r < RT; ++r) wr[d][r] = ld_w(r, jd);
#pragma unroll
            for (int c = 0; c < C; ++c) xr[d][c] = ld_x(c, jd);
        }
        for (size_t j0 = 0; j0 < cols; j0 += P) {
            FoldArith::Dot30 acc[RT][C][WPT];
#pragma unroll
            for (int u = 0; u < P; ++u) {
                const size_t j = j0 + u, jp = j + FD < cols ? j + FD : cols - 1;
                V w[RT], xv[C];
#pragma unroll
                for (int r = 0; r < RT; ++r) { w[r] = wr[u % FD][r]; wr[u % FD][r] = ld_w(r, jp); }
#pragma unroll
                for (int c = 0; c < C; ++c) { xv[c] = xr[u % FD][c]; xr[u % FD][c] = ld_x(c, jp); }
                __builtin_amdgcn_sched_barrier(0);   // ... and the requests stay up here (the scheduler otherwise sinks them to the end of the column to save registers)
#pragma unroll
                for (int k = 0; k < WPT; ++k) {
                    H wh[RT], xh[C];
#pragma unroll
                    for (int r = 0; r < RT; ++r) wh[r] = FoldArith::split30(w[r].v[k]);
#pragma unroll
                    for (int c = 0; c < C; ++c) xh[c] = FoldArith::split30(xv[c].v[k]);
#pragma unroll
                    for (int c = 0; c < C; ++c)
#pragma unroll
                        for (int r = 0; r < RT; ++r) {
                            if (u == 0) acc[r][c][k] = FoldArith::Dot30{run[r][c][k], 0, 0};
                            FoldArith::dot30_mac(acc[r][c][k], wh[r], xh[c]);
                        }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int r = 0; r < RT; ++r) {
#pragma unroll
                for (int c = 0; c < C; ++c)
#pragma unroll
                    for (int k = 0; k < WPT; ++k) run[r][c][k] = FoldArith::dot30_fold0(acc[r][c][k], lc);
                __builtin_amdgcn_sched_barrier(0);   // one row of folds at a time: interleaving all sixteen costs ten more registers (and the third wave per SIMD)
            }
        }
    } else {
    static_assert(WD >= 1 && FoldArith::kDot30Period % WD == 0, "the W ring must divide the period");
    V wq[WD][RT], xv[C];
#pragma unroll
    for (int d = 0; d < WD; ++d)
#pragma unroll
        for (int r = 0; r < RT; ++r) wq[d][r] = ld_w(r, (size_t)d < cols ? (size_t)d : cols - 1);
#pragma unroll
    for (int c = 0; c < C; ++c) xv[c] = ld_x(c, 0);
    // Periods of P columns, unrolled: the accumulators of a period start from {running word, 0, 0} as multiply-add addends (no
    // zeroing moves), the operands of column j + 1 are requested before the RT x C products of column j, one fold ends the period.
    for (size_t j0 = 0; j0 < cols; j0 += P) {
        FoldArith::Dot30 acc[RT][C][WPT];
#pragma unroll
        for (int u = 0; u < P; ++u) {
            const size_t j = j0 + u;
            if constexpr (!FULL) {
                if (j >= cols) {   // ragged last period: nothing to add (uniform branch)
                    if (u == 0) break;
                    continue;
                }
            }
            const size_t jn = j + 1 < cols ? j + 1 : j, jw = j + WD < cols ? j + WD : cols - 1;
            V w[RT], xn[C];
#pragma unroll
            for (int r = 0; r < RT; ++r) { w[r] = wq[u % WD][r]; wq[u % WD][r] = ld_w(r, jw); }   // slot of column j is free: column j + WD goes there
#pragma unroll
            for (int c = 0; c < C; ++c) xn[c] = ld_x(c, jn);
#pragma unroll
            for (int k = 0; k < WPT; ++k) {
                H wh[RT], xh[C];
#pragma unroll
                for (int r = 0; r < RT; ++r) wh[r] = FoldArith::split30(w[r].v[k]);
#pragma unroll
                for (int c = 0; c < C; ++c) xh[c] = FoldArith::split30(xv[c].v[k]);
#pragma unroll
                for (int c = 0; c < C; ++c)
#pragma unroll
                    for (int r = 0; r < RT; ++r) {
                        if (u == 0) acc[r][c][k] = FoldArith::Dot30{run[r][c][k], 0, 0};
                        FoldArith::dot30_mac(acc[r][c][k], wh[r], xh[c]);
                    }
            }
#pragma unroll
            for (int c = 0; c < C; ++c) xv[c] = xn[c];
        }
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int k = 0; k < WPT; ++k) run[r][c][k] = FoldArith::dot30_fold(acc[r][c][k], 0, lc);
    }
    }
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        if (!FULL && row0 + r >= rows) break;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            V o;
#pragma unroll
            for (int k = 0; k < WPT; ++k) o.v[k] = FoldArith::canon_small(run[r][c][k], lc);
            *reinterpret_cast<V*>(&(y + (((row0 + r) * polys_per_col + c) * L + limb) * n)[w0]) = o;
        }
    }
}

// A7, scalar weights (SURVEY.md section 8a A7 "cheap special case"): W_ij are residues in Z_q (one word per limb),
// y_i = sum_j w_ij * x_j.  The weights of a row tile are workgroup-uniform (scalar loads -> SGPR multiplier operands),
// x_j is loaded once per column and used for RT rows: RT*4 multiply-accumulates per 32 bytes loaded - ALU-bound.
// d_w: [rows][cols][L];  x: [cols][2][L][N];  y: [rows][2][L][N].
template <class Arith, int RT>
__global__ __launch_bounds__(256) void matvec_scalar_kernel(u64* y, const u64* w, const u64* x, const LimbConst* lcs, int n_limbs, int n,
                                                            int chunks, size_t rows, size_t cols) {
    const size_t L = (size_t)n_limbs;
    const ChunkWork wk = chunk_work(blockIdx.x, chunks, L);   // poly = row tile
    const int chunk = wk.chunk, limb = wk.limb;
    const size_t row0 = wk.poly * RT;
    const int w0 = chunk * 512 + threadIdx.x * 2;
    if (w0 >= n) return;
    const LimbConst lc = lcs[limb];
    const u64 two64 = lc.two64;
    const size_t xstride = 2 * L * n;
    Acc128 acc[RT][2][2];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[r][c][0] = acc[r][c][1] = Acc128{0, 0};
    const u64* xp = x + (size_t)limb * n + w0;
    size_t since = 0;
    for (size_t j = 0; j < cols; ++j) {
        const U64x2 x0 = *reinterpret_cast<const U64x2*>(xp + j * xstride);
        const U64x2 x1 = *reinterpret_cast<const U64x2*>(xp + j * xstride + L * n);
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const size_t row = row0 + r < rows ? row0 + r : rows - 1;   // clamp: out-of-range rows are computed, not stored
            const u64 wr = w[(row * cols + j) * L + limb];              // uniform -> scalar load
            acc_mac(acc[r][0][0], wr, x0.a); acc_mac(acc[r][0][1], wr, x0.b);
            acc_mac(acc[r][1][0], wr, x1.a); acc_mac(acc[r][1][1], wr, x1.b);
        }
        if (++since == 128) {
#pragma unroll
            for (int r = 0; r < RT; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int k = 0; k < 2; ++k) acc[r][c][k] = Acc128{acc_reduce<Arith>(acc[r][c][k], lc, two64), 0};
            since = 0;
        }
    }
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        if (row0 + r >= rows) break;
        u64* yp = y + (((row0 + r) * 2) * L + limb) * n + w0;
        *reinterpret_cast<U64x2*>(yp) = U64x2{acc_reduce<Arith>(acc[r][0][0], lc, two64), acc_reduce<Arith>(acc[r][0][1], lc, two64)};
        *reinterpret_cast<U64x2*>(yp + L * n) = U64x2{acc_reduce<Arith>(acc[r][1][0], lc, two64), acc_reduce<Arith>(acc[r][1][1], lc, two64)};
    }
}

}  // namespace dpfhe
