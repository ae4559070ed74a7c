// kernels_poly.h - coefficient-wise streaming (HBM-bound) kernels: A3 dyadic ops and the plain copy.
// Included by cabi_poly.hip only.  No reference counterpart.
#pragma once
#include <hip/hip_runtime.h>

#include "launch.h"
#include "modarith.h"
#include "stream_access.h"

namespace dpfhe {

// ------------------------------------------------------------------------------------------------
// A3: coefficient-wise ops.  One workgroup per residue polynomial (limb constants are scalar loads),
// 16-byte accesses, every load of an iteration issued before its first use.
// ------------------------------------------------------------------------------------------------
// (DyOp: launch.h)

template <class Arith, int OP>
__device__ __forceinline__ u64 dy_apply(u64 a, u64 b, u64 acc, const LimbConst& lc) {
    if (OP == DY_MUL) return Arith::mul_var(a, b, lc);
    if (OP == DY_MUL_ADD) return add_mod(acc, Arith::mul_var(a, b, lc), lc.q);
    if (OP == DY_ADD) return add_mod(a, b, lc.q);
    if (OP == DY_SUB) return sub_mod(a, b, lc.q);
    return neg_mod(a, lc.q);
}

// b_period = 0: b is shaped like a; b_period = L: ONE RNS polynomial (a plaintext), broadcast over the residue polynomials of a (A7 multiply_plain:
// its L tiles stay in L2, the launch moves two polynomials per polynomial instead of three)
// NT: operands and result go around the Infinity Cache (chosen by the launcher when the launch touches more than the cache holds: +4-8 % there,
// slower below it, like the copy kernel)
template <class Arith, int OP, bool NT = false>
__global__ __launch_bounds__(256) void dyadic_kernel(u64* out, const u64* a, const u64* b, const LimbConst* lcs, int n_limbs, int n, int b_period = 0) {
    const size_t p = blockIdx.x;
    const LimbConst lc = lcs[p % (size_t)n_limbs];
    const U64x2* pa = reinterpret_cast<const U64x2*>(a + p * n);
    const U64x2* pb = reinterpret_cast<const U64x2*>(b + (b_period ? p % (size_t)b_period : p) * n);
    U64x2* po = reinterpret_cast<U64x2*>(out + p * n);
    const int nv = n >> 1;
    constexpr int UN = 4;
    for (int base = threadIdx.x; base < nv; base += 256 * UN) {
        U64x2 va[UN], vb[UN], vc[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int i = base + u * 256;
            if (i < nv) {
                va[u] = ld_vec<NT>(pa + i);
                if (OP != DY_NEG) vb[u] = b_period ? pb[i] : ld_vec<NT>(pb + i);   // a broadcast plaintext is re-read: it stays cached
                if (OP == DY_MUL_ADD) vc[u] = ld_vec<NT>(po + i);
            }
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int i = base + u * 256;
            if (i < nv) {
                U64x2 r;
                r.a = dy_apply<Arith, OP>(va[u].a, vb[u].a, vc[u].a, lc);
                r.b = dy_apply<Arith, OP>(va[u].b, vb[u].b, vc[u].b, lc);
                st_vec<NT>(po + i, r);
            }
        }
    }
}

// The practical HBM ceiling the transforms are read against ("also report a measured device-copy bandwidth"):
// a plain copy with the streaming kernels' access shape - 16 bytes per lane, 4 KiB-contiguous per wave instruction, eight
// independent loads in flight per thread, one 32 KiB tile (a residue polynomial at N = 4096) per workgroup.
template <bool NT>   // NT: non-temporal loads and stores (a stream far beyond the 256 MiB Infinity Cache gains from not allocating there)
__global__ __launch_bounds__(256) void copy_kernel(U64x2* __restrict__ dst, const U64x2* __restrict__ src, size_t n_vec) {
    const size_t base = (size_t)blockIdx.x * 2048 + threadIdx.x;
    if ((size_t)blockIdx.x * 2048 + 2048 <= n_vec) {   // whole tile (workgroup-uniform)
        U64x2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (NT) { v[u].a = __builtin_nontemporal_load(&src[base + u * 256].a); v[u].b = __builtin_nontemporal_load(&src[base + u * 256].b); }
            else v[u] = src[base + u * 256];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (NT) { __builtin_nontemporal_store(v[u].a, &dst[base + u * 256].a); __builtin_nontemporal_store(v[u].b, &dst[base + u * 256].b); }
            else dst[base + u * 256] = v[u];
        }
    } else {
        for (size_t i = base; i < n_vec; i += 256) dst[i] = src[i];
    }
}

}  // namespace dpfhe
