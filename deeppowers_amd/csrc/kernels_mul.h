// kernels_mul.h - the multiply at ring degrees above 8192 (device).  Included by cabi_mul.hip only.
//
// The fused multiply kernels of kernels.h keep whole polynomials in one workgroup's registers and LDS, which stops at
// N = 8192 (one 1024-thread workgroup at N = 16384 has 128 VGPRs per thread; four polynomials of 16 words per thread do not fit).
// Above, the same operation is COMPOSED (cabi_mul.hip: ct_mul_composed) from the batched transforms of kernels.h / ntt_top.h and the
// streaming kernel below: one HBM pass, 16 bytes per lane, one workgroup per 512-word chunk of one residue polynomial.  All words canonical
// in and out; results equal the fused kernels' (tests/test_gpu_parity.py (test_large_rings_multiply_and_key_switch_composed_behind_the_c_abi and the slicing test)).
#pragma once
#include <hip/hip_runtime.h>

#include "modarith.h"
#include "workmap.h"

namespace dpfhe {

// (a0, a1) (x) (b0, b1) -> (a0 b0, a0 b1 + a1 b0, a1 b1), NTT domain.  a2, b2: [batch][2][L][N]; out3: [batch][3][L][N].
template <class Arith>
__global__ __launch_bounds__(256) void tensor3_kernel(u64* __restrict__ out3, const u64* __restrict__ a2, const u64* __restrict__ b2, const LimbConst* lcs,
                                                      int n_limbs, int n, int chunks) {
    const ChunkWork wk = chunk_work(blockIdx.x, chunks, n_limbs);
    const int chunk = wk.chunk, limb = wk.limb;
    const size_t pair = wk.poly;
    const int w0 = chunk * 512 + threadIdx.x * 2;
    if (w0 >= n) return;
    const LimbConst lc = lcs[limb];
    const size_t poly = (size_t)n_limbs * n, off = (size_t)limb * n + w0;
    const U64x2 a0 = *reinterpret_cast<const U64x2*>(a2 + (pair * 2 + 0) * poly + off), a1 = *reinterpret_cast<const U64x2*>(a2 + (pair * 2 + 1) * poly + off);
    const U64x2 b0 = *reinterpret_cast<const U64x2*>(b2 + (pair * 2 + 0) * poly + off), b1 = *reinterpret_cast<const U64x2*>(b2 + (pair * 2 + 1) * poly + off);
    U64x2 d0, d1, d2;
    d0.a = Arith::mul_var(a0.a, b0.a, lc); d0.b = Arith::mul_var(a0.b, b0.b, lc);
    d1.a = add_mod(Arith::mul_var(a0.a, b1.a, lc), Arith::mul_var(a1.a, b0.a, lc), lc.q);
    d1.b = add_mod(Arith::mul_var(a0.b, b1.b, lc), Arith::mul_var(a1.b, b0.b, lc), lc.q);
    d2.a = Arith::mul_var(a1.a, b1.a, lc); d2.b = Arith::mul_var(a1.b, b1.b, lc);
    *reinterpret_cast<U64x2*>(out3 + (pair * 3 + 0) * poly + off) = d0;
    *reinterpret_cast<U64x2*>(out3 + (pair * 3 + 1) * poly + off) = d1;
    *reinterpret_cast<U64x2*>(out3 + (pair * 3 + 2) * poly + off) = d2;
}

}  // namespace dpfhe
