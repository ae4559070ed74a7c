// fhe_internal.h - private to the facade's units (fhe_*.cpp): error plumbing, the one place a Context's handle becomes a dpfhe_ctx*, and the few functions
// one unit defines for another.  Nothing here is part of the library's surface: namespace detail has hidden visibility.
#pragma once
#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "deeppowers/fhe.hpp"
#include "dpfhe.h"

namespace deeppowers {
namespace fhe {
namespace detail __attribute__((visibility("hidden"))) {

[[noreturn]] inline void raise(int code, const char* what) {
    std::string msg = std::string(what) + ": " + dpfhe_last_error();
    if (msg.size() <= std::string(what).size() + 2) msg = std::string(what) + ": " + dpfhe_strerror(code);
    throw Exception(static_cast<ErrorCode>(code), msg);
}
inline void check(int code, const char* what) {
    if (code != DPFHE_SUCCESS) raise(code, what);
}
// like the reference's HAL device (src/core/hal/cuda/cuda_device.cpp:9-16): runtime errors become exceptions
inline void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess)
        throw Exception(e == hipErrorOutOfMemory ? ErrorCode::OUT_OF_MEMORY : ErrorCode::DEVICE_ERROR, std::string(what) + ": " + hipGetErrorString(e));
}
inline dpfhe_ctx* handle_of(const Context& ctx) { return static_cast<dpfhe_ctx*>(ctx.handle()); }
template <class T>
T* device_alloc(int device_id, size_t count) {   // the caller owns it (hipFree)
    hip_check(hipSetDevice(device_id), "hipSetDevice");
    void* p = nullptr;
    hip_check(hipMalloc(&p, count * sizeof(T)), "hipMalloc");
    return static_cast<T*>(p);
}

// a scratch buffer that belongs to an object: grown (by make(batch)) when a larger batch arrives, never shrunk, so steady-state calls allocate nothing
template <class T, class Make>
T& grow_scratch(std::unique_ptr<T>& slot, size_t batch, Make make) {
    if (!slot || slot->batch() < batch) slot.reset(make(batch));
    return *slot;
}

// signed weights |v| < 2^62 as canonical residues, [rows.size()][L] over p's limbs (a negative v is q - (|v| mod q), 0 stays 0); row `constant_row` is a
// constant at the OUTPUT scale of the rescale that follows and carries the factor q_last
inline std::vector<uint64_t> signed_weight_rows(const FheParams& p, const std::vector<int64_t>& rows, size_t constant_row) {
    const size_t L = p.n_limbs();
    std::vector<uint64_t> w(rows.size() * L);
    for (size_t row = 0; row < rows.size(); ++row) {
        const int64_t v = rows[row];
        for (size_t l = 0; l < L; ++l) {
            const uint64_t q = p.moduli[l];
            uint64_t m = (uint64_t)(v < 0 ? -v : v) % q;
            if (row == constant_row) m = (uint64_t)((unsigned __int128)m * (p.moduli.back() % q) % q);
            w[row * L + l] = (v < 0 && m) ? q - m : m;
        }
    }
    return w;
}

// the level drop of a coefficient-domain ciphertext: the first limbs of each of its `polys` polynomials ARE the ciphertext on dst_ctx (same scale), copied on `stream`
inline void keep_first_limbs(uint64_t* dst, const Context& dst_ctx, const uint64_t* src, const Context& src_ctx, size_t polys, Stream* stream) {
    const size_t n = src_ctx.params().n(), src_row = src_ctx.params().n_limbs() * n * 8, dst_row = dst_ctx.params().n_limbs() * n * 8;
    hip_check(hipMemcpy2DAsync(dst, dst_row, src, src_row, dst_row, polys, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)), "hipMemcpy2DAsync D2D");
}

// ---- the vocabulary of the approximate family's error bounds (fhe.hpp states each bound in these terms).  A helper wraps only what the bounds evaluate as a
// unit, in the order they always did: the returned doubles are pinned bit for bit (tests/test_approx_bounds_cpu.py).
struct BoundUnits {
    double N, H, u, u8;   // ring degree; (N + 1) / 2, a rounding's worst slot error over N; float64's unit roundoff; the decode transform's 8 log2(N) u
    explicit BoundUnits(uint32_t log2_n) : N(std::ldexp(1.0, (int)log2_n)), H((N + 1) / 2), u(std::ldexp(1.0, -53)), u8(8.0 * log2_n * u) {}
};
inline uint64_t max_modulus(const std::vector<uint64_t>& moduli, size_t count) {   // of the first `count`
    uint64_t qmax = 0;
    for (size_t j = 0; j < count; ++j) qmax = std::max(qmax, moduli[j]);
    return qmax;
}
// K = 21 Ld N rho, rho = qmax / P: a hybrid key switch's error per coefficient
inline double keyswitch_term(double Ld, double N, double rho) { return 21.0 * Ld * N * rho; }
inline double keyswitch_term(double Ld, double N, uint64_t qmax, uint64_t P) { return keyswitch_term(Ld, N, (double)qmax / (double)P); }
// level r (one special prime each) works on the first L0 - r data limbs: drop[r] = the prime its rescale drops, K[r] = its key-switch term
struct LevelLadder {
    std::vector<uint64_t> drop;
    std::vector<double> K;
};
inline LevelLadder level_ladder(const std::vector<uint64_t>& data_moduli, const std::vector<uint64_t>& special_primes, double N) {
    LevelLadder t;
    for (size_t r = 0; r < special_primes.size(); ++r) {
        const size_t Lr = data_moduli.size() - r;
        t.drop.push_back(data_moduli[Lr - 1]);
        t.K.push_back(keyswitch_term((double)Lr, N, max_modulus(data_moduli, Lr), special_primes[r]));
    }
    return t;
}

struct Sampler;   // fhe_sampler.h

// fhe_keys.cpp, also for fhe_keyswitch.cpp.  NTT(sigma_g(s)) on ctx - the target of the switching key for Galois element g:
PolyBuffer galois_target_ntt(const Context& ctx, const std::vector<int8_t>& secret_coefficients, uint32_t galois_elt);
// key_j = (-(a_j s) + e_j + g_j * target, a_j) for the first n_digits limbs (0 = all), everything in the NTT domain; with n_digits < L (hybrid) only the
// data limbs are digits and d_target_ntt must already carry the factor P.  seed_out != null: a_j = expand(*seed_out, j, ., 1), the seed drawn from rng first.
void make_switch_key(const Context& ctx, const SecretKey& sk, Sampler& rng, const uint64_t* d_target_ntt, PolyBuffer& out, size_t n_digits, Seed* seed_out);

}  // namespace detail
}  // namespace fhe
}  // namespace deeppowers
