// fhe_internal.h - private to the facade's units (fhe_*.cpp): error plumbing, the one place a Context's handle becomes a dpfhe_ctx*, and the few functions
// one unit defines for another.  Nothing here is part of the library's surface: namespace detail has hidden visibility.
#pragma once
#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>

#include <memory>
#include <string>

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

struct Sampler;   // fhe_sampler.h

// fhe_keys.cpp, also for fhe_keyswitch.cpp.  NTT(sigma_g(s)) on ctx - the target of the switching key for Galois element g:
PolyBuffer galois_target_ntt(const Context& ctx, const std::vector<int8_t>& secret_coefficients, uint32_t galois_elt);
// key_j = (-(a_j s) + e_j + g_j * target, a_j) for the first n_digits limbs (0 = all), everything in the NTT domain; with n_digits < L (hybrid) only the
// data limbs are digits and d_target_ntt must already carry the factor P.  seed_out != null: a_j = expand(*seed_out, j, ., 1), the seed drawn from rng first.
void make_switch_key(const Context& ctx, const SecretKey& sk, Sampler& rng, const uint64_t* d_target_ntt, PolyBuffer& out, size_t n_digits, Seed* seed_out);

}  // namespace detail
}  // namespace fhe
}  // namespace deeppowers
