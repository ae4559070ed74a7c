// What the C++ facade's test programs (tests/cpp/*.cpp) share: failure counting, the two generators of test cases, a few helpers on facade objects and -
// for the programs that define FACADE_TEST_GATE before including this - the stream-gate protocol of tests/stream_gate.py.  Header-only C++17.  The rigs,
// the cases and the numerical bounds belong to each program.  Built through tests/cpp_build.py.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "deeppowers/fhe.hpp"

namespace facade_test {
using namespace deeppowers::fhe;

// ---- failure counting -------------------------------------------------------------------------------------------------------------------------------------
inline int failures = 0;
#define CHECK(cond)                                                                                                \
    do {                                                                                                           \
        if (!(cond)) { std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); ++facade_test::failures; }    \
    } while (0)
// a HIP runtime call that must succeed (the program includes <hip/hip_runtime_api.h> itself, or defines FACADE_TEST_GATE)
#define HIP(call)                                                                                                                                   \
    do {                                                                                                                                            \
        hipError_t e_ = (call);                                                                                                                     \
        if (e_ != hipSuccess) { std::printf("FAIL %s:%d  %s: %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_)); ++facade_test::failures; } \
    } while (0)

template <class F>
void expect_error(ErrorCode code, F f, const char* what) {
    try {
        f();
        std::printf("FAIL %s: no exception\n", what);
        ++failures;
    } catch (const Exception& e) {
        if (e.code() != code) { std::printf("FAIL %s: code %d (%s)\n", what, (int)e.code(), e.what()); ++failures; }
    }
}

// the end of main(): "<n> failures" and exit code 1, or the program's own OK line and 0
inline int finish(const char* ok_line) {
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("%s\n", ok_line);
    return 0;
}

// ---- generators: each program sets its own seed and keeps its own order of draws ---------------------------------------------------------------------
static const uint64_t T_MOD = 65537;

struct Lcg {
    uint64_t seed;
    uint64_t step() { return seed = seed * 6364136223846793005ull + 1442695040888963407ull; }
    uint64_t operator()(uint64_t m) { return (step() >> 33) % m; }                  // uniform below m
    uint64_t small8(uint64_t t = T_MOD) { return (t + (*this)(255) - 127) % t; }    // 8-bit quantised, centred, mod t
};

struct SplitMix64 {
    uint64_t state = 0;
    uint64_t next() {
        uint64_t z = (state += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    double unit() { return (double)(next() >> 11) * std::ldexp(1.0, -53); }          // uniform on [0, 1)
    double sym() { return (double)(next() >> 11) * std::ldexp(1.0, -52) - 1.0; }     // uniform on [-1, 1]
};

// ---- helpers ----------------------------------------------------------------------------------------------------------------------------------------------
inline std::vector<uint64_t> words(const PolyBuffer& b) {   // the buffer's device words
    std::vector<uint64_t> h(b.words());
    b.copy_to_host(h.data());
    return h;
}

inline uint64_t modpow(uint64_t b, uint64_t e, uint64_t q) {
    uint64_t r = 1;
    for (b %= q; e; e >>= 1) {
        if (e & 1) r = (uint64_t)((unsigned __int128)r * b % q);
        b = (uint64_t)((unsigned __int128)b * b % q);
    }
    return r;
}

// the chain primes of FheParams::n8192 seen at ring degree 2^log2n (psi raised to the power 8192 / N); the last one is returned as the special prime
inline FheParams ring(unsigned log2n, size_t data_limbs, uint64_t& special, uint64_t& special_psi) {
    FheParams p = FheParams::n8192(data_limbs + 1);
    const size_t n = (size_t)1 << log2n;
    for (size_t l = 0; l < p.moduli.size(); ++l) p.psi[l] = modpow(p.psi[l], 8192 / n, p.moduli[l]);
    special = p.moduli.back(); special_psi = p.psi.back();
    p.log2_n = log2n; p.moduli.pop_back(); p.psi.pop_back();
    return p;
}

// y = W x + b mod t (b may be null)
inline std::vector<uint64_t> affine(const std::vector<uint64_t>& W, const uint64_t* b, size_t rows, size_t cols, const uint64_t* x, uint64_t t) {
    std::vector<uint64_t> y(rows);
    for (size_t r = 0; r < rows; ++r) {
        unsigned __int128 acc = b ? b[r] : 0;
        for (size_t c = 0; c < cols; ++c) acc += (unsigned __int128)W[r * cols + c] * x[c];
        y[r] = (uint64_t)(acc % t);
    }
    return y;
}

}  // namespace facade_test

// ---- the gate ---------------------------------------------------------------------------------------------------------------------------------------------
#ifdef FACADE_TEST_GATE
#include <hip/hip_runtime_api.h>

#include <chrono>
#include <functional>

extern "C" int stream_gate_enqueue(void* stream, uint64_t ticks, uint64_t max_iters);
extern "C" int stream_gate_stream_create(void** out);
extern "C" int stream_gate_stream_destroy(void* stream);

namespace facade_test {

struct Late { void* dst; const void* zero; const void* real; size_t bytes; };   // an input buffer: zeros during the warm-up and the gate, the real words behind it
struct Out { void* p; size_t bytes; };                                          // an output buffer: wiped behind the gate
inline Late late(PolyBuffer& dst, const PolyBuffer& zero, const PolyBuffer& real) { return Late{dst.data(), zero.data(), real.data(), dst.words() * 8}; }
inline Out out_of(PolyBuffer& b) { return Out{b.data(), b.words() * 8}; }

inline std::vector<uint8_t> download(const std::vector<Out>& outs) {
    size_t total = 0;
    for (auto& o : outs) total += o.bytes;
    std::vector<uint8_t> h(total);
    size_t at = 0;
    for (auto& o : outs) { HIP(hipMemcpy(h.data() + at, o.p, o.bytes, hipMemcpyDeviceToHost)); at += o.bytes; }
    return h;
}

// One non-blocking stream S for the life of the object, the gate length G in seconds, and what the gated calls added up to.
struct Gate {
    void* S = nullptr;
    double G;
    double slowest = 0;
    std::string slowest_what;
    int gated_calls = 0;

    explicit Gate(double seconds) : G(seconds) { if (stream_gate_stream_create(&S) != 0) S = nullptr; }
    ~Gate() { if (S) stream_gate_stream_destroy(S); }
    Gate(const Gate&) = delete;
    Gate& operator=(const Gate&) = delete;
    bool ok() const { return S != nullptr; }

    // The protocol of tests/stream_gate.py for one facade call on S:
    //   warm-up on the zero inputs on S, synchronise;  gate on S, event E, then the real inputs arrive by hipMemcpyAsync on S and every output buffer is
    //   wiped on S;  the call, timed on the host;  hipEventQuery(E) must still be hipErrorNotReady (the call waited for neither S nor the device) and the call
    //   must have taken at most G / 4;  synchronise S;  the result must differ from the warm-up's.  What the result must BE is the caller's to check.
    // A launch or copy on another stream runs during the gate, on the zero inputs or on the warm-up's intermediates, or is wiped: the result is wrong.
    // Without outputs the first input is the result (an in-place method).  Without inputs (a case that cannot take them late) the inputs are in place from
    // the start, and the wipe alone separates the result from the warm-up's.
    // enqueue_only = false (a method documented to synchronise `stream`): the call must return only after S has run.
    // Returns the host time of the call in seconds.
    double gated(const char* what, const std::vector<Late>& ins, const std::vector<Out>& outs, const std::function<void(Stream*)>& call, bool enqueue_only = true) {
        hipStream_t hs = static_cast<hipStream_t>(S);
        const std::vector<Out> result = outs.empty() ? std::vector<Out>{{ins.at(0).dst, ins.at(0).bytes}} : outs;
        for (auto& i : ins) HIP(hipMemcpy(i.dst, i.zero, i.bytes, hipMemcpyDeviceToDevice));
        HIP(hipDeviceSynchronize());
        call(S);
        HIP(hipStreamSynchronize(hs));
        const std::vector<uint8_t> warm = download(result);
        for (auto& i : ins) HIP(hipMemcpy(i.dst, i.zero, i.bytes, hipMemcpyDeviceToDevice));   // (an in-place method changed its input)
        HIP(hipDeviceSynchronize());
        hipEvent_t E;
        HIP(hipEventCreateWithFlags(&E, hipEventDisableTiming));
        const uint64_t ticks = (uint64_t)(G * 1e8);
        CHECK(stream_gate_enqueue(S, ticks, 4 * ticks / 100) == 0);
        HIP(hipEventRecord(E, hs));
        for (auto& i : ins) HIP(hipMemcpyAsync(i.dst, i.real, i.bytes, hipMemcpyDeviceToDevice, hs));
        for (auto& o : outs) HIP(hipMemsetAsync(o.p, 0xA5, o.bytes, hs));
        const auto t0 = std::chrono::steady_clock::now();
        call(S);
        const double t_enqueue = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const hipError_t q = hipEventQuery(E);
        if (enqueue_only) {
            if (q != hipErrorNotReady) { std::printf("FAIL %s: synchronised - the gate on S had ended when the call returned (t_enqueue %.3f ms, G %.1f ms)\n", what, t_enqueue * 1e3, G * 1e3); ++failures; }
            else if (t_enqueue > G / 4) { std::printf("FAIL %s: inconclusive - t_enqueue %.3f ms > G / 4, G %.1f ms\n", what, t_enqueue * 1e3, G * 1e3); ++failures; }
            else if (t_enqueue > slowest) { slowest = t_enqueue; slowest_what = what; }
        } else if (q != hipSuccess) {
            std::printf("FAIL %s: documented to synchronise `stream`, but S had not run when it returned\n", what);
            ++failures;
        }
        (void)hipGetLastError();
        HIP(hipStreamSynchronize(hs));
        HIP(hipDeviceSynchronize());
        HIP(hipEventDestroy(E));
        if (!ins.empty() && download(result) == warm) {
            std::printf("FAIL %s: the result equals the warm-up's on zero inputs: the case cannot see a launch that ran too early\n", what);
            ++failures;
        }
        ++gated_calls;
        return t_enqueue;
    }
};

}  // namespace facade_test
#endif  // FACADE_TEST_GATE
