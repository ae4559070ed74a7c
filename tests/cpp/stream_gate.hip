// Test-only: a bounded gate on a stream (tests/stream_gate.py, tests/cpp/test_stream_api.cpp).
//
// stream_gate_enqueue(stream, ticks, max_iters) launches ONE workgroup of ONE thread that reads the real-time counter (wall_clock64(): 100 MHz on gfx950)
// until `ticks` have passed or `max_iters` loop turns are done, sleeping between reads.  It takes no pointer and touches no memory.  Whatever the clock
// does, the loop ends after max_iters turns; the host side rejects requests beyond kMaxTicks / kMaxIters, so a gate never holds a stream for more than a
// fraction of a second (one turn is a 2048-cycle sleep and one counter read: about a microsecond).
//
// The two stream helpers create and destroy the NON-BLOCKING stream the gated tests run on, on the same HIP runtime this library is linked to.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {
constexpr uint64_t kMaxTicks = 25000000;   // 0.25 s of the 100 MHz counter
constexpr uint64_t kMaxIters = 200000;

__global__ void stream_gate_kernel(uint64_t ticks, uint64_t max_iters) {
    const uint64_t t0 = wall_clock64();
    for (uint64_t i = 0; i < max_iters; ++i) {
        if (static_cast<uint64_t>(wall_clock64()) - t0 >= ticks) break;
        __builtin_amdgcn_s_sleep(32);
    }
}
}  // namespace

extern "C" int stream_gate_enqueue(void* stream, uint64_t ticks, uint64_t max_iters) {
    if (ticks > kMaxTicks || max_iters > kMaxIters) return -1;
    hipLaunchKernelGGL(stream_gate_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), ticks, max_iters);
    return static_cast<int>(hipGetLastError());
}

extern "C" int stream_gate_stream_create(void** out) {
    hipStream_t s = nullptr;
    const hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    *out = s;
    return static_cast<int>(e);
}

extern "C" int stream_gate_stream_destroy(void* stream) { return static_cast<int>(hipStreamDestroy(static_cast<hipStream_t>(stream))); }
