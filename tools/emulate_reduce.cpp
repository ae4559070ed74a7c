// emulate_reduce.cpp - CPU emulation of reduce_thin_kernel's per-thread loop (TEST INFRASTRUCTURE, like emulate.cpp).
// Runs deeppowers_amd/csrc/reduce_thin.h thin_sum - the very code the kernel runs - for every thread of one 2 * threads-word
// chunk and every batch split, with the split bounds the launcher passes, and adds the canonical partials the way the kernel's
// atomics do.  The wrap-around counter of the lazy sums is armed.  Built by tests/test_reduce_thin_cpu.py (g++), never shipped.
#define DPFHE_EMU_CHECK 1
#include "../deeppowers_amd/csrc/reduce_thin.h"

namespace dpfhe {
long g_emu_overflows = 0;
}
using namespace dpfhe;

extern "C" long emu_reduce_overflows() { return g_emu_overflows; }

// in: [count][2 * threads] canonical words of one limb; out: [2 * threads] = the sum of the at most 15 canonical partials (what
// reduce_final_kernel then canonicalises).  returns 0, or 2000 on bad arguments.
extern "C" int emu_reduce_thin(u64 q, const u64* in, size_t count, unsigned nsplit, unsigned threads, u64* out) {
    if (!in || !out || count == 0 || nsplit == 0 || nsplit > 15 || q >= (1ull << 60) || (1ull << 60) - q >= (1ull << 24)) return 2000;
    LimbConst lc{};
    lc.q = q;
    lc.d = (1ull << 60) - q;
    const size_t words = 2 * (size_t)threads, per = count / nsplit;
    const unsigned rem = (unsigned)(count % nsplit);
    for (size_t w = 0; w < words; ++w) out[w] = 0;
    for (unsigned split = 0; split < nsplit; ++split) {
        const size_t lo = split * per + (split < rem ? split : rem), hi = (split + 1) * per + (split + 1 < rem ? split + 1 : rem);
        for (unsigned t = 0; t < threads; ++t) {
            const U64x2 s = thin_sum([&](size_t it) { return U64x2{in[it * words + 2 * t], in[it * words + 2 * t + 1]}; }, lo, hi, lc);
            if (s.a >= q || s.b >= q) return -1;   // a partial must be canonical: 15 of them are what the final pass can take
            if (hi > lo) { out[2 * t] += s.a; out[2 * t + 1] += s.b; }
        }
    }
    return 0;
}
