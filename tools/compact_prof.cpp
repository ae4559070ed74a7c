// compact_prof.cpp - cost of compact result ciphertexts (dpfhe_compact) and what they save on the device-to-host copy.
//   (1) the kernel alone at N = 4096 / L = 4 / 8192 items, N = 16384 / L = 6 / 256 items and N = 8192 / L = 10 / 1024 items, widths
//       CompactCiphertext::recommended_bits(log2_n, 65537): time per launch, bytes moved (16 L N read + the record written per item) and the share of
//       the HBM peak (8 TB/s);
//   (2) per case, the device-event time of copy_to_host of the full words against compact + copy_to_host of the records.
// Build: g++ -O2 -std=c++17 -Iinclude tools/compact_prof.cpp -Ldeeppowers_amd -ldpfhe_api -ldpfhe_hip -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,...
// Run it under rocprofv3 --kernel-trace --stats for the kernel's own durations (compact_kernel<L>, one dispatch size per case).
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <vector>

#include <deeppowers/fhe.hpp>

using namespace deeppowers::fhe;

namespace {
const uint64_t T_MOD = 65537;
uint64_t g_seed = 11;
uint64_t rnd(uint64_t m) { g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull; return (g_seed >> 33) % m; }

template <class F>
float event_ms(int reps, F f) {   // mean device time of f() over reps calls (after one warm-up)
    hipEvent_t a, b;
    (void)hipEventCreate(&a); (void)hipEventCreate(&b);
    f();
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(a, nullptr);
    for (int i = 0; i < reps; ++i) f();
    (void)hipEventRecord(b, nullptr);
    (void)hipEventSynchronize(b);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, a, b);
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    return ms / reps;
}

void run(const FheParams& p, size_t batch, const char* name) {
    const size_t n = p.n(), L = p.n_limbs();
    Context ctx(p, 0);
    Evaluator ev(ctx);
    Ciphertext ct(ctx, 2, batch);
    {   // canonical random residues (the kernel's work does not depend on them, but keep the input honest)
        std::vector<uint64_t> h(ct.words());
        for (size_t i = 0; i < h.size(); ++i) h[i] = rnd(p.moduli[(i / n) % L]);
        ct.copy_from_host(h.data());
    }
    const auto w = CompactCiphertext::recommended_bits(p.log2_n, T_MOD);
    CompactCiphertext cc(ctx, batch, w.first, w.second);
    const float ms = event_ms(20, [&] { ev.compact(ct, cc); });
    const double bytes = 16.0 * L * n * batch + (double)cc.bytes();
    std::printf("%s: %zu items, widths (%u, %u): compact %.3f ms per launch, %.3f GB moved, %.2f TB/s, %.1f %% of 8 TB/s\n", name, batch, w.first, w.second, ms,
                bytes / 1e9, bytes / (ms * 1e-3) / 1e12, 100.0 * bytes / (ms * 1e-3) / 8e12);
    std::vector<uint64_t> full(ct.words());
    std::vector<uint8_t> rec(cc.bytes());
    const float full_ms = event_ms(5, [&] { ct.copy_to_host(full.data()); });
    const float comp_ms = event_ms(5, [&] { ev.compact(ct, cc); cc.copy_to_host(rec.data()); });
    std::printf("%s: copy_to_host of the full words %.3f ms (%.1f MB) | compact + copy_to_host of the records %.3f ms (%.1f MB) -> %.1fx less time, %.1fx fewer bytes\n",
                name, full_ms, 8.0 * ct.words() / 1e6, comp_ms, cc.bytes() / 1e6, full_ms / comp_ms, 8.0 * ct.words() / cc.bytes());
}
}  // namespace

int main() {
    try {
        run(FheParams::n4096_l4(), 8192, "N=4096 L=4");
        run(FheParams::n16384(6), 256, "N=16384 L=6");
        run(FheParams::n8192(10), 1024, "N=8192 L=10");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    return 0;
}
