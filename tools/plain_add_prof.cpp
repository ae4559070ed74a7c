// plain_add_prof.cpp - cost of exact plaintext addition (dpfhe_add_plain_scaled) alone and inside a biased PackedLinear::apply.
//   (1) 8192 two-component ciphertexts at N = 4096 / L = 4, in place, broadcast plaintext: time per launch and its share of the HBM peak
//       (16 bytes moved per c0 word: read + write);
//   (2) a biased 768 x 768 PackedLinear (GPT-2 small's attention projection) at 8 tokens on N = 8192 (5 data limbs) and N = 16384 (6 data limbs):
//       time of one apply() and of its bias addition alone (the same launch on the layer's output), both from device events.
// Build: g++ -O2 -std=c++17 -Iinclude tools/plain_add_prof.cpp -Ldeeppowers_amd -ldpfhe_api -ldpfhe_hip -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,...
// Run it under rocprofv3 --kernel-trace --stats for the kernel's own durations (add_plain_scaled_kernel, one dispatch size per case).
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <vector>

#include <deeppowers/fhe.hpp>

using namespace deeppowers::fhe;

namespace {
const uint64_t T_MOD = 65537;
uint64_t g_seed = 7;
uint64_t rnd(uint64_t m) { g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull; return (g_seed >> 33) % m; }

template <class F>
float event_ms(int reps, F f) {   // mean device time of f() over reps launches (after one warm-up)
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

void stream_case() {
    const FheParams p = FheParams::n4096_l4();
    const size_t batch = 8192, n = p.n(), L = p.n_limbs();
    Context ctx(p, 0);
    Evaluator ev(ctx);
    Ciphertext ct(ctx, 2, batch);   // contents irrelevant to the timing (the kernel reads and writes every c0 word whatever they hold)
    ExactPlaintext b(ctx, T_MOD, 1);
    std::vector<int64_t> coeffs(n);
    for (auto& v : coeffs) v = (int64_t)rnd(T_MOD);
    b.set_coefficients(coeffs.data());
    const float ms = event_ms(20, [&] { ev.add_plain_exact(ct, b, ct); });
    const double bytes = 16.0 * batch * L * n;
    std::printf("stream: 8192 items N=4096 L=4 in place: %.3f ms per launch, %.2f GB moved, %.2f TB/s, %.1f %% of 8 TB/s\n", ms, bytes / 1e9,
                bytes / (ms * 1e-3) / 1e12, 100.0 * bytes / (ms * 1e-3) / 8e12);
}

void layer_case(const FheParams& full, const char* name) {
    FheParams p = full;
    const uint64_t special = p.moduli.back(), special_psi = p.psi.back();
    p.moduli.pop_back(); p.psi.pop_back();
    const size_t n = p.n(), d = 768, T = 8;
    Context ctx(p, 0);
    Evaluator ev(ctx);
    KeyGenerator kg(ctx, TestSeed{1});
    Encryptor enc(ctx, kg.secret_key(), TestSeed{2});
    BatchEncoder be(ctx, T_MOD);
    HybridKeySwitcher hks(ctx, kg.secret_key(), special, special_psi, TestSeed{3});
    std::vector<uint64_t> W(d * d), bias(d), x(d), slots(n);
    for (auto& v : W) v = (T_MOD + rnd(255) - 127) % T_MOD;
    for (auto& v : bias) v = rnd(T_MOD);
    for (auto& v : x) v = (T_MOD + rnd(255) - 127) % T_MOD;
    PackedLinear lin(ctx, be, hks, W.data(), d, d, 1, bias.data());
    std::vector<int64_t> cx(T * n);
    lin.pack_input(x.data(), slots.data());
    for (size_t tk = 0; tk < T; ++tk) be.encode(slots.data(), &cx[tk * n]);
    Ciphertext ct(ctx, 2, T), cy(ctx, 2, lin.output_ciphertexts() * T);
    enc.encrypt_exact(cx.data(), T_MOD, ct);
    // the bias addition alone: the same launch apply() ends with (plaintext items = output ciphertexts)
    ExactPlaintext b(ctx, T_MOD, lin.output_ciphertexts());
    std::vector<int64_t> bc(lin.output_ciphertexts() * n);
    for (auto& v : bc) v = (int64_t)rnd(T_MOD);
    b.set_coefficients(bc.data());
    const float apply_ms = event_ms(5, [&] { lin.apply(ct, cy); });
    const float add_ms = event_ms(20, [&] { ev.add_plain_exact(cy, b, cy); });
    std::printf("layer %s: 768 x 768 biased PackedLinear, %zu tokens, %zu output ciphertext(s): apply %.3f ms, bias add %.4f ms = %.3f %% of apply\n", name, T,
                lin.output_ciphertexts(), apply_ms, add_ms, 100.0 * add_ms / apply_ms);
}
}  // namespace

int main() {
    try {
        stream_case();
        layer_case(FheParams::n8192(6), "N=8192 L=5");
        layer_case(FheParams::n16384(7), "N=16384 L=6");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    return 0;
}
