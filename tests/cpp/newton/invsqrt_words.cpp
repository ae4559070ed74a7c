// The words ApproxInvSqrt::apply gives on TRANSPARENT inputs - ciphertexts (c0, 0) whose c0 hold the residues of known integer polynomials - for
// tests/test_gpu_invsqrt_words.py, which compares them word for word with the integer model of tests/invsqrt_model.py (with c1 = 0 every relinearisation
// digit is zero, every division by P is exact and the Newton steps are a deterministic integer function of their inputs).
//   invsqrt_words <case file> <output file>
// The case file (little-endian 64-bit words, doubles by their bits), written by the Python test:
//   magic "AISW1", log2 N, L, moduli[L], psi[L], P, psi_P, T, K, v_scale, guess_scale, c0_v[T][L][N], c0_y[T][L][N].
// Level r runs on the context of the first L - r limbs with its own key switcher (same secret, same P); L >= 2 K + 1.
// It prints one line
//   iterations K depth E scales <hex double s_0 .. s_K> weights <w_0 .. w_{K-1}>
// and writes the output words [T][2][L - 2 K][N] to the output file.  Exit code 0 = written.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "deeppowers/fhe.hpp"

using namespace deeppowers::fhe;

int main(int argc, char** argv) {
    if (argc != 3) { std::printf("usage: invsqrt_words <case file> <output file>\n"); return 2; }
    std::vector<uint64_t> w;
    {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) { std::printf("FAIL cannot read %s\n", argv[1]); return 2; }
        std::fseek(f, 0, SEEK_END);
        const long bytes = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        w.resize(bytes > 0 ? (size_t)bytes / 8 : 0);
        const size_t got = std::fread(w.data(), 8, w.size(), f);
        std::fclose(f);
        if (bytes <= 0 || bytes % 8 || got != w.size()) { std::printf("FAIL %s: not a whole number of words\n", argv[1]); return 2; }
    }
    size_t at = 0;
    auto u = [&]() -> uint64_t { return at < w.size() ? w[at++] : 0; };
    auto dbl = [&]() { const uint64_t v = u(); double x; std::memcpy(&x, &v, 8); return x; };
    if (u() != 0x3157534941ull) { std::printf("FAIL %s: not a case file\n", argv[1]); return 2; }
    FheParams p;
    p.log2_n = (uint32_t)u();
    const size_t L = (size_t)u();
    if (p.log2_n < 8 || p.log2_n > 16 || L < 3 || L > 16) { std::printf("FAIL case header\n"); return 2; }
    for (size_t l = 0; l < L; ++l) p.moduli.push_back(u());
    for (size_t l = 0; l < L; ++l) p.psi.push_back(u());
    const uint64_t special = u(), special_psi = u();
    const size_t T = (size_t)u(), K = (size_t)u();
    const double v_scale = dbl(), guess_scale = dbl();
    if (T == 0 || T > 64 || K < 1 || L < 2 * K + 1) { std::printf("FAIL case header\n"); return 2; }
    const size_t N = p.n();
    if (at > w.size() || w.size() - at != 2 * T * L * N) { std::printf("FAIL case body: c0_v and c0_y need %zu words\n", 2 * T * L * N); return 2; }
    const uint64_t* c0_v = w.data() + at;
    const uint64_t* c0_y = c0_v + T * L * N;

    try {
        std::vector<FheParams> level(1, p);
        for (size_t r = 0; r < 2 * K; ++r) level.push_back(level.back().drop_last_limb());
        std::vector<std::unique_ptr<Context>> ctx;
        for (const FheParams& q : level) ctx.emplace_back(new Context(q, 0));
        KeyGenerator kg(*ctx[0], TestSeed{11});
        std::vector<std::unique_ptr<SecretKey>> sk;
        std::vector<std::unique_ptr<HybridKeySwitcher>> hks;
        std::vector<HybridKeySwitcher*> levels;
        for (size_t r = 0; r < 2 * K; ++r) {
            sk.emplace_back(new SecretKey(*ctx[r], kg.secret_key().coefficients()));
            hks.emplace_back(new HybridKeySwitcher(*ctx[r], *sk[r], special, special_psi, TestSeed{12 + r}));
            levels.push_back(hks.back().get());
        }
        ApproxInvSqrt inv(levels, *ctx[2 * K], v_scale, guess_scale);
        Ciphertext v(*ctx[0], 2, T), y0(*ctx[0], 2, T), y(*ctx[2 * K], 2, T);
        auto transparent = [&](const uint64_t* c0, Ciphertext& ct) {
            std::vector<uint64_t> host(T * 2 * L * N, 0);
            for (size_t t = 0; t < T; ++t) std::memcpy(&host[(2 * t) * L * N], c0 + t * L * N, L * N * 8);
            ct.copy_from_host(host.data());
        };
        transparent(c0_v, v);
        transparent(c0_y, y0);
        inv.apply(v, y0, y);
        ctx[0]->synchronize();
        if (y.is_ntt()) { std::printf("FAIL the output is flagged NTT\n"); return 1; }
        std::printf("iterations %zu depth %zu scales", inv.iterations(), inv.depth());
        for (size_t n = 0; n <= K; ++n) std::printf(" %a", inv.scale(n));
        std::printf(" weights");
        for (size_t n = 0; n < K; ++n) std::printf(" %lld", (long long)inv.weight(n));
        std::printf("\n");
        std::vector<uint64_t> out(y.words());
        y.copy_to_host(out.data());
        FILE* f = std::fopen(argv[2], "wb");
        if (!f || std::fwrite(out.data(), 8, out.size(), f) != out.size()) { std::printf("FAIL cannot write %s\n", argv[2]); return 1; }
        std::fclose(f);
        std::printf("words %zu\n", out.size());
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    std::printf("inverse square root words written\n");
    return 0;
}
