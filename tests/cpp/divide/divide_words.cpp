// The words ApproxDivide::apply gives on TRANSPARENT inputs - ciphertexts (c0, 0) whose c0 hold the residues of known integer polynomials - for
// tests/test_gpu_divide_words.py, which compares them word for word with the integer model of tests/divide_model.py (with c1 = 0 every relinearisation
// digit is zero, every division by P is exact and the Goldschmidt steps are a deterministic integer function of their inputs).
//   divide_words <case file> <output file>
// The case file (little-endian 64-bit words, doubles by their bits), written by the Python test:
//   magic "ADVW1", log2 N, L, moduli[L], psi[L], P, psi_P, G, T, K, num_scale, den_scale, c0_num[G * T][L][N], c0_den[G][L][N].
// Level n runs on the context of the first L - n limbs with its own key switcher (same secret, same P); L >= K + 1.
// It prints one line
//   iterations K depth E den_scales <hex double sigma_0 .. sigma_K> num_scales <hex double nu_0 .. nu_K> kappas <kappa_0 .. kappa_{K-1}>
// and writes the output words [G * T][2][L - K][N] to the output file.  Exit code 0 = written.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "deeppowers/fhe.hpp"

using namespace deeppowers::fhe;

int main(int argc, char** argv) {
    if (argc != 3) { std::printf("usage: divide_words <case file> <output file>\n"); return 2; }
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
    if (u() != 0x3157564441ull) { std::printf("FAIL %s: not a case file\n", argv[1]); return 2; }
    FheParams p;
    p.log2_n = (uint32_t)u();
    const size_t L = (size_t)u();
    if (p.log2_n < 8 || p.log2_n > 16 || L < 2 || L > 16) { std::printf("FAIL case header\n"); return 2; }
    for (size_t l = 0; l < L; ++l) p.moduli.push_back(u());
    for (size_t l = 0; l < L; ++l) p.psi.push_back(u());
    const uint64_t special = u(), special_psi = u();
    const size_t G = (size_t)u(), T = (size_t)u(), K = (size_t)u();
    const double num_scale = dbl(), den_scale = dbl();
    if (G == 0 || G > 64 || T == 0 || T > 64 || K < 1 || L < K + 1) { std::printf("FAIL case header\n"); return 2; }
    const size_t N = p.n();
    if (at > w.size() || w.size() - at != (G * T + G) * L * N) { std::printf("FAIL case body: c0_num and c0_den need %zu words\n", (G * T + G) * L * N); return 2; }
    const uint64_t* c0_num = w.data() + at;
    const uint64_t* c0_den = c0_num + G * T * L * N;

    try {
        std::vector<FheParams> level(1, p);
        for (size_t r = 0; r < K; ++r) level.push_back(level.back().drop_last_limb());
        std::vector<std::unique_ptr<Context>> ctx;
        for (const FheParams& q : level) ctx.emplace_back(new Context(q, 0));
        KeyGenerator kg(*ctx[0], TestSeed{11});
        std::vector<std::unique_ptr<SecretKey>> sk;
        std::vector<std::unique_ptr<HybridKeySwitcher>> hks;
        std::vector<HybridKeySwitcher*> levels;
        for (size_t r = 0; r < K; ++r) {
            sk.emplace_back(new SecretKey(*ctx[r], kg.secret_key().coefficients()));
            hks.emplace_back(new HybridKeySwitcher(*ctx[r], *sk[r], special, special_psi, TestSeed{12 + r}));
            levels.push_back(hks.back().get());
        }
        ApproxDivide div(levels, *ctx[K], num_scale, den_scale);
        Ciphertext num(*ctx[0], 2, G * T), den(*ctx[0], 2, G), y(*ctx[K], 2, G * T);
        auto transparent = [&](const uint64_t* c0, size_t items, Ciphertext& ct) {
            std::vector<uint64_t> host(items * 2 * L * N, 0);
            for (size_t t = 0; t < items; ++t) std::memcpy(&host[(2 * t) * L * N], c0 + t * L * N, L * N * 8);
            ct.copy_from_host(host.data());
        };
        transparent(c0_num, G * T, num);
        transparent(c0_den, G, den);
        div.apply(num, den, y);
        ctx[0]->synchronize();
        if (y.is_ntt()) { std::printf("FAIL the output is flagged NTT\n"); return 1; }
        std::printf("iterations %zu depth %zu den_scales", div.iterations(), div.depth());
        for (size_t n = 0; n <= K; ++n) std::printf(" %a", div.den_scale(n));
        std::printf(" num_scales");
        for (size_t n = 0; n <= K; ++n) std::printf(" %a", div.num_scale(n));
        std::printf(" kappas");
        for (size_t n = 0; n < K; ++n) std::printf(" %lld", (long long)div.kappa(n));
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
    std::printf("division words written\n");
    return 0;
}
