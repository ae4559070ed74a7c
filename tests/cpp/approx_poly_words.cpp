// The words ApproxPolynomial::apply gives on a TRANSPARENT input - a ciphertext (c0, 0) whose c0 holds the residues of a known integer polynomial - for
// tests/test_gpu_approx_poly_words.py, which compares them word for word with the integer model of tests/approx_poly_model.py (with c1 = 0 every
// relinearisation digit is zero, every division by P is exact and the polynomial is a deterministic integer function of its inputs).
//   approx_poly_words <case file> <output file>
// The case file (little-endian 64-bit words, doubles by their bits), written by the Python test:
//   magic "APPW1", log2 N, L, moduli[L], psi[L], P, psi_P, T, d, input_scale, output_scale, a[d + 1], c0[T][L][N].
// Level r runs on the context of the first L - r limbs with its own key switcher (same secret, same P); L = ceil(log2 d) + 2.
// It prints one line
//   degree D depth E scales <hex double s_1 .. s_d> weights <c_0' c_1 .. c_d>
// and writes the output words [T][2][L - depth][N] to the output file.  Exit code 0 = written.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "deeppowers/fhe.hpp"

using namespace deeppowers::fhe;

int main(int argc, char** argv) {
    if (argc != 3) { std::printf("usage: approx_poly_words <case file> <output file>\n"); return 2; }
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
    if (u() != 0x3157505041ull) { std::printf("FAIL %s: not a case file\n", argv[1]); return 2; }
    FheParams p;
    p.log2_n = (uint32_t)u();
    const size_t L = (size_t)u();
    if (p.log2_n < 8 || p.log2_n > 16 || L < 3 || L > 16) { std::printf("FAIL case header\n"); return 2; }
    for (size_t l = 0; l < L; ++l) p.moduli.push_back(u());
    for (size_t l = 0; l < L; ++l) p.psi.push_back(u());
    const uint64_t special = u(), special_psi = u();
    const size_t T = (size_t)u(), d = (size_t)u();
    const double input_scale = dbl(), output_scale = dbl();
    if (T == 0 || T > 64 || d < 2 || d > 15) { std::printf("FAIL case header\n"); return 2; }
    std::vector<double> a(d + 1);
    for (double& v : a) v = dbl();
    const size_t N = p.n();
    if (at > w.size() || w.size() - at != T * L * N) { std::printf("FAIL case body: c0 needs %zu words\n", T * L * N); return 2; }
    const uint64_t* c0 = w.data() + at;
    size_t rstar = 0;
    while (((size_t)1 << rstar) < d) ++rstar;
    if (L != rstar + 2) { std::printf("FAIL the case needs ceil(log2 d) + 2 limbs\n"); return 2; }

    try {
        std::vector<FheParams> level(1, p);
        for (size_t r = 0; r <= rstar; ++r) level.push_back(level.back().drop_last_limb());
        std::vector<std::unique_ptr<Context>> ctx;
        for (const FheParams& q : level) ctx.emplace_back(new Context(q, 0));
        KeyGenerator kg(*ctx[0], TestSeed{11});
        std::vector<std::unique_ptr<SecretKey>> sk;
        std::vector<std::unique_ptr<HybridKeySwitcher>> hks;
        std::vector<HybridKeySwitcher*> levels;
        for (size_t r = 0; r < rstar; ++r) {
            sk.emplace_back(new SecretKey(*ctx[r], kg.secret_key().coefficients()));
            hks.emplace_back(new HybridKeySwitcher(*ctx[r], *sk[r], special, special_psi, TestSeed{12 + r}));
            levels.push_back(hks.back().get());
        }
        ApproxPolynomial poly(levels, *ctx[rstar], *ctx[rstar + 1], a, input_scale, output_scale);
        Ciphertext x(*ctx[0], 2, T), y(*ctx[rstar + 1], 2, T);
        {
            std::vector<uint64_t> host(T * 2 * L * N, 0);
            for (size_t t = 0; t < T; ++t) std::memcpy(&host[(2 * t) * L * N], c0 + t * L * N, L * N * 8);
            x.copy_from_host(host.data());
        }
        poly.apply(x, y);
        ctx[0]->synchronize();
        if (y.is_ntt()) { std::printf("FAIL the output is flagged NTT\n"); return 1; }
        std::printf("degree %zu depth %zu scales", poly.degree(), poly.depth());
        for (size_t k = 1; k <= d; ++k) std::printf(" %a", poly.power_scale(k));
        std::printf(" weights");
        for (size_t k = 0; k <= d; ++k) std::printf(" %lld", (long long)poly.weight(k));
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
    std::printf("approximate polynomial words written\n");
    return 0;
}
