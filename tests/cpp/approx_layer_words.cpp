// The words ApproxPackedLinear::apply gives on a TRANSPARENT input - a ciphertext (c0, 0) whose c0 holds the residues of a known integer polynomial - for
// tests/test_gpu_approx_layer_words.py, which compares them word for word with the integer model of tests/approx_layer_model.py (DESIGN.md section 4:
// with c1 = 0 every key-switch digit is zero, every division by P is exact and the layer is a deterministic integer function of its inputs).
//   approx_layer_words <case file> <output file>
// The case file (little-endian 64-bit words, doubles by their bits), written by the Python test:
//   magic "APLW1", log2 N, L, moduli[L], psi[L], P, psi_P, T, tokens per ciphertext, layers (1 or 2), input_scale,
//   per layer: out_dim, in_dim, has_bias, weight_scale, W[out_dim * in_dim], bias[out_dim] (only with a bias),
//   c0[T][L][N].
// Layer k runs from the context on the first L - k limbs to the one on the first L - k - 1, each level with its own key switcher (same secret, same P);
// the second layer takes the first layer's output as it is and the first's output_scale() as its input_scale.
// Per layer it prints one line
//   layer K passes A n1 B n2 C dim D input_period E output_scale <hex double> rows <row_of_slot of every (output ciphertext, slot), -1 for none>
// and it writes the last layer's output words [passes * T][2][limbs][N] to the output file.  Exit code 0 = written.
// (A no-device `geometry` mode cannot be had: the geometry lives in the layer object, whose constructor allocates on the device.)
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "deeppowers/fhe.hpp"

using namespace deeppowers::fhe;

struct Reader {
    std::vector<uint64_t> w;
    size_t at = 0;
    bool ok = true;
    uint64_t u() { if (at >= w.size()) { ok = false; return 0; } return w[at++]; }
    double d() { const uint64_t v = u(); double x; std::memcpy(&x, &v, 8); return x; }
    std::vector<double> doubles(size_t count) {
        std::vector<double> out;
        if (count > w.size() - at) { ok = false; return out; }
        out.resize(count);
        std::memcpy(out.data(), w.data() + at, count * 8);
        at += count;
        return out;
    }
};

struct LayerSpec {
    size_t out_dim = 0, in_dim = 0;
    bool has_bias = false;
    double weight_scale = 0;
    std::vector<double> W, b;
};

int main(int argc, char** argv) {
    if (argc != 3) { std::printf("usage: approx_layer_words <case file> <output file>\n"); return 2; }
    Reader r;
    {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) { std::printf("FAIL cannot read %s\n", argv[1]); return 2; }
        std::fseek(f, 0, SEEK_END);
        const long bytes = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        r.w.resize(bytes > 0 ? (size_t)bytes / 8 : 0);
        const size_t got = std::fread(r.w.data(), 8, r.w.size(), f);
        std::fclose(f);
        if (bytes <= 0 || bytes % 8 || got != r.w.size()) { std::printf("FAIL %s: not a whole number of words\n", argv[1]); return 2; }
    }
    if (r.u() != 0x31574c5041ull) { std::printf("FAIL %s: not a case file\n", argv[1]); return 2; }
    FheParams p;
    p.log2_n = (uint32_t)r.u();
    const size_t L = (size_t)r.u();
    if (!r.ok || p.log2_n < 3 || p.log2_n > 16 || L < 2 || L > 16) { std::printf("FAIL case header\n"); return 2; }
    for (size_t l = 0; l < L; ++l) p.moduli.push_back(r.u());
    for (size_t l = 0; l < L; ++l) p.psi.push_back(r.u());
    const uint64_t special = r.u(), special_psi = r.u();
    const size_t T = (size_t)r.u(), tpc = (size_t)r.u(), layers = (size_t)r.u();
    const double input_scale = r.d();
    if (!r.ok || T == 0 || T > 64 || (layers != 1 && layers != 2) || layers >= L) { std::printf("FAIL case header\n"); return 2; }
    std::vector<LayerSpec> spec(layers);
    for (LayerSpec& s : spec) {
        s.out_dim = (size_t)r.u(); s.in_dim = (size_t)r.u(); s.has_bias = r.u() != 0; s.weight_scale = r.d();
        if (!r.ok || s.out_dim == 0 || s.in_dim == 0 || s.out_dim > (1u << 16) || s.in_dim > (1u << 16)) { std::printf("FAIL layer header\n"); return 2; }
        s.W = r.doubles(s.out_dim * s.in_dim);
        if (s.has_bias) s.b = r.doubles(s.out_dim);
    }
    const size_t N = p.n();
    if (!r.ok || r.w.size() - r.at != T * L * N) { std::printf("FAIL case body: %zu words left, c0 needs %zu\n", r.w.size() - r.at, T * L * N); return 2; }
    const uint64_t* c0 = r.w.data() + r.at;

    try {
        const auto t0 = std::chrono::steady_clock::now();
        // level k: the context on the first L - k limbs
        std::vector<FheParams> level(1, p);
        for (size_t k = 0; k < layers; ++k) level.push_back(level.back().drop_last_limb());
        std::vector<std::unique_ptr<Context>> ctx;
        for (const FheParams& q : level) ctx.emplace_back(new Context(q, 0));
        KeyGenerator kg(*ctx[0], TestSeed{11});
        ComplexEncoder cenc(*ctx[0]);
        std::vector<std::unique_ptr<SecretKey>> sk;
        std::vector<std::unique_ptr<HybridKeySwitcher>> hks;
        for (size_t k = 0; k < layers; ++k) {
            sk.emplace_back(new SecretKey(*ctx[k], kg.secret_key().coefficients()));
            hks.emplace_back(new HybridKeySwitcher(*ctx[k], *sk[k], special, special_psi, TestSeed{12 + k}));
        }
        // the transparent input: (c0, 0)
        std::unique_ptr<Ciphertext> x(new Ciphertext(*ctx[0], 2, T));
        {
            std::vector<uint64_t> host(T * 2 * L * N, 0);
            for (size_t t = 0; t < T; ++t) std::memcpy(&host[(2 * t) * L * N], c0 + t * L * N, L * N * 8);
            x->copy_from_host(host.data());
        }
        double scale = input_scale;
        for (size_t k = 0; k < layers; ++k) {
            const LayerSpec& s = spec[k];
            ApproxPackedLinear lin(*ctx[k], *ctx[k + 1], cenc, *hks[k], s.W.data(), s.out_dim, s.in_dim, s.weight_scale, scale, tpc, s.has_bias ? s.b.data() : nullptr);
            const size_t passes = lin.output_ciphertexts();
            if (k + 1 < layers && passes != 1) { std::printf("FAIL a chained layer must give one output ciphertext\n"); return 1; }
            std::unique_ptr<Ciphertext> y(new Ciphertext(*ctx[k + 1], 2, passes * T));
            lin.apply(*x, *y);
            ctx[k + 1]->synchronize();
            if (y->is_ntt()) { std::printf("FAIL the output is flagged NTT\n"); return 1; }
            std::printf("layer %zu passes %zu n1 %zu n2 %zu dim %zu input_period %zu output_scale %a rows", k, passes, lin.baby_steps(), lin.giant_steps(), lin.dim(),
                        lin.input_period(), lin.output_scale());
            for (size_t o = 0; o < passes; ++o)
                for (size_t sl = 0; sl < N / 2; ++sl) {
                    const size_t R = lin.row_of_slot(o, sl);
                    if (R == (size_t)-1) std::printf(" -1"); else std::printf(" %zu", R);
                }
            std::printf("\n");
            scale = lin.output_scale();
            x = std::move(y);
        }
        std::vector<uint64_t> out(x->words());
        x->copy_to_host(out.data());
        FILE* f = std::fopen(argv[2], "wb");
        if (!f || std::fwrite(out.data(), 8, out.size(), f) != out.size()) { std::printf("FAIL cannot write %s\n", argv[2]); return 1; }
        std::fclose(f);
        std::printf("words %zu seconds %.3f\n", out.size(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    std::printf("approximate layer words written\n");
    return 0;
}
