// encrypted_gpt2_linear_approx.cpp - GPT-2-small's dense layers under encryption with REAL weights: y = W x + b in the approximate (CKKS-style) family
// (deeppowers::fhe::ApproxPackedLinear), the counterpart of encrypted_gpt2_linear's layers over Z_65537.  N = 8192, six pinned 60-bit primes (five carry
// the data, the sixth is the special prime of hybrid key switching); weights, biases and activations uniform in [-1, 1]; the input is encoded at 2^50, the
// diagonals at 2^58, and the layer's rescale leaves the output at 2^108 / q_5 on four limbs.
//   usage: encrypted_gpt2_linear_approx [layer = all | square | qkv | ffn_up | ffn_down | <out>x<in> | add_plain] [reps = 2] [text | json] [tokens = 1] [log2_n = 13 | 14]
//          [tokens_per_ciphertext = 1 | 2]
// Prints, per layer, the time per token, the measured maximum error against the float64 W x + b and the layer's stated worst-case error_bound.
// `add_plain`: the time of one Evaluator::add_plain (dpfhe_add_plain, a broadcast plaintext) beside one Evaluator::add on the same ciphertext bytes.
// SECURITY: as for encrypted_gpt2_linear - at N = 8192 the 360-bit modulus under key switching is a performance shape, log2_n = 14 is inside the budget.
#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <deeppowers/fhe.hpp>

using namespace deeppowers::fhe;
typedef std::complex<double> cplx;

struct Shape { const char* name; size_t out, in; };

static uint64_t g_state = 1;
static double uni() {   // SplitMix64 -> uniform on [-1, 1)
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * std::ldexp(1.0, -52) - 1.0;
}

// one add_plain and one add over `items` 2-component ciphertexts of `ctx`, microseconds per call by events around `reps` back-to-back calls
static int time_add_plain(const Context& ctx, size_t items, int reps, bool json) {
    Evaluator ev(ctx);
    Ciphertext a(ctx, 2, items), b(ctx, 2, items), out(ctx, 2, items);
    Plaintext p(ctx, 1);
    (void)hipMemset(a.data(), 0, a.words() * 8); (void)hipMemset(b.data(), 0, b.words() * 8); (void)hipMemset(p.data(), 0, p.words() * 8);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    float ms_plain[2] = {0, 0}, ms_add = 0;
    for (int in_place = 0; in_place < 2; ++in_place) {
        Ciphertext& o = in_place ? a : out;
        ev.add_plain(a, p, o);
        (void)hipEventRecord(e0, nullptr);
        for (int i = 0; i < reps; ++i) ev.add_plain(a, p, o);
        (void)hipEventRecord(e1, nullptr);
        (void)hipEventSynchronize(e1);
        (void)hipEventElapsedTime(&ms_plain[in_place], e0, e1);
    }
    ev.add(a, b, out);
    (void)hipEventRecord(e0, nullptr);
    for (int i = 0; i < reps; ++i) ev.add(a, b, out);
    (void)hipEventRecord(e1, nullptr);
    (void)hipEventSynchronize(e1);
    (void)hipEventElapsedTime(&ms_add, e0, e1);
    const double mib = (double)a.words() * 8 / (1 << 20);
    std::printf(json ? "{\"entry\": \"add_plain\", \"items\": %zu, \"ciphertext_mib\": %.1f, \"add_plain_us\": %.2f, \"add_plain_in_place_us\": %.2f, \"add_us\": %.2f}\n"
                     : "add_plain on %zu ciphertexts (%.1f MiB): out of place %.2f us, in place %.2f us; add of two such buffers %.2f us\n",
                items, mib, ms_plain[0] * 1e3 / reps, ms_plain[1] * 1e3 / reps, ms_add * 1e3 / reps);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    std::printf("OK\n");
    return 0;
}

int main(int argc, char** argv) {
    const std::string which = argc > 1 ? argv[1] : "all";
    const int reps = argc > 2 ? std::atoi(argv[2]) : 2;
    const bool json = argc > 3 && !std::strcmp(argv[3], "json");
    const size_t T = argc > 4 ? (size_t)std::atol(argv[4]) : 1;
    const int log2n = argc > 5 ? std::atoi(argv[5]) : 13;
    if (log2n != 13 && log2n != 14) { std::fprintf(stderr, "log2_n must be 13 or 14\n"); return 1; }
    const size_t tpc = argc > 6 ? (size_t)std::atol(argv[6]) : 1;
    if ((tpc != 1 && tpc != 2) || T == 0 || T % tpc || reps < 1) { std::fprintf(stderr, "tokens_per_ciphertext must be 1 or 2 and divide the token count\n"); return 1; }
    const size_t C = T / tpc;   // ciphertexts per application
    std::vector<Shape> shapes;
    const Shape known[] = {{"square", 768, 768}, {"qkv", 2304, 768}, {"ffn_up", 3072, 768}, {"ffn_down", 768, 3072}};
    for (const Shape& k : known)
        if (which == k.name || which == "all") shapes.push_back(k);
    if (shapes.empty() && which != "add_plain") {
        size_t o = 0, i = 0;
        if (std::sscanf(which.c_str(), "%zux%zu", &o, &i) == 2 && o && i) shapes.push_back(Shape{"custom", o, i});
        else { std::fprintf(stderr, "unknown layer '%s'\n", which.c_str()); return 1; }
    }
    try {
        FheParams p = log2n == 14 ? FheParams::n16384(6) : FheParams::n8192_l6();
        const uint64_t special = p.moduli.back(), special_psi = p.psi.back();
        p.moduli.pop_back(); p.psi.pop_back();
        const size_t n = p.n(), row = n / 2;
        Context ctx(p, 0), next(p.drop_last_limb(), 0);
        if (which == "add_plain") return time_add_plain(next, 8 * T, std::max(reps, 20), json);
        KeyGenerator kg(ctx);   // OS CSPRNG (TestSeed{..} would make the run reproducible)
        SecretKey sk_next(next, kg.secret_key().coefficients());
        Encryptor enc(ctx, kg.secret_key());
        Decryptor dec(next, sk_next);
        ComplexEncoder ce(ctx);
        HybridKeySwitcher hks(ctx, kg.secret_key(), special, special_psi);
        const double input_scale = std::ldexp(1.0, 50), weight_scale = std::ldexp(1.0, 58);
        int rc = 0;
        for (const Shape& sh : shapes) {
            g_state = 5 + sh.out;
            std::vector<double> W(sh.out * sh.in), b(sh.out), x(T * sh.in), want(T * sh.out);
            for (auto& v : W) v = uni();
            for (auto& v : b) v = uni();
            for (auto& v : x) v = uni();
            for (size_t tk = 0; tk < T; ++tk)
                for (size_t r = 0; r < sh.out; ++r) {
                    double acc = b[r];
                    for (size_t c = 0; c < sh.in; ++c) acc += W[r * sh.in + c] * x[tk * sh.in + c];
                    want[tk * sh.out + r] = acc;
                }
            auto t0 = std::chrono::steady_clock::now();
            ApproxPackedLinear layer(ctx, next, ce, hks, W.data(), sh.out, sh.in, weight_scale, input_scale, tpc, b.data());   // encodes the diagonals, generates the rotation keys
            const double setup_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            const size_t outs = layer.output_ciphertexts();
            std::vector<cplx> slots(row), got(outs * row);
            std::vector<int64_t> coeffs(C * n), dm(outs * C * n);
            std::vector<double> y(sh.out), y1(sh.out);
            for (size_t c = 0; c < C; ++c) {   // ciphertext c: token c, or tokens 2 c | 2 c + 1 in the real and imaginary parts
                if (tpc == 1) layer.pack_input(&x[c * sh.in], slots.data());
                else layer.pack_input_pair(&x[(2 * c) * sh.in], &x[(2 * c + 1) * sh.in], slots.data());
                ce.encode(slots.data(), input_scale, &coeffs[c * n]);
            }
            Ciphertext cx(ctx, 2, C), cy(next, 2, outs * C);
            enc.encrypt(coeffs.data(), 0, cx);
            layer.apply(cx, cy);                                // warm-up (code objects, allocator)
            ctx.synchronize();
            t0 = std::chrono::steady_clock::now();
            for (int i = 0; i < reps; ++i) layer.apply(cx, cy);
            ctx.synchronize();
            const double apply_ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3 / reps / (double)T;
            dec.decrypt(cy, 0, dm.data());
            double worst = 0;
            for (size_t c = 0; c < C; ++c) {
                for (size_t o = 0; o < outs; ++o) ce.decode(dm.data() + (o * C + c) * n, layer.output_scale(), got.data() + o * row);
                if (tpc == 1) layer.unpack_output(got.data(), y.data());
                else layer.unpack_output_pair(got.data(), y.data(), y1.data());
                for (size_t r = 0; r < sh.out; ++r) {
                    worst = std::max(worst, std::fabs(y[r] - want[(tpc * c) * sh.out + r]));
                    if (tpc == 2) worst = std::max(worst, std::fabs(y1[r] - want[(2 * c + 1) * sh.out + r]));
                }
            }
            // a fresh symmetric ciphertext: |e| <= 21, the rounding 1/2, the encoder's E at input_scale
            const double bound = layer.error_bound(1.0, 21.5 + 8.0 * log2n * std::ldexp(1.0, -53) * input_scale * std::sqrt((double)tpc));
            const bool ok = worst <= bound;
            if (json)
                std::printf("{\"layer\": \"%s\", \"family\": \"approx\", \"out_dim\": %zu, \"in_dim\": %zu, \"log2_n\": %d, \"data_limbs\": %zu, \"baby_steps\": %zu, "
                            "\"giant_steps\": %zu, \"output_ciphertexts\": %zu, \"key_switches\": %zu, \"tokens_per_apply\": %zu, \"tokens_per_ciphertext\": %zu, \"setup_s\": %.2f, "
                            "\"encode_s\": %.3f, \"ms_per_token\": %.3f, \"max_error_log2\": %.2f, \"error_bound_log2\": %.2f, \"correct\": %s}\n",
                            sh.name, sh.out, sh.in, log2n, p.n_limbs(), layer.baby_steps(), layer.giant_steps(), outs, layer.key_switches_per_apply(), T, tpc, setup_s,
                            layer.encode_seconds(), apply_ms, std::log2(worst), std::log2(bound), ok ? "true" : "false");
            else
                std::printf("%-8s %5zu <- %4zu: period %zu, %zu baby x %zu giant steps, %zu output ciphertext(s), %zu key switches, %zu token(s) per apply; setup %.2f s, "
                            "apply %.3f ms per token; max error 2^%.2f, error_bound 2^%.2f: %s\n",
                            sh.name, sh.out, sh.in, layer.input_period(), layer.baby_steps(), layer.giant_steps(), outs, layer.key_switches_per_apply(), T, setup_s, apply_ms,
                            std::log2(worst), std::log2(bound), ok ? "within the bound of W x + b" : "MISMATCH");
            if (!ok) rc = 1;
        }
        std::printf(rc ? "FAILED\n" : "OK\n");
        return rc;
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
}
