// encrypted_gpt2_ffn_approx.cpp - GPT-2-small's feed-forward block under encryption with REAL weights and a REAL-valued activation, in the approximate
// (CKKS-style) family:
//     y = W_down p(W_up x + b_up) + b_down,   W_up: 768 -> 3072, W_down: 3072 -> 768,   p(u) = a0 + u / 2 + a2 u^2 + a4 u^4
// p is a degree-4 fit of GELU: GELU(u) = u / 2 + u (Phi(u) - 1/2), whose second term is even; a0, a2, a4 are its least-squares fit on [-B, B], B = 4,
// computed below (the odd part of GELU beyond u / 2 is zero, so nothing odd is lost).  W_up is scaled so that every pre-activation of the drawn tokens
// stays inside [-B, B] - asserted in plaintext - because outside the interval the fit means nothing.
// Levels at FheParams::n32768: 6 data limbs + the special prime (420 of the ring's 881 bits): W_up (6 -> 5 limbs), two rotate-and-add steps that repeat
// its 3072 outputs with W_down's input period 4096, ApproxPolynomial (5 -> 2: two product levels and the sum), W_down (2 -> 1).
//   usage: encrypted_gpt2_ffn_approx [tokens = 1] [reps = 2] [json | text]
// Prints the time per token; the measured error against the float64 W_down p(W_up x + b_up) + b_down beside the composed worst-case bound (the layers' and
// the polynomial's error_bound, each fed the bound of the stage before it); and - a DIFFERENT thing - the plaintext fit error max |p(u) - GELU(u)| on
// [-B, B], which no amount of precision removes.
// STAND-INS: a polynomial for GELU, no LayerNorm, no residual; one FFN block, no attention.  Weights and inputs are drawn, not a trained model's.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include <deeppowers/fhe.hpp>

using namespace deeppowers::fhe;
typedef std::complex<double> cplx;

static uint64_t g_state = 1;
static double uni() {   // SplitMix64 -> uniform on [-1, 1)
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * std::ldexp(1.0, -52) - 1.0;
}

static double gelu(double u) { return 0.5 * u * (1.0 + std::erf(u / std::sqrt(2.0))); }

// least squares of a0 + a2 u^2 + a4 u^4 to the even part of GELU, u (Phi(u) - 1/2) = u erf(u / sqrt 2) / 2, on a grid over [0, B] (normal equations, 3 x 3)
static void fit_even_part(double B, double& a0, double& a2, double& a4) {
    double A[3][4] = {{0}};
    const int grid = 4000;
    for (int i = 0; i <= grid; ++i) {
        const double u = B * i / grid, g = 0.5 * u * std::erf(u / std::sqrt(2.0)), phi[3] = {1.0, u * u, u * u * u * u};
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) A[r][c] += phi[r] * phi[c];
            A[r][3] += phi[r] * g;
        }
    }
    for (int c = 0; c < 3; ++c) {   // Gauss-Jordan with the largest pivot of the column
        int piv = c;
        for (int r = c + 1; r < 3; ++r) if (std::fabs(A[r][c]) > std::fabs(A[piv][c])) piv = r;
        std::swap_ranges(A[c], A[c] + 4, A[piv]);
        for (int r = 0; r < 3; ++r) {
            if (r == c) continue;
            const double f = A[r][c] / A[c][c];
            for (int k = c; k < 4; ++k) A[r][k] -= f * A[c][k];
        }
    }
    a0 = A[0][3] / A[0][0]; a2 = A[1][3] / A[1][1]; a4 = A[2][3] / A[2][2];
}

int main(int argc, char** argv) {
    const size_t T = argc > 1 ? (size_t)std::atol(argv[1]) : 1;
    const int reps = argc > 2 ? std::atoi(argv[2]) : 2;
    const bool json = argc > 3 && !std::strcmp(argv[3], "json");
    if (T == 0 || T > 64 || reps < 1) { std::fprintf(stderr, "tokens in [1, 64], reps >= 1\n"); return 1; }
    const size_t d = 768, h = 3072, period = 4096;
    const unsigned log2n = 15;
    const double B = 4.0;
    try {
        // ---- the plaintext side: the fit, the weights, the reference --------------------------------------------------------------------------
        double a0, a2, a4;
        fit_even_part(B, a0, a2, a4);
        const std::vector<double> coeffs{a0, 0.5, a2, 0.0, a4};
        auto p_of = [&](double u) { return a0 + u * (0.5 + u * (a2 + u * u * a4)); };
        double fit_err = 0;
        for (int i = -4000; i <= 4000; ++i) fit_err = std::max(fit_err, std::fabs(p_of(B * i / 4000.0) - gelu(B * i / 4000.0)));
        g_state = 2024;
        std::vector<double> Wu(h * d), bu(h), Wd(d * h), bd(d), x(T * d), u(T * h), act(T * h), want(T * d);
        for (auto& v : Wu) v = uni();
        for (auto& v : bu) v = 0.25 * uni();
        for (auto& v : Wd) v = uni() / 64.0;
        for (auto& v : bd) v = uni();
        for (auto& v : x) v = uni();
        auto pre_activations = [&] {
            double m = 0;
            for (size_t t = 0; t < T; ++t)
                for (size_t r = 0; r < h; ++r) {
                    double acc = bu[r];
                    for (size_t c = 0; c < d; ++c) acc += Wu[r * d + c] * x[t * d + c];
                    u[t * h + r] = acc;
                    m = std::max(m, std::fabs(acc));
                }
            return m;
        };
        const double shrink = 0.9 * B / pre_activations();      // W_up and b_up scaled so that the drawn tokens' pre-activations reach 0.9 B
        for (auto& v : Wu) v *= shrink;
        for (auto& v : bu) v *= shrink;
        const double umax = pre_activations();
        double pmax = 0, ymax = 0;
        for (size_t t = 0; t < T; ++t) {
            for (size_t r = 0; r < h; ++r) { act[t * h + r] = p_of(u[t * h + r]); pmax = std::max(pmax, std::fabs(act[t * h + r])); }
            for (size_t r = 0; r < d; ++r) {
                double acc = bd[r];
                for (size_t c = 0; c < h; ++c) acc += Wd[r * h + c] * act[t * h + c];
                want[t * d + r] = acc;
                ymax = std::max(ymax, std::fabs(acc));
            }
        }

        // ---- the encrypted side ------------------------------------------------------------------------------------------------------------------
        auto t0 = std::chrono::steady_clock::now();
        FheParams p0 = FheParams::n32768(7);
        const uint64_t special = p0.moduli.back(), special_psi = p0.psi.back();
        p0.moduli.pop_back(); p0.psi.pop_back();
        std::vector<FheParams> params(1, p0);
        for (size_t r = 0; r < 5; ++r) params.push_back(params.back().drop_last_limb());
        std::vector<std::unique_ptr<Context>> ctx;
        for (const FheParams& q : params) ctx.emplace_back(new Context(q, 0));
        const size_t n = p0.n(), row = n / 2;
        KeyGenerator kg(*ctx[0]);   // OS CSPRNG
        std::vector<std::unique_ptr<SecretKey>> sk;
        for (auto& c : ctx) sk.emplace_back(new SecretKey(*c, kg.secret_key().coefficients()));
        auto switcher = [&](size_t depth) { return std::unique_ptr<HybridKeySwitcher>(new HybridKeySwitcher(*ctx[depth], *sk[depth], special, special_psi)); };
        std::unique_ptr<HybridKeySwitcher> ks0 = switcher(0), ks1 = switcher(1), ks2 = switcher(2), ks4 = switcher(4);
        ComplexEncoder ce(*ctx[0]);
        Encryptor enc(*ctx[0], kg.secret_key());
        Decryptor dec(*ctx[5], *sk[5]);
        Evaluator ev1(*ctx[1]);
        const double Dx = std::ldexp(1.0, 59), Dw_up = std::ldexp(1.0, 60), S = std::ldexp(1.0, 50), Dw_down = std::ldexp(1.0, 58);
        ApproxPackedLinear up(*ctx[0], *ctx[1], ce, *ks0, Wu.data(), h, d, Dw_up, Dx, 1, bu.data());
        const double Du = up.output_scale();
        ApproxPolynomial poly({ks1.get(), ks2.get()}, *ctx[3], *ctx[4], coeffs, Du, S);
        ApproxPackedLinear down(*ctx[4], *ctx[5], ce, *ks4, Wd.data(), d, h, Dw_down, S, 1, bd.data());
        if (up.output_ciphertexts() != 1 || down.output_ciphertexts() != 1 || down.input_period() != period) { std::printf("unexpected layer geometry\nFAILED\n"); return 1; }
        const std::vector<uint32_t> rot1(T, ce.galois_element(-(int)period)), rot2(T, ce.galois_element(-2 * (int)period));
        ks1->add_galois_element(rot1[0]);
        ks1->add_galois_element(rot2[0]);
        const double setup_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

        std::vector<cplx> slots(row);
        std::vector<int64_t> msg(T * n);
        for (size_t t = 0; t < T; ++t) {
            up.pack_input(&x[t * d], slots.data());
            ce.encode(slots.data(), Dx, &msg[t * n]);
        }
        Ciphertext cx(*ctx[0], 2, T), cu(*ctx[1], 2, T), cr(*ctx[1], 2, T), cu2(*ctx[1], 2, T), cu4(*ctx[1], 2, T), ca(*ctx[4], 2, T), cy(*ctx[5], 2, T);
        enc.encrypt(msg.data(), 0, cx);
        auto block = [&] {
            up.apply(cx, cu);                          // W_up x + b_up: row r at slot r < 3072, zero elsewhere
            ks1->apply_galois_many(cu, rot1, cr);      // ... repeated with period 4096: + the copy 4096 slots to the right,
            ev1.add(cu, cr, cu2);
            ks1->apply_galois_many(cu2, rot2, cr);     //     + both copies 8192 slots to the right
            ev1.add(cu2, cr, cu4);
            poly.apply(cu4, ca);                       // p slot-wise (the padding slots hold p(0): W_down's diagonals are zero there)
            down.apply(ca, cy);                        // W_down p(.) + b_down
        };
        block();                                       // warm-up: code objects, scratch, packed keys
        ctx[0]->synchronize();
        t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < reps; ++i) block();
        ctx[0]->synchronize();
        const double ms_per_token = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3 / reps / (double)T;

        std::vector<int64_t> dm(T * n);
        dec.decrypt(cy, 0, dm.data());
        std::vector<double> y(d);
        double worst = 0;
        for (size_t t = 0; t < T; ++t) {
            ce.decode(&dm[t * n], down.output_scale(), slots.data());
            down.unpack_output(slots.data(), y.data());
            for (size_t r = 0; r < d; ++r) worst = std::max(worst, std::fabs(y[r] - want[t * d + r]));
        }

        // ---- the bound, stage by stage (each stage's slot error e becomes the next one's coefficient bound scale * e / N) ---------------------------
        const double N = (double)n, u8 = 8.0 * log2n * std::ldexp(1.0, -53), H = (N + 1) / 2;
        const double e_up = up.error_bound(1.0, 21.5 + u8 * Dx);
        uint64_t qmax = 0;
        for (uint64_t m : params[1].moduli) qmax = std::max(qmax, m);
        const double K1 = 21.0 * (double)params[1].n_limbs() * N * ((double)qmax / (double)special);
        const double e_rep = 4 * e_up + 3 * N * (K1 + H) / Du;    // two rotate-and-add steps: four terms meet in a slot, three of them key switched
        const double e_act = poly.error_bound(B, Du * e_rep / N);
        const double bound = down.error_bound(pmax + e_act, S * e_act / N);
        const bool inside = umax + e_rep <= B, ok = inside && worst <= bound;
        if (json)
            std::printf("{\"block\": \"ffn_gelu_polynomial\", \"family\": \"approx\", \"hidden\": %zu, \"inner\": %zu, \"log2_n\": %u, \"data_limbs\": 6, \"levels\": 5, \"tokens\": %zu, "
                        "\"setup_s\": %.2f, \"ms_per_token\": %.3f, \"max_abs_preactivation\": %.4f, \"interval\": %.1f, \"fit\": [%.10g, 0.5, %.10g, 0, %.10g], "
                        "\"fit_error_vs_gelu\": %.6f, \"max_abs_output\": %.4f, \"max_error_log2\": %.2f, \"error_bound_log2\": %.2f, \"correct\": %s}\n",
                        d, h, log2n, T, setup_s, ms_per_token, umax, B, a0, a2, a4, fit_err, ymax, std::log2(worst), std::log2(bound), ok ? "true" : "false");
        else
            std::printf("FFN block %zu -> %zu -> p(.) -> %zu in the approximate family at N = %zu, 6 data limbs, 5 levels, %zu token(s) per application; setup %.2f s, %.3f ms per token\n"
                        "  p(u) = %.8f + u / 2 + %.8f u^2 + %.8f u^4 on [-%.0f, %.0f]; max|W_up x + b_up| = %.4f: %s\n"
                        "  encrypted result against the float64 W_down p(W_up x + b_up) + b_down: max|y| %.4f, max error 2^%.2f, composed worst-case bound 2^%.2f: %s\n"
                        "  plaintext fit error of p against GELU on the interval (a property of the polynomial, not of the encryption): max |p(u) - GELU(u)| = %.6f\n",
                        d, h, d, n, T, setup_s, ms_per_token, a0, a2, a4, B, B, umax, inside ? "inside the interval" : "OUTSIDE THE INTERVAL", ymax, std::log2(worst),
                        std::log2(bound), worst <= bound ? "within the bound" : "MISMATCH", fit_err);
        std::printf(ok ? "OK\n" : "FAILED\n");
        return ok ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
}
