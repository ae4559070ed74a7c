// encrypted_softmax_approx.cpp - the softmax of an attention head under encryption in the approximate (CKKS-style) family: p_ij = exp(s_ij) / sum_k exp(s_ik)
// for T tokens' scores, one ciphertext per (query, key) with the score REPLICATED over its slots - the layout encrypted_attention_mix_approx takes its weights
// in, so this example is the step before that one.  N = 32768, FheParams::n32768(14): thirteen primes carry the data, the fourteenth is the special prime of
// hybrid key switching; eleven levels are used and two limbs are left for the result (a quotient near 1 at a scale near the primes needs them).
//   client   encrypts the T * T scores, shifted by the client into [-B, 0] (B = 2: subtract the row's maximum, clip), at 2^59.
//   server   1. exp(x / 4) as a degree-7 ApproxPolynomial (Taylor; 4 levels), at an output scale chosen so that after the squarings the denominator's scale
//               sits at the primes;
//            2. two squarings (HybridKeySwitcher::multiply_rescale_range with both operands the same range; 2 levels): e_ij = exp(s_ij);
//            3. the row sums d_i = sum_j e_ij (dpfhe_reduce_sum per query: additions, no level);
//            4. ApproxDivide, K = 5 Goldschmidt steps (5 levels) on the constant guess c = guess(T e^-B, T) folded into the scales: numerators and
//               denominators are both read at scale / c, so the quotient is p_ij itself.
//   client   decrypts, decodes and compares every slot of every weight with float64's softmax.
//   usage: encrypted_softmax_approx [tokens = 8] [reps = 3] [text | json]
// Prints OK when every slot is within error_bound + |p| residual(lo, hi, K): ApproxDivide::error_bound on input noise bounds that carry everything upstream
// (the polynomial's error_bound, its truncation, the squarings' amplification and roundings), plus what K steps leave of the constant guess.
// A context that holds any of primes 9 to 14 of FheParams::n32768 runs the context-wide generic arithmetic on every limb: levels 0 to 5 here.
// SECURITY: 13 x 60 + 60 = 840 bits under key switching at N = 32768 is inside the 881-bit budget FheParams::n32768 documents for 128 bits.
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
#include <memory>
#include <stdexcept>
#include <vector>

#include <deeppowers/fhe.hpp>
#include <dpfhe.h>

using namespace deeppowers::fhe;
typedef std::complex<double> cplx;

static uint64_t g_state = 77;
static double unit() {   // SplitMix64 -> uniform on [0, 1)
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * std::ldexp(1.0, -53);
}

int main(int argc, char** argv) {
    const size_t T = argc > 1 ? (size_t)std::atol(argv[1]) : 8;
    const int reps = argc > 2 ? std::atoi(argv[2]) : 3;
    const bool json = argc > 3 && !std::strcmp(argv[3], "json");
    if (T < 2 || T > 16 || reps < 1) { std::fprintf(stderr, "tokens in [2, 16], reps positive\n"); return 1; }
    const double B = 2.0;
    const size_t degree = 7, r = 2, K = 5, poly_levels = 4, data_limbs = 13, depth = poly_levels + r + K;   // 11 levels, two limbs left
    try {
        FheParams p0 = FheParams::n32768(data_limbs + 1);
        const uint64_t special = p0.moduli.back(), special_psi = p0.psi.back();
        p0.moduli.pop_back(); p0.psi.pop_back();
        const size_t n = p0.n(), row = n / 2;
        const double N = (double)n, H = (N + 1) / 2, u = std::ldexp(1.0, -53);
        std::vector<FheParams> params(1, p0);
        for (size_t l = 0; l < depth; ++l) params.push_back(params.back().drop_last_limb());
        std::vector<std::unique_ptr<Context>> ctx;
        for (const FheParams& p : params) ctx.emplace_back(new Context(p, 0));
        auto q = [&](size_t level) { return (double)params[level].moduli.back(); };   // the prime level `level` drops
        KeyGenerator kg(*ctx[0]);   // OS CSPRNG (TestSeed{..} would make the run reproducible)
        Encryptor enc(*ctx[0], kg.secret_key());
        SecretKey sk_out(*ctx[depth], kg.secret_key().coefficients());
        Decryptor dec(*ctx[depth], sk_out);
        ComplexEncoder ce(*ctx[0]);
        auto t0 = std::chrono::steady_clock::now();
        std::vector<std::unique_ptr<SecretKey>> sk;
        std::vector<std::unique_ptr<HybridKeySwitcher>> ks(depth);   // relinearisation keys only; level 3 (the polynomial's sum) has no key switch
        for (size_t l = 0; l < depth; ++l) {
            sk.emplace_back(new SecretKey(*ctx[l], kg.secret_key().coefficients()));
            if (l != poly_levels - 1) ks[l].reset(new HybridKeySwitcher(*ctx[l], *sk[l], special, special_psi));
        }
        const double setup_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

        // scales: the division wants its denominator, read at den_scale = s_e / c, at the prime its first level drops; s_e = ((S^2 / q_4)^2) / q_5
        const double lo = (double)T * std::exp(-B), hi = (double)T, c = ApproxDivide::guess(lo, hi);
        const double Sx = std::ldexp(1.0, 59), S = std::sqrt(std::sqrt(c * q(6) * q(5)) * q(4));
        const double s_sq = (S * S) / q(4), s_e = (s_sq * s_sq) / q(5), div_scale = s_e / c;
        std::vector<double> coeffs(degree + 1);   // exp(x / 2^r) = sum_k x^k / (k! 2^(r k))
        double a = 1, tau = 1;                    // tau: the truncation |t|^(d+1) / (d+1)! at t = B / 2^r (alternating series, t <= 0)
        for (size_t k = 0; k <= degree; ++k) { coeffs[k] = a; a /= (double)(k + 1) * std::ldexp(1.0, (int)r); }
        for (size_t k = 1; k <= degree + 1; ++k) tau *= (B / std::ldexp(1.0, (int)r)) / (double)k;
        ApproxPolynomial poly({ks[0].get(), ks[1].get(), ks[2].get()}, *ctx[3], *ctx[4], coeffs, Sx, S);
        std::vector<HybridKeySwitcher*> div_levels;
        for (size_t l = poly_levels + r; l < depth; ++l) div_levels.push_back(ks[l].get());
        ApproxDivide div(div_levels, *ctx[depth], div_scale, div_scale);

        // the scores in [-B, 0], float64's softmax
        std::vector<double> s(T * T), want(T * T);
        double pmax = 0;
        for (size_t i = 0; i < T; ++i) {
            double sum = 0;
            for (size_t j = 0; j < T; ++j) sum += std::exp(s[i * T + j] = -B * unit());
            for (size_t j = 0; j < T; ++j) pmax = std::max(pmax, want[i * T + j] = std::exp(s[i * T + j]) / sum);
        }
        std::vector<cplx> slots(row);
        std::vector<int64_t> msg(T * T * n);
        Ciphertext x(*ctx[0], 2, T * T), e4(*ctx[4], 2, T * T), e5(*ctx[5], 2, T * T), e6(*ctx[6], 2, T * T), d6(*ctx[6], 2, T), y(*ctx[depth], 2, T * T);
        for (size_t ij = 0; ij < T * T; ++ij) {   // query-major: item i * T + j is s_ij in every slot
            std::fill(slots.begin(), slots.end(), cplx(s[ij], 0.0));
            ce.encode(slots.data(), Sx, &msg[ij * n]);
        }
        enc.encrypt(msg.data(), 0, x);

        dpfhe_ctx* h6 = static_cast<dpfhe_ctx*>(ctx[6]->handle());
        const size_t ct6 = 2 * params[6].n_limbs() * n;
        auto softmax = [&]() {
            poly.apply(x, e4);                                                  // exp(x / 4)
            ks[4]->multiply_rescale_range(e4, 0, e4, 0, T * T, e5, 0);         // exp(x / 2)
            ks[5]->multiply_rescale_range(e5, 0, e5, 0, T * T, e6, 0);         // exp(x)
            for (size_t i = 0; i < T; ++i)                                      // d_i = sum_j e_ij
                if (dpfhe_reduce_sum(h6, d6.data() + i * ct6, e6.data() + i * T * ct6, T, 2, nullptr)) throw std::runtime_error("dpfhe_reduce_sum failed");
            div.apply(e6, d6, y);                                               // e_ij / d_i
        };
        softmax();   // warm-up (code objects, scratch)
        ctx[0]->synchronize();
        t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < reps; ++i) softmax();
        ctx[0]->synchronize();
        const double ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3 / reps;

        std::vector<int64_t> m(T * T * n);
        dec.decrypt(y, 0, m.data());
        // the bound.  Upstream of the division, in units of the value: the polynomial (its own bound on a fresh input, and the truncation), then per squaring
        // v -> v^2 with |v| <= 1: twice the error, its square, the relinearisation and the rescale's rounding in a slot, the scale's own rounding
        auto fresh = [&](double scale, double X) { return 21.5 + 8.0 * 15 * u * scale * X; };
        auto keyswitch = [&](size_t level) {
            const std::vector<uint64_t>& mods = params[level].moduli;
            return 21.0 * (double)mods.size() * N * ((double)*std::max_element(mods.begin(), mods.end()) / (double)special);
        };
        double eps = poly.error_bound(B, fresh(Sx, B)) + tau;
        eps = 2 * eps + eps * eps + (N * (keyswitch(4) + H) / q(4) + N * H) / s_sq + 4 * u;
        eps = 2 * eps + eps * eps + (N * (keyswitch(5) + H) / q(5) + N * H) / s_e + 4 * u;
        // the division reads c e_ij and c d_i at scale s_e / c: slot errors s_e eps and T s_e eps in the phases, handed over as coefficient errors (a slot is at
        // most N times a coefficient: the bound multiplies them back)
        const double rho = (hi - lo) / (hi + lo), hair = 1 + std::ldexp(1.0, -40);
        const double bound = div.error_bound((1 + rho) * hair, (1 + rho) * hair, (double)T * s_e * eps / N, s_e * eps / N);
        const double residual = ApproxDivide::residual(lo, hi, K);
        double err = 0, over = 0;
        for (size_t ij = 0; ij < T * T; ++ij) {
            ce.decode(&m[ij * n], div.num_scale(K), slots.data());
            for (size_t k = 0; k < row; ++k) {
                const double off = std::max(std::fabs(slots[k].real() - want[ij]), std::fabs(slots[k].imag()));
                err = std::max(err, off);
                over = std::max(over, off - (bound + want[ij] * residual));
            }
        }
        const bool ok = over <= 0 && bound + pmax * residual < pmax;
        if (json)
            std::printf("{\"example\": \"softmax\", \"family\": \"approx\", \"log2_n\": 15, \"data_limbs\": %zu, \"levels\": %zu, \"tokens\": %zu, \"weights\": %zu, \"score_range\": %.1f, "
                        "\"degree\": %zu, \"squarings\": %zu, \"goldschmidt_steps\": %zu, \"setup_s\": %.2f, \"softmax_ms\": %.3f, \"error_log2\": %.2f, \"error_bound_log2\": %.2f, "
                        "\"residual_log2\": %.2f, \"weight_max\": %.4f, \"correct\": %s}\n",
                        data_limbs, depth, T, T * T, B, degree, r, K, setup_s, ms, std::log2(err), std::log2(bound), std::log2(residual), pmax, ok ? "true" : "false");
        else
            std::printf("softmax of %zu x %zu scores in [-%.0f, 0], N = %zu on %zu data limbs, %zu levels (degree %zu, %zu squarings, %zu Goldschmidt steps): setup %.2f s; %.3f ms; "
                        "accuracy reached: max error 2^%.2f on weights up to %.4f; error_bound 2^%.2f, residual 2^%.2f: %s\n",
                        T, T, B, n, data_limbs, depth, degree, r, K, setup_s, ms, std::log2(err), pmax, std::log2(bound), std::log2(residual), ok ? "within the bound" : "MISMATCH");
        std::printf(ok ? "OK\n" : "FAILED\n");
        return ok ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
}
