// encrypted_layernorm_approx.cpp - a whole LayerNorm under encryption in the approximate (CKKS-style) family: gamma (x - mean) / sqrt(var) + beta of an
// encrypted GPT-2-small hidden state (d = 768).  N = 32768, FheParams::n32768(14): thirteen 60-bit primes carry the data, the fourteenth is the special prime
// of hybrid key switching.  Every token has its own spread, drawn so that the variances cover about [0.1, 1]; the state is packed the way
// ApproxPackedLinear::pack_input packs a layer's input - period 1024, zeros above d - and encoded at 2^56.
//   mean       SlotSum(1024) on the input's level: every slot holds sum_i x_i = d mean                                           level 0
//   centred    mask (.) x - (mask / d) (.) sum: two plaintext products at 2^60 and one rescale                                  level 0 -> 1
//   variance   one HybridKeySwitcher::multiply_rescale (the square) and a second SlotSum(1024): every slot holds d var - read as var at d times the scale
//                                                                                                                               level 1 -> 2
//   guess      a cubic ApproxPolynomial: the interpolant of v^-1/2 at the four Chebyshev nodes of the range (about 10 % off at its worst)  level 2 -> 5
//   Newton     two steps of ApproxInvSqrt, y <- 1.5 y - 0.5 (v y)(y y): the cubic's 1e-1 becomes 1.5e-2, then 3e-4                       level 5 -> 9
//   normalise  (x - mean) * y by multiply_rescale                                                                               level 9 -> 10
//   affine     gamma in one plaintext product and a rescale, beta by add_plain                                                  level 10 -> 11
//   usage: encrypted_layernorm_approx [tokens = 4] [reps = 3] [text | json]
// Prints the normalised vector against float64: the exact LayerNorm, and the float64 pipeline with the same cubic and the same two steps (their difference is
// Newton's, not the encryption's).  Two gates.  The Newton stage alone: the decrypted y against the float64 iteration from the DECRYPTED v and guess, within
// ApproxInvSqrt::error_bound.  The whole: the encrypted result's error against the exact LayerNorm may exceed the float64 pipeline's by at most that bound.
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
#include <functional>
#include <memory>
#include <stdexcept>
#include <vector>

#include <deeppowers/fhe.hpp>

using namespace deeppowers::fhe;
typedef std::complex<double> cplx;

static uint64_t g_state = 177;
static double uni() {   // SplitMix64 -> uniform on [-1, 1)
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * std::ldexp(1.0, -52) - 1.0;
}

// the power-basis coefficients of the cubic through (t_i, t_i^-1/2) at the four Chebyshev nodes of [lo, hi]
static std::vector<double> cubic_guess(double lo, double hi) {
    double A[4][5];
    for (int i = 0; i < 4; ++i) {
        const double t = 0.5 * (lo + hi) + 0.5 * (hi - lo) * std::cos(M_PI * (2 * i + 1) / 8.0);
        A[i][0] = 1; A[i][1] = t; A[i][2] = t * t; A[i][3] = t * t * t; A[i][4] = 1.0 / std::sqrt(t);
    }
    for (int c = 0; c < 4; ++c) {   // Gauss-Jordan with partial pivoting
        int p = c;
        for (int r = c + 1; r < 4; ++r) if (std::fabs(A[r][c]) > std::fabs(A[p][c])) p = r;
        for (int k = 0; k < 5; ++k) std::swap(A[c][k], A[p][k]);
        for (int r = 0; r < 4; ++r) {
            if (r == c) continue;
            const double f = A[r][c] / A[c][c];
            for (int k = c; k < 5; ++k) A[r][k] -= f * A[c][k];
        }
    }
    return {A[0][4] / A[0][0], A[1][4] / A[1][1], A[2][4] / A[2][2], A[3][4] / A[3][3]};
}

static double seconds_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

int main(int argc, char** argv) {
    const size_t T = argc > 1 ? (size_t)std::atol(argv[1]) : 4;
    const int reps = argc > 2 ? std::atoi(argv[2]) : 3;
    const bool json = argc > 3 && !std::strcmp(argv[3], "json");
    if (T == 0 || reps < 1) { std::fprintf(stderr, "tokens and reps must be positive\n"); return 1; }
    const size_t d = 768, period = 1024, kLevels = 12, kSteps = 2;
    const double v_lo = 0.1, v_hi = 1.0;
    try {
        FheParams p0 = FheParams::n32768(14);
        const uint64_t special = p0.moduli.back(), special_psi = p0.psi.back();
        p0.moduli.pop_back(); p0.psi.pop_back();
        const size_t n = p0.n(), row = n / 2, L0 = p0.n_limbs();
        std::vector<FheParams> params(1, p0);
        for (size_t r = 1; r < kLevels; ++r) params.push_back(params.back().drop_last_limb());
        std::vector<std::unique_ptr<Context>> c;
        for (const FheParams& p : params) c.emplace_back(new Context(p, 0));
        auto q_of = [&](size_t level) { return (double)params[level].moduli.back(); };   // the prime level `level` drops
        auto t0 = std::chrono::steady_clock::now();
        KeyGenerator kg(*c[0]);   // OS CSPRNG (TestSeed{..} would make the run reproducible)
        std::vector<std::unique_ptr<SecretKey>> sk;
        for (size_t r = 0; r < kLevels; ++r) sk.emplace_back(new SecretKey(*c[r], kg.secret_key().coefficients()));
        std::vector<std::unique_ptr<HybridKeySwitcher>> ks;   // levels 0 .. 9: every level at which a product or a rotation happens
        for (size_t r = 0; r <= 9; ++r) ks.emplace_back(new HybridKeySwitcher(*c[r], *sk[r], special, special_psi));
        Encryptor enc(*c[0], kg.secret_key());
        ComplexEncoder ce(*c[0]);
        Evaluator ev0(*c[0]), ev10(*c[10]), ev11(*c[11]);
        SlotSum sum0(*ks[0], period), sum2(*ks[2], period);   // ten rotation keys each

        // scales: input D, masks W; centred s1; square s2; the variance is the slot total d var at s2, read as var at v_scale = d s2
        const double D = std::ldexp(1.0, 56), W = std::ldexp(1.0, 60), s1 = D * W / q_of(0), s2 = s1 * s1 / q_of(1), v_scale = (double)d * s2;
        const double guess_scale = ApproxInvSqrt::balanced_guess_scale(v_scale, (uint64_t)q_of(5), (uint64_t)q_of(6));
        const std::vector<double> cubic = cubic_guess(v_lo, v_hi);
        ApproxPolynomial guess({ks[2].get(), ks[3].get()}, *c[4], *c[5], cubic, v_scale, guess_scale);
        ApproxInvSqrt newton({ks[5].get(), ks[6].get(), ks[7].get(), ks[8].get()}, *c[9], v_scale, guess_scale);
        const double sy = newton.scale(kSteps), sn = s1 * sy / q_of(9), Wg = std::ldexp(1.0, 56), sf = sn * Wg / q_of(10);
        const double setup_s = seconds_since(t0);

        // the tokens (spread sigma_t: var = sigma_t^2 over [v_lo, v_hi] up to the sample's own deviation), gamma and beta, the float64 references
        std::vector<double> x(T * d), mean(T), var(T), gamma(d), beta(d);
        for (size_t i = 0; i < d; ++i) { gamma[i] = 1.0 + 0.5 * uni(); beta[i] = 0.5 * uni(); }
        for (size_t t = 0; t < T; ++t) {
            const double target = T > 1 ? v_lo * 1.15 + (v_hi * 0.87 - v_lo * 1.15) * (double)t / (double)(T - 1) : 0.5, sigma = std::sqrt(3.0 * target);
            double s = 0, qq = 0;
            for (size_t i = 0; i < d; ++i) { x[t * d + i] = sigma * uni(); s += x[t * d + i]; }
            mean[t] = s / (double)d;
            for (size_t i = 0; i < d; ++i) qq += (x[t * d + i] - mean[t]) * (x[t * d + i] - mean[t]);
            var[t] = qq / (double)d;
            if (var[t] < v_lo || var[t] > v_hi) throw std::runtime_error("a token's variance left the range of the guess");
        }
        std::vector<double> exact(T * d), pipe(T * d), y_pipe(T);
        for (size_t t = 0; t < T; ++t) {
            double y = ((cubic[3] * var[t] + cubic[2]) * var[t] + cubic[1]) * var[t] + cubic[0];
            for (size_t k = 0; k < kSteps; ++k) y = 1.5 * y - 0.5 * ((var[t] * y) * (y * y));
            y_pipe[t] = y;
            for (size_t i = 0; i < d; ++i) {
                exact[t * d + i] = gamma[i] * (x[t * d + i] - mean[t]) / std::sqrt(var[t]) + beta[i];
                pipe[t * d + i] = gamma[i] * ((x[t * d + i] - mean[t]) * y) + beta[i];
            }
        }
        std::vector<cplx> slots(row);
        std::vector<int64_t> coeffs(T * n);
        for (size_t t = 0; t < T; ++t) {
            for (size_t i = 0; i < row; ++i) slots[i] = cplx(i % period < d ? x[t * d + i % period] : 0.0, 0.0);
            ce.encode(slots.data(), D, &coeffs[t * n]);
        }
        Ciphertext cx(*c[0], 2, T);
        enc.encrypt(coeffs.data(), 0, cx);
        // plaintexts, encoded on the device: the two masks of the centring step (NTT domain, level 0), gamma (NTT domain, level 10), beta (level 11)
        std::vector<double> host(4 * row);
        for (size_t i = 0; i < row; ++i) {
            const bool in = i % period < d;
            host[i] = in ? 1.0 : 0.0; host[row + i] = host[i] / (double)d;
            host[2 * row + i] = in ? gamma[i % period] : 0.0; host[3 * row + i] = in ? beta[i % period] : 0.0;
        }
        double* d_host = nullptr;
        if (hipMalloc(&d_host, host.size() * sizeof(double)) != hipSuccess || hipMemcpy(d_host, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
            throw std::runtime_error("hipMalloc / hipMemcpy of the plaintext slots");
        Plaintext pa(*c[0], 1), pb(*c[0], 1), pg(*c[10], 1), pbeta(*c[11], 1);
        ce.encode_device(d_host, 1, W, pa, /*to_ntt=*/true, /*real=*/true);
        ce.encode_device(d_host + row, 1, W, pb, true, true);
        ce.encode_device(d_host + 2 * row, 1, Wg, pg, true, true);
        ce.encode_device(d_host + 3 * row, 1, sf, pbeta, false, true);
        c[0]->synchronize();
        (void)hipFree(d_host);

        Ciphertext csum(*c[0], 2, T), xn(*c[0], 2, T), sm(*c[0], 2, T), ya(*c[0], 2, T), yb(*c[0], 2, T), cen(*c[1], 2, T), sq(*c[2], 2, T), cvar(*c[2], 2, T),
            y0(*c[5], 2, T), v5(*c[5], 2, T), y(*c[9], 2, T), cen9(*c[9], 2, T), norm(*c[10], 2, T), scaled(*c[10], 2, T), out(*c[11], 2, T);
        // a ciphertext at a lower level: the first limbs of every polynomial (the ciphertext and its scale do not change)
        auto drop = [&](const Ciphertext& src, size_t from, Ciphertext& dst, size_t to) {
            const size_t src_row = (L0 - from) * n * 8, dst_row = (L0 - to) * n * 8;
            if (hipMemcpy2DAsync(dst.data(), dst_row, src.data(), src_row, dst_row, 2 * T, hipMemcpyDeviceToDevice, nullptr) != hipSuccess) throw std::runtime_error("hipMemcpy2DAsync");
            dst.set_ntt(false);
        };
        std::vector<std::pair<const char*, std::function<void()>>> stages;
        stages.emplace_back("mean", [&] { sum0.apply(cx, csum); });
        stages.emplace_back("centre", [&] {
            (void)hipMemcpyAsync(xn.data(), cx.data(), cx.words() * 8, hipMemcpyDeviceToDevice, nullptr);   // the transforms are in place
            (void)hipMemcpyAsync(sm.data(), csum.data(), csum.words() * 8, hipMemcpyDeviceToDevice, nullptr);
            xn.set_ntt(false); sm.set_ntt(false);
            ev0.transform_to_ntt_inplace(xn); ev0.transform_to_ntt_inplace(sm);
            ev0.multiply_plain(xn, pa, ya); ev0.multiply_plain(sm, pb, yb);
            ev0.sub(ya, yb, ya);
            ev0.transform_from_ntt_inplace(ya);
            ev0.rescale(ya, cen);
        });
        stages.emplace_back("variance", [&] { ks[1]->multiply_rescale(cen, cen, sq); sum2.apply(sq, cvar); });
        stages.emplace_back("guess", [&] { guess.apply(cvar, y0); });
        stages.emplace_back("newton", [&] { drop(cvar, 2, v5, 5); newton.apply(v5, y0, y); });
        stages.emplace_back("normalise", [&] { drop(cen, 1, cen9, 9); ks[9]->multiply_rescale(cen9, y, norm); });
        stages.emplace_back("affine", [&] {
            ev10.transform_to_ntt_inplace(norm);
            ev10.multiply_plain(norm, pg, scaled);
            ev10.transform_from_ntt_inplace(scaled);
            ev10.rescale(scaled, out);
            ev11.add_plain(out, pbeta, out);
        });
        for (auto& s : stages) s.second();   // warm-up (code objects, scratch, key packs)
        c[0]->synchronize();
        std::vector<double> stage_ms(stages.size(), 0.0);
        for (int i = 0; i < reps; ++i)
            for (size_t s = 0; s < stages.size(); ++s) {
                t0 = std::chrono::steady_clock::now();
                stages[s].second();
                c[0]->synchronize();
                stage_ms[s] += seconds_since(t0) * 1e3 / reps / (double)T;
            }
        double total_ms = 0;
        for (double m : stage_ms) total_ms += m;

        // results
        auto decode = [&](const Ciphertext& ct, size_t level, double scale) {
            Decryptor dec(*c[level], *sk[level]);
            std::vector<int64_t> m(T * n);
            dec.decrypt(ct, 0, m.data());
            std::vector<cplx> z(T * row);
            for (size_t t = 0; t < T; ++t) ce.decode(&m[t * n], scale, &z[t * row]);
            return z;
        };
        const std::vector<cplx> zv = decode(v5, 5, v_scale), zy0 = decode(y0, 5, guess_scale), zy = decode(y, 9, sy), zo = decode(out, 11, sf);
        // gate 1, the Newton stage alone: the float64 iteration from the values its inputs decrypt to
        double V = 0, Y = 0, newton_err = 0, guess_off = 0, y_off = 0;
        for (size_t t = 0; t < T; ++t)
            for (size_t i = 0; i < row; ++i) {
                const double v = zv[t * row + i].real();
                double yn = zy0[t * row + i].real();
                V = std::max(V, std::fabs(v)); Y = std::max(Y, std::fabs(yn));
                guess_off = std::max(guess_off, std::fabs(yn * std::sqrt(var[t]) - 1));
                for (size_t k = 0; k < kSteps; ++k) { yn = 1.5 * yn - 0.5 * ((v * yn) * (yn * yn)); Y = std::max(Y, std::fabs(yn)); }
                newton_err = std::max(newton_err, std::max(std::fabs(zy[t * row + i].real() - yn), std::fabs(zy[t * row + i].imag())));
                y_off = std::max(y_off, std::fabs(zy[t * row + i].real() * std::sqrt(var[t]) - 1));
            }
        // the inputs' phases ARE the decoded values times the scale, up to the decode's own rounding E = u8 scale max|value| per coefficient
        const double u8 = 8.0 * 15 * std::ldexp(1.0, -53);
        const double bound = newton.error_bound(V, Y * (1 + std::ldexp(1.0, -40)), u8 * v_scale * V, u8 * guess_scale * Y);
        // gate 2, the whole: errors against the exact LayerNorm
        double err_enc = 0, err_pipe = 0, out_max = 0;
        for (size_t t = 0; t < T; ++t)
            for (size_t i = 0; i < row; ++i) {
                if (i % period >= d) continue;
                const size_t k = t * d + i % period;
                err_enc = std::max(err_enc, std::abs(zo[t * row + i] - exact[k]));
                err_pipe = std::max(err_pipe, std::fabs(pipe[k] - exact[k]));
                out_max = std::max(out_max, std::fabs(exact[k]));
            }
        const bool ok = newton_err <= bound && err_enc <= err_pipe + bound;
        const size_t levels_used = 11, limbs_left = L0 - levels_used;
        if (json) {
            std::printf("{\"example\": \"layernorm\", \"family\": \"approx\", \"d\": %zu, \"period\": %zu, \"log2_n\": 15, \"data_limbs\": %zu, \"tokens\": %zu, \"levels\": %zu, "
                        "\"limbs_left\": %zu, \"setup_s\": %.2f, \"ms_per_token\": %.3f, \"stage_ms_per_token\": {", d, period, L0, T, levels_used, limbs_left, setup_s, total_ms);
            for (size_t s = 0; s < stages.size(); ++s) std::printf("%s\"%s\": %.3f", s ? ", " : "", stages[s].first, stage_ms[s]);
            std::printf("}, \"guess_relative_error\": %.3e, \"newton_relative_error\": %.3e, \"newton_stage_error_log2\": %.2f, \"newton_error_bound_log2\": %.2f, "
                        "\"max_error\": %.3e, \"float64_pipeline_error\": %.3e, \"relative_error\": %.3e, \"output_max\": %.3f, \"correct\": %s}\n",
                        guess_off, y_off, std::log2(newton_err), std::log2(bound), err_enc, err_pipe, err_enc / out_max, out_max, ok ? "true" : "false");
        } else {
            std::printf("LayerNorm of %zu token(s), d = %zu in periods of %zu, N = %zu, %zu data limbs: %zu levels consumed, %zu limbs left; setup %.2f s; %.3f ms per token\n", T, d,
                        period, n, L0, levels_used, limbs_left, setup_s, total_ms);
            std::printf("  ms per token per stage:");
            for (size_t s = 0; s < stages.size(); ++s) std::printf(" %s %.3f", stages[s].first, stage_ms[s]);
            std::printf("\n  1/sqrt(var): the cubic guess is within %.2e (relative), after %zu Newton steps %.2e; the Newton stage against the float64 iteration from its decrypted "
                        "inputs: max error 2^%.2f, error_bound 2^%.2f: %s\n", guess_off, kSteps, y_off, std::log2(newton_err), std::log2(bound),
                        newton_err <= bound ? "within the bound" : "MISMATCH");
            std::printf("  gamma (x - mean) / sqrt(var) + beta against float64: max error %.3e on values up to %.3f (relative %.3e); the float64 pipeline with the same guess "
                        "and steps: %.3e: %s\n", err_enc, out_max, err_enc / out_max, err_pipe, err_enc <= err_pipe + bound ? "no further than the bound beyond it" : "MISMATCH");
        }
        std::printf(ok ? "OK\n" : "FAILED\n");
        return ok ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
}
