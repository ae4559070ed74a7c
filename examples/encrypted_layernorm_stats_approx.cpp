// encrypted_layernorm_stats_approx.cpp - the statistics of a LayerNorm under encryption in the approximate (CKKS-style) family: the mean and the variance of
// an encrypted GPT-2-small hidden state (d = 768), by sums across slots (deeppowers::fhe::SlotSum).  N = 8192, six pinned 60-bit primes (five carry the data,
// the sixth is the special prime of hybrid key switching); the state, uniform in [-1, 1], is packed the way ApproxPackedLinear::pack_input packs a layer's
// input - period 1024, zeros above d - and encoded at 2^50.
//   mean      SlotSum(1024) on the input's level: every slot holds sum_i x_i = d mean, at the input's scale
//   centred   mask (.) x - (mask / d) (.) sum: two plaintext products at 2^58 (mask: 1 on the d slots of every period, 0 on the padding) and one rescale
//   variance  one HybridKeySwitcher::multiply_rescale (the square) and a second SlotSum(1024) one level down: every slot holds d var
//   usage: encrypted_layernorm_stats_approx [tokens = 8] [reps = 5] [text | json]
// Prints both results against float64.  The mean's error stands beside SlotSum::error_bound and is held to it.  The variance's error is printed WITHOUT a
// gate: a worst-case bound chained over its three stages (sum, product, sum) multiplies a factor N per stage (T1 of include/deeppowers/fhe.hpp) and is
// vacuous - orders of magnitude above the values -, so it would gate nothing.  The division by the standard deviation is not here: it needs a polynomial
// for 1 / sqrt(v) over a caller-chosen range (ApproxPolynomial), which is the step these sums unblock.
// SECURITY: as for encrypted_gpt2_linear_approx - at N = 8192 the 360-bit modulus under key switching is a performance shape, not a 128-bit parameter set.
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
#include <stdexcept>
#include <vector>

#include <deeppowers/fhe.hpp>

using namespace deeppowers::fhe;
typedef std::complex<double> cplx;

static uint64_t g_state = 77;
static double uni() {   // SplitMix64 -> uniform on [-1, 1)
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * std::ldexp(1.0, -52) - 1.0;
}

int main(int argc, char** argv) {
    const size_t T = argc > 1 ? (size_t)std::atol(argv[1]) : 8;
    const int reps = argc > 2 ? std::atoi(argv[2]) : 5;
    const bool json = argc > 3 && !std::strcmp(argv[3], "json");
    if (T == 0 || reps < 1) { std::fprintf(stderr, "tokens and reps must be positive\n"); return 1; }
    const size_t d = 768, period = 1024;
    try {
        FheParams p0 = FheParams::n8192_l6();
        const uint64_t special = p0.moduli.back(), special_psi = p0.psi.back();
        p0.moduli.pop_back(); p0.psi.pop_back();
        const FheParams p1 = p0.drop_last_limb(), p2 = p1.drop_last_limb();
        const size_t n = p0.n(), row = n / 2;
        Context c0(p0, 0), c1(p1, 0), c2(p2, 0);
        KeyGenerator kg(c0);   // OS CSPRNG (TestSeed{..} would make the run reproducible)
        SecretKey sk1(c1, kg.secret_key().coefficients()), sk2(c2, kg.secret_key().coefficients());
        Encryptor enc(c0, kg.secret_key());
        Decryptor dec0(c0, kg.secret_key()), dec2(c2, sk2);
        ComplexEncoder ce(c0);
        Evaluator ev0(c0);
        HybridKeySwitcher ks0(c0, kg.secret_key(), special, special_psi), ks1(c1, sk1, special, special_psi), ks2(c2, sk2, special, special_psi);
        const double D = std::ldexp(1.0, 50), W = std::ldexp(1.0, 58);
        auto t0 = std::chrono::steady_clock::now();
        SlotSum sum0(ks0, period), sum2(ks2, period);   // ten rotation keys each
        const double setup_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

        // the tokens, their float64 statistics, their packed encodings
        std::vector<double> x(T * d), mean(T), var(T);
        for (auto& v : x) v = uni();
        for (size_t t = 0; t < T; ++t) {
            double s = 0, q = 0;
            for (size_t i = 0; i < d; ++i) s += x[t * d + i];
            mean[t] = s / (double)d;
            for (size_t i = 0; i < d; ++i) q += (x[t * d + i] - mean[t]) * (x[t * d + i] - mean[t]);
            var[t] = q / (double)d;
        }
        std::vector<cplx> slots(row);
        std::vector<int64_t> coeffs(T * n);
        for (size_t t = 0; t < T; ++t) {
            for (size_t i = 0; i < row; ++i) slots[i] = cplx(i % period < d ? x[t * d + i % period] : 0.0, 0.0);
            ce.encode(slots.data(), D, &coeffs[t * n]);
        }
        Ciphertext cx(c0, 2, T);
        enc.encrypt(coeffs.data(), 0, cx);
        // the two plaintexts of the centring step, encoded on the device at W and kept in the NTT domain
        std::vector<double> mask(2 * row);
        for (size_t i = 0; i < row; ++i) { mask[i] = i % period < d ? 1.0 : 0.0; mask[row + i] = mask[i] / (double)d; }
        double* d_mask = nullptr;
        if (hipMalloc(&d_mask, mask.size() * sizeof(double)) != hipSuccess || hipMemcpy(d_mask, mask.data(), mask.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
            throw std::runtime_error("hipMalloc / hipMemcpy of the masks");
        Plaintext pa(c0, 1), pb(c0, 1);
        ce.encode_device(d_mask, 1, W, pa, /*to_ntt=*/true, /*real=*/true);
        ce.encode_device(d_mask + row, 1, W, pb, /*to_ntt=*/true, /*real=*/true);
        c0.synchronize();
        (void)hipFree(d_mask);

        Ciphertext csum(c0, 2, T), xn(c0, 2, T), sn(c0, 2, T), ya(c0, 2, T), yb(c0, 2, T), cen(c1, 2, T), sq(c2, 2, T), cvar(c2, 2, T);
        auto mean_stage = [&] { sum0.apply(cx, csum); };
        auto variance_stage = [&] {
            (void)hipMemcpyAsync(xn.data(), cx.data(), cx.words() * 8, hipMemcpyDeviceToDevice, nullptr);   // the transforms are in place
            (void)hipMemcpyAsync(sn.data(), csum.data(), csum.words() * 8, hipMemcpyDeviceToDevice, nullptr);
            xn.set_ntt(false); sn.set_ntt(false);
            ev0.transform_to_ntt_inplace(xn); ev0.transform_to_ntt_inplace(sn);
            ev0.multiply_plain(xn, pa, ya); ev0.multiply_plain(sn, pb, yb);
            ev0.sub(ya, yb, ya);
            ev0.transform_from_ntt_inplace(ya);
            ev0.rescale(ya, cen);
            ks1.multiply_rescale(cen, cen, sq);
            sum2.apply(sq, cvar);
        };
        mean_stage(); variance_stage();   // warm-up (code objects, scratch, key packs)
        c0.synchronize();
        t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < reps; ++i) mean_stage();
        c0.synchronize();
        const double mean_ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3 / reps / (double)T;
        t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < reps; ++i) variance_stage();
        c0.synchronize();
        const double var_ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3 / reps / (double)T;

        // results: every slot of csum holds d mean at D; every slot of cvar holds d var at s2
        const double q4 = (double)p0.moduli.back(), q3 = (double)p1.moduli.back(), s1 = D * W / q4, s2 = s1 * s1 / q3;
        std::vector<int64_t> m0(T * n), m2(T * n);
        dec0.decrypt(csum, 0, m0.data());
        dec2.decrypt(cvar, 0, m2.data());
        double mean_err = 0, var_err = 0, var_max = 0;
        for (size_t t = 0; t < T; ++t) {
            ce.decode(&m0[t * n], D, slots.data());
            for (size_t i = 0; i < row; ++i) mean_err = std::max(mean_err, std::abs(slots[i] / (double)d - mean[t]));
            ce.decode(&m2[t * n], s2, slots.data());
            for (size_t i = 0; i < row; ++i) var_err = std::max(var_err, std::abs(slots[i] / (double)d - var[t]));
            var_max = std::max(var_max, var[t]);
        }
        // a fresh symmetric ciphertext: |e| <= 21, the rounding 1/2, the encoder's E at D; the sum's bound is in units of the sum, the mean's is 1 / d of it
        const double bound = sum0.error_bound(D, 1.0, 21.5 + 8.0 * 13 * std::ldexp(1.0, -53) * D) / (double)d;
        const bool ok = mean_err <= bound;
        if (json)
            std::printf("{\"example\": \"layernorm_stats\", \"family\": \"approx\", \"d\": %zu, \"period\": %zu, \"log2_n\": 13, \"data_limbs\": %zu, \"tokens\": %zu, "
                        "\"key_switches_mean\": %zu, \"key_switches_variance\": %zu, \"setup_s\": %.2f, \"mean_ms_per_token\": %.3f, \"variance_ms_per_token\": %.3f, "
                        "\"mean_error_log2\": %.2f, \"mean_error_bound_log2\": %.2f, \"variance_error_log2\": %.2f, \"variance_max\": %.4f, \"correct\": %s}\n",
                        d, period, p0.n_limbs(), T, sum0.steps(), sum2.steps() + 1, setup_s, mean_ms, var_ms, std::log2(mean_err), std::log2(bound), std::log2(var_err), var_max,
                        ok ? "true" : "false");
        else
            std::printf("LayerNorm statistics of %zu token(s), d = %zu in periods of %zu: setup %.2f s; mean %.3f ms per token (%zu key switches), max error 2^%.2f, "
                        "error_bound 2^%.2f: %s; variance %.3f ms per token more (%zu key switches), max error 2^%.2f on values up to %.4f (no gate: a chained worst-case "
                        "bound is vacuous)\n",
                        T, d, period, setup_s, mean_ms, sum0.steps(), std::log2(mean_err), std::log2(bound), ok ? "within the bound" : "MISMATCH", var_ms, sum2.steps() + 1,
                        std::log2(var_err), var_max);
        std::printf(ok ? "OK\n" : "FAILED\n");
        return ok ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
}
