// encrypted_attention_mix_approx.cpp - the mixing step of an attention head under encryption in the approximate (CKKS-style) family: out_i = sum_j p_ij v_j
// for T tokens of a GPT-2-small hidden state (d = 768), ALL T outputs in one deeppowers::fhe::ApproxProductSum::apply - T * T tensor products summed T at a
// time before ONE key switch and ONE rescale per output, with the values v_j shared by all queries (transformed once).  N = 32768, FheParams::n32768(8):
// seven fold primes carry the data, the eighth is the special prime of hybrid key switching.
//   client   encrypts the T values v_j (packed with period 1024, zeros above d) at 2^59 and the T * T weights p_ij, each REPLICATED over every slot of its
//            own ciphertext, at 2^59.  The weights are a softmax of random scores computed IN THE CLEAR by the client: the encrypted softmax (an exponential and
//            a division under encryption) is not there yet - this example is the step that follows it.
//   server   y = ApproxProductSum(ks, T, shared).apply(p, v): item i = sum_j p_ij (.) v_j one level down, at scale 2^118 / q_last.
//   client   decrypts, decodes and compares every slot with float64 and with ApproxProductSum::error_bound.
//   usage: encrypted_attention_mix_approx [tokens = 8] [reps = 3] [text | json]
// Prints OK when every slot of every output is within the bound.
// SECURITY: 7 x 60 + 60 = 480 bits under key switching at N = 32768 is inside the 881-bit budget FheParams::n32768 documents for 128 bits.
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

static uint64_t g_state = 99;
static double uni() {   // SplitMix64 -> uniform on [-1, 1)
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * std::ldexp(1.0, -52) - 1.0;
}

int main(int argc, char** argv) {
    const size_t T = argc > 1 ? (size_t)std::atol(argv[1]) : 8;
    const int reps = argc > 2 ? std::atoi(argv[2]) : 3;
    const bool json = argc > 3 && !std::strcmp(argv[3], "json");
    if (T == 0 || T > 64 || reps < 1) { std::fprintf(stderr, "tokens in [1, 64], reps positive\n"); return 1; }
    const size_t d = 768, period = 1024;
    try {
        FheParams p0 = FheParams::n32768(8);
        const uint64_t special = p0.moduli.back(), special_psi = p0.psi.back();
        p0.moduli.pop_back(); p0.psi.pop_back();
        const FheParams p1 = p0.drop_last_limb();
        const size_t n = p0.n(), row = n / 2;
        Context c0(p0, 0), c1(p1, 0);
        KeyGenerator kg(c0);   // OS CSPRNG (TestSeed{..} would make the run reproducible)
        SecretKey sk1(c1, kg.secret_key().coefficients());
        Encryptor enc(c0, kg.secret_key());
        Decryptor dec1(c1, sk1);
        ComplexEncoder ce(c0);
        auto t0 = std::chrono::steady_clock::now();
        HybridKeySwitcher ks(c0, kg.secret_key(), special, special_psi);   // relinearisation keys only
        const double setup_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const double Sp = std::ldexp(1.0, 59), Sv = std::ldexp(1.0, 59);
        ApproxProductSum mix(ks, T, /*b_shared=*/true, Sp, Sv);

        // the values, the weights (softmax of random scores, in the clear), the float64 outputs
        std::vector<double> v(T * d), p(T * T), want(T * d, 0.0);
        for (auto& x : v) x = uni();
        double pmax = 0;
        for (size_t i = 0; i < T; ++i) {
            double sum = 0;
            for (size_t j = 0; j < T; ++j) sum += (p[i * T + j] = std::exp(2.0 * uni()));
            for (size_t j = 0; j < T; ++j) pmax = std::max(pmax, p[i * T + j] /= sum);
            for (size_t k = 0; k < d; ++k) {
                double s = 0;
                for (size_t j = 0; j < T; ++j) s += p[i * T + j] * v[j * d + k];
                want[i * d + k] = s;
            }
        }
        std::vector<cplx> slots(row);
        std::vector<int64_t> coeffs(T * T * n);
        Ciphertext cv(c0, 2, T), cp(c0, 2, T * T), y(c1, 2, T);
        for (size_t j = 0; j < T; ++j) {
            for (size_t i = 0; i < row; ++i) slots[i] = cplx(i % period < d ? v[j * d + i % period] : 0.0, 0.0);
            ce.encode(slots.data(), Sv, &coeffs[j * n]);
        }
        enc.encrypt(coeffs.data(), 0, cv);
        for (size_t ij = 0; ij < T * T; ++ij) {   // query-major: item i * T + j is p_ij in every slot
            std::fill(slots.begin(), slots.end(), cplx(p[ij], 0.0));
            ce.encode(slots.data(), Sp, &coeffs[ij * n]);
        }
        enc.encrypt(coeffs.data(), 0, cp);

        mix.apply(cp, cv, y);   // warm-up (code objects, scratch)
        c0.synchronize();
        t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < reps; ++i) mix.apply(cp, cv, y);
        c0.synchronize();
        const double ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3 / reps;

        std::vector<int64_t> m(T * n);
        dec1.decrypt(y, 0, m.data());
        double err = 0, big = 0;
        for (size_t i = 0; i < T; ++i) {
            ce.decode(&m[i * n], mix.output_scale(), slots.data());
            for (size_t s = 0; s < row; ++s) {
                const double w = s % period < d ? want[i * d + s % period] : 0.0;
                err = std::max(err, std::max(std::fabs(slots[s].real() - w), std::fabs(slots[s].imag())));
                big = std::max(big, std::fabs(w));
            }
        }
        // a fresh symmetric ciphertext: |e| <= 21, the rounding 1/2, the encoder's own error at its scale
        auto fresh = [&](double scale, double X) { return 21.5 + 8.0 * 15 * std::ldexp(1.0, -53) * scale * X; };
        const double bound = mix.error_bound(pmax, 1.0, fresh(Sp, pmax), fresh(Sv, 1.0));
        const bool ok = err <= bound && bound < big;
        if (json)
            std::printf("{\"example\": \"attention_mix\", \"family\": \"approx\", \"d\": %zu, \"log2_n\": 15, \"data_limbs\": %zu, \"tokens\": %zu, \"products\": %zu, "
                        "\"key_switches\": %zu, \"setup_s\": %.2f, \"apply_ms\": %.3f, \"error_log2\": %.2f, \"error_bound_log2\": %.2f, \"output_max\": %.4f, \"correct\": %s}\n",
                        d, p0.n_limbs(), T, T * T, T, setup_s, ms, std::log2(err), std::log2(bound), big, ok ? "true" : "false");
        else
            std::printf("attention mix of %zu token(s), d = %zu, N = %zu on %zu data limbs: setup %.2f s; %zu products under %zu key switches in %.3f ms; max error 2^%.2f, "
                        "error_bound 2^%.2f on outputs up to %.4f: %s (softmax itself is not encrypted here: the weights were computed in the clear)\n",
                        T, d, n, p0.n_limbs(), setup_s, T * T, T, ms, std::log2(err), std::log2(bound), big, ok ? "within the bound" : "MISMATCH");
        std::printf(ok ? "OK\n" : "FAILED\n");
        return ok ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
}
