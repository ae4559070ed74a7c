// encrypted_attention_scores_approx.cpp - the first step of an attention head under encryption in the approximate (CKKS-style) family: the causal scores
// s_ij = <q_i, k_j> / sqrt(d_head), j <= i, of T tokens for ALL 12 heads of GPT-2 small at once, in one deeppowers::fhe::ApproxAttentionScores::apply - the
// T (T + 1) / 2 tensor products of the T + T operands in one all-pairs product step (every operand transformed once), one key switch and one rescale per pair,
// then ONE 6-step rotate-and-add ladder over all pairs on the next level.  N = 32768, FheParams::n32768(8): seven fold primes carry the data, the eighth is the
// special prime of hybrid key switching.
//   client   encrypts the T queries and the T keys at 2^59, heads INTERLEAVED: value `dim` of head `head` in slot dim * 16 + head (12 of the 16 residues carry a
//            head, the other four hold zeros), period 64 * 16 = 1024.
//   server   scores = ApproxAttentionScores(ks, ks_next, T, 64, 16, causal, 2^59, 2^59, 1 / 8).apply(q, k): pair (i, j <= i) at item i (i + 1) / 2 + j, one level
//            down; slot dim * 16 + head of it holds head's score for every dim - replicated over the head's own slots, the layout a slot-wise mix with v packed the
//            same way takes.  The factor 1 / sqrt(64) is folded into the scale: the client decodes at output_scale().
//   client   decrypts, decodes and compares EVERY slot of every pair with float64 and with ApproxAttentionScores::error_bound.
//   usage: encrypted_attention_scores_approx [tokens = 8] [reps = 3] [text | json]
// Prints OK when every slot of every pair is within the bound.
// NOT chained yet, and why: examples/encrypted_softmax_approx takes scores that the client has shifted into [-2, 0] - an encrypted row maximum is not there - and
// spends 11 of 13 levels on its own; the level budget of a whole head (scores, softmax, mix) is later work.
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

static uint64_t g_state = 123;
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
    if (T == 0 || T > 32 || reps < 1) { std::fprintf(stderr, "tokens in [1, 32], reps positive\n"); return 1; }
    const size_t heads = 12, dh = 64, stride = 16, period = dh * stride, pairs = T * (T + 1) / 2;
    const double post = 0.125;   // 1 / sqrt(64)
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
        HybridKeySwitcher ks(c0, kg.secret_key(), special, special_psi), ks1(c1, sk1, special, special_psi);   // relinearisation keys; the ladder's six on ks1
        const double Sq = std::ldexp(1.0, 59), Sk = std::ldexp(1.0, 59);
        ApproxAttentionScores att(ks, ks1, T, dh, stride, /*causal=*/true, Sq, Sk, post);
        const double setup_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

        std::vector<double> q(T * heads * dh), k(T * heads * dh);
        for (auto& x : q) x = uni();
        for (auto& x : k) x = uni();
        auto slot_of = [&](const std::vector<double>& v, size_t t, size_t s) {
            const size_t head = s % stride, dim = (s / stride) % dh;
            return head < heads ? v[(t * heads + head) * dh + dim] : 0.0;
        };
        std::vector<cplx> slots(row);
        std::vector<int64_t> coeffs(std::max(T, pairs) * n);
        Ciphertext cq(c0, 2, T), ck(c0, 2, T), scores(c1, 2, pairs);
        for (int side = 0; side < 2; ++side) {
            for (size_t t = 0; t < T; ++t) {
                for (size_t s = 0; s < row; ++s) slots[s] = cplx(slot_of(side ? k : q, t, s), 0.0);
                ce.encode(slots.data(), side ? Sk : Sq, &coeffs[t * n]);
            }
            enc.encrypt(coeffs.data(), 0, side ? ck : cq);
        }

        att.apply(cq, ck, scores);   // warm-up (code objects, scratch, the ladder's keys packed)
        c0.synchronize();
        t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < reps; ++i) att.apply(cq, ck, scores);
        c0.synchronize();
        const double ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3 / reps;

        dec1.decrypt(scores, 0, coeffs.data());
        double err = 0, big = 0;
        for (size_t i = 0; i < T; ++i)
            for (size_t j = 0; j <= i; ++j) {
                double want[16] = {0};
                for (size_t h = 0; h < heads; ++h) {
                    double s = 0;
                    for (size_t d = 0; d < dh; ++d) s += q[(i * heads + h) * dh + d] * k[(j * heads + h) * dh + d];
                    want[h] = post * s;
                    big = std::max(big, std::fabs(want[h]));
                }
                ce.decode(&coeffs[(i * (i + 1) / 2 + j) * n], att.output_scale(), slots.data());
                for (size_t s = 0; s < row; ++s) err = std::max(err, std::max(std::fabs(slots[s].real() - want[s % stride]), std::fabs(slots[s].imag())));
            }
        // a fresh symmetric ciphertext: |e| <= 21, the rounding 1/2, the encoder's own error at its scale
        auto fresh = [&](double scale, double X) { return 21.5 + 8.0 * 15 * std::ldexp(1.0, -53) * scale * X; };
        const double bound = att.error_bound(1.0, 1.0, fresh(Sq, 1.0), fresh(Sk, 1.0));
        const bool ok = err <= bound && bound < big;
        if (json)
            std::printf("{\"example\": \"attention_scores\", \"family\": \"approx\", \"heads\": %zu, \"d_head\": %zu, \"log2_n\": 15, \"data_limbs\": %zu, \"tokens\": %zu, "
                        "\"pairs\": %zu, \"key_switches\": %zu, \"setup_s\": %.2f, \"apply_ms\": %.3f, \"error_log2\": %.2f, \"error_bound_log2\": %.2f, \"score_max\": %.4f, "
                        "\"correct\": %s}\n",
                        heads, dh, p0.n_limbs(), T, pairs, pairs * 7, setup_s, ms, std::log2(err), std::log2(bound), big, ok ? "true" : "false");
        else
            std::printf("causal attention scores of %zu token(s), %zu heads x %zu, N = %zu on %zu data limbs: setup %.2f s; %zu pairs (x %zu slots) under %zu key switches in "
                        "%.3f ms; max error 2^%.2f, error_bound 2^%.2f on scores up to %.4f: %s\n",
                        T, heads, dh, n, p0.n_limbs(), setup_s, pairs, row, pairs * 7, ms, std::log2(err), std::log2(bound), big, ok ? "within the bound" : "MISMATCH");
        std::printf(ok ? "OK\n" : "FAILED\n");
        return ok ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
}
