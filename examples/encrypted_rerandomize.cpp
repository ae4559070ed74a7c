// encrypted_rerandomize.cpp - a served layer that protects its weights: evaluate -> rerandomize -> compact.
// GPT-2-small's 768 x 768 dense layer with a bias under encryption (PackedLinear at N = 8192, five data limbs + the special prime, t = 65537) for
// `tokens` hidden states; before the results leave the server a fresh public-key encryption of zero with a flooding error is added to each
// (deeppowers::fhe::Rerandomizer), then they are switched to compact form.  The client decrypts (W x + b) mod t exactly and can no longer read the
// layer's noise, which is a function of W.
//   usage: encrypted_rerandomize [tokens = 8] [reps = 20] [lambda = 40]
// Prints the noise budget before and after the step, the flooding width, and the median time of the layer's apply and of the step over `reps` calls each.
// The noise bound is PUBLIC and belongs to the circuit: here the client reads the budget of one run of this layer once (a deployment would take it from
// its noise model, as examples/encrypted_gpt2_stack.cpp does) and the server uses the bound for every later request.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <deeppowers/fhe.hpp>

using namespace deeppowers::fhe;

template <class F>
static double median_ms(const Context& ctx, int reps, F f) {
    std::vector<double> ms;
    for (int i = 0; i < reps; ++i) {
        ctx.synchronize();
        const auto t0 = std::chrono::steady_clock::now();
        f();
        ctx.synchronize();
        ms.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3);
    }
    std::sort(ms.begin(), ms.end());
    return ms[ms.size() / 2];
}

int main(int argc, char** argv) {
    const size_t T = argc > 1 ? (size_t)std::atol(argv[1]) : 8;
    const int reps = argc > 2 ? std::atoi(argv[2]) : 20;
    const unsigned lambda = argc > 3 ? (unsigned)std::atoi(argv[3]) : 40;
    if (T == 0 || reps < 1) { std::fprintf(stderr, "tokens and reps must be positive\n"); return 1; }
    try {
        FheParams p = FheParams::n8192_l6();
        const uint64_t special = p.moduli.back(), special_psi = p.psi.back();
        p.moduli.pop_back(); p.psi.pop_back();
        const size_t n = p.n(), d = 768;
        Context ctx(p, 0);
        Evaluator ev(ctx);
        KeyGenerator kg(ctx);   // OS CSPRNG
        PublicKey pk(ctx);
        kg.create_public_key(pk);
        Encryptor enc(ctx, kg.secret_key());
        Decryptor dec(ctx, kg.secret_key());
        BatchEncoder be(ctx, 65537);
        const uint64_t t = be.plain_modulus();
        HybridKeySwitcher hks(ctx, kg.secret_key(), special, special_psi);
        uint64_t s = 7;
        auto rnd = [&](uint64_t m) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (s >> 33) % m; };
        std::vector<uint64_t> W(d * d), bias(d), x(T * d), slots(n);
        for (auto& v : W) v = (t + rnd(255) - 127) % t;
        for (auto& v : x) v = (t + rnd(255) - 127) % t;
        for (auto& v : bias) v = rnd(t);
        PackedLinear layer(ctx, be, hks, W.data(), d, d, 1, bias.data());
        const size_t outs = layer.output_ciphertexts();
        std::vector<int64_t> coeffs(T * n);
        for (size_t tk = 0; tk < T; ++tk) {
            layer.pack_input(&x[tk * d], slots.data());
            be.encode(slots.data(), &coeffs[tk * n]);
        }
        Ciphertext cx(ctx, 2, T), cy(ctx, 2, outs * T), scratch(ctx, 2, outs * T);
        enc.encrypt_exact(coeffs.data(), t, cx);
        layer.apply(cx, cy);   // warm-up (code objects, allocator)
        const double apply_ms = median_ms(ctx, reps, [&] { layer.apply(cx, cy); });

        double lq = 0;
        for (uint64_t q : p.moduli) lq += std::log2((double)q);
        const double before = dec.noise_budget_bits(cy, t), noise_bits = lq - 1 - std::log2((double)t) - before;
        const unsigned flood_bits = Rerandomizer::flood_bits_for(noise_bits, p.log2_n, lambda);
        Rerandomizer rr(ctx, pk);   // a fresh secret seed from the OS CSPRNG for every call
        if (flood_bits > rr.max_flood_bits(t)) { std::printf("no room: flood_bits %u above %u\n", flood_bits, rr.max_flood_bits(t)); return 1; }
        // timed on a scratch copy (every call adds another mask); the checked result below is re-randomised once
        std::vector<uint64_t> words(cy.words());
        cy.copy_to_host(words.data());
        scratch.copy_from_host(words.data());
        rr.rerandomize(scratch, t, flood_bits);   // warm-up: allocates the work buffer
        const double rr_ms = median_ms(ctx, reps, [&] { rr.rerandomize(scratch, t, flood_bits); });

        rr.rerandomize(cy, t, flood_bits);
        ctx.synchronize();
        const double after = dec.noise_budget_bits(cy, t);
        const auto w = CompactCiphertext::recommended_bits(p.log2_n, t);
        CompactCiphertext cc(ctx, cy.batch(), w.first, w.second);
        ev.compact(cy, cc);
        ctx.synchronize();
        std::vector<uint64_t> dm(cy.batch() * n), got(outs * n), y(d);
        dec.decrypt_exact(cc, t, dm.data());
        size_t bad = 0;
        for (size_t tk = 0; tk < T; ++tk) {
            for (size_t o = 0; o < outs; ++o) be.decode(&dm[(o * T + tk) * n], &got[o * n]);
            layer.unpack_output(got.data(), y.data());
            for (size_t r = 0; r < d; ++r) {
                unsigned __int128 acc = bias[r];
                for (size_t c = 0; c < d; ++c) acc += (unsigned __int128)W[r * d + c] * x[tk * d + c];
                bad += y[r] != (uint64_t)(acc % t);
            }
        }
        std::printf("768 x 768 + bias, N = %zu, %zu data limbs, %zu token(s), %zu result ciphertext(s)\n", n, p.n_limbs(), T, cy.batch());
        std::printf("noise budget: %.0f bits after the layer (public noise bound %.0f bits), flood_bits = %u (lambda = %u), %.0f bits after rerandomize, %.0f bits compact (%u + %u bits per coefficient)\n",
                    before, noise_bits, flood_bits, lambda, after, dec.noise_budget_bits(cc, t), w.first, w.second);
        std::printf("median of %d: apply %.3f ms, rerandomize %.1f us (%.1f %% of the layer)\n", reps, apply_ms, rr_ms * 1e3, 100.0 * rr_ms / apply_ms);
        std::printf("{\"tokens\": %zu, \"result_ciphertexts\": %zu, \"apply_ms\": %.4f, \"rerandomize_us\": %.2f, \"flood_bits\": %u, \"budget_before\": %.1f, \"budget_after\": %.1f, \"correct\": %s}\n",
                    T, cy.batch(), apply_ms, rr_ms * 1e3, flood_bits, before, after, bad ? "false" : "true");
        std::printf(bad ? "FAILED\n" : "OK: decrypts to (W x + b) mod t\n");
        return bad ? 1 : 0;
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
}
