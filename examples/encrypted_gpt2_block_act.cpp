// encrypted_gpt2_block_act.cpp - one GPT-2-small transformer block on encrypted, slot-packed hidden states WITH the FFN's non-linearity,
// the closest this library comes to BASELINE configs[4] as a forward pass:
//     qkv = W_qkv x (768 -> 2304);  a = v (attention over one position);  h1 = x + W_o a;  h2 = h1 + W_down (W_up h1)^2
// over Z_65537 (/root/reference/src/core/execution/models/gpt_model.cpp:722-784 forward_transformer_layer, :786-840 attention, :842-859
// forward_mlp with x^2 standing in for GELU).  N = 8192.  The attention half and W_up run on five 60-bit limbs; then the modulus is switched
// to two limbs, the activation is an EXACT ciphertext x ciphertext multiply (ExactMultiplier: the fused tensor-product kernel, i.e. the
// metric op, inside the forward) + relinearisation, and W_down and the residual run on two limbs.  Every stage is decrypted and compared
// with the plaintext computation; the noise budget is reported after every stage (six levels: qkv, the v mask, W_o, W_up, the square, W_down).
//   usage: encrypted_gpt2_block_act [tokens = 4] [reps = 2] [json | text] [ladder | flat] [log2_n = 13 | 14 | 15] [tokens_per_ciphertext = 1 | 2]
// tokens_per_ciphertext = 2 (round 6): the two slot rows of a ciphertext carry two tokens (PackedLinear's two-token packing): the same kernels, half the
// ciphertexts - every stage is still decrypted and compared for BOTH rows.
// STAND-INS (what this is not): x^2 for GELU, no LayerNorm, attention = v (exact at one position only), ONE of the reference's 12 blocks, no LM head.
// SECURITY: at N = 8192 the 360-bit modulus under key switching is far beyond the 218 bits the Homomorphic Encryption Standard allows at 128-bit security
// (ternary secret, sigma = 3.2): that ring is BASELINE configs[4]'s, a performance shape, not a deployable parameter set.  log2_n = 14 runs the same block
// on six primes = 1 mod 2^15 at N = 16384, where 360 bits are inside the 438-bit budget of 128-bit security (the key switches and the multiply are then
// composed from the batched transforms: slower per token, but a parameter set with a margin).  log2_n = 15: the same block on FheParams::n32768(6) at
// N = 32768 - 360 of the 881 bits that ring allows, the room encrypted_gpt2_stack uses for further blocks.
// `ladder`: the modulus falls WITH the noise budget inside the block: qkv on 5 limbs, the v hand-over and W_o on 4, W_up on 3, the square and W_down on 2.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include <deeppowers/fhe.hpp>

using namespace deeppowers::fhe;

namespace {
const size_t D = 768, H = 3072;
const uint64_t TM = 65537;
uint64_t g_seed = 77;
uint64_t rnd(uint64_t m) { g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull; return (g_seed >> 33) % m; }
void fill8(std::vector<uint64_t>& v) { for (auto& x : v) x = (TM + rnd(255) - 127) % TM; }
void matvec(const std::vector<uint64_t>& W, size_t rows, size_t cols, const uint64_t* x, uint64_t* y) {
    for (size_t r = 0; r < rows; ++r) {
        unsigned __int128 acc = 0;
        for (size_t c = 0; c < cols; ++c) acc += (unsigned __int128)W[r * cols + c] * x[c];
        y[r] = (uint64_t)(acc % TM);
    }
}
}  // namespace

int main(int argc, char** argv) {
    const size_t T = argc > 1 ? (size_t)std::atol(argv[1]) : 4;
    const int reps = argc > 2 ? std::atoi(argv[2]) : 2;
    const bool json = argc > 3 && !std::strcmp(argv[3], "json");
    // "ladder": the modulus falls WITH the budget - qkv on 5 limbs, the v hand-over and W_o on 4, W_up on 3, the square and W_down on 2 (a layer's
    // cost goes with digits x limbs: 30 / 20 / 12 / 6 instead of 30 / 30 / 30 / 6); default: the attention half and W_up all on 5 limbs
    const bool ladder = argc > 4 && !std::strcmp(argv[4], "ladder");
    const int log2n = argc > 5 ? std::atoi(argv[5]) : 13;
    if (log2n < 13 || log2n > 15) { std::fprintf(stderr, "log2_n must be 13, 14 or 15\n"); return 1; }
    const size_t tpc = argc > 6 ? (size_t)std::atol(argv[6]) : 1;
    if ((tpc != 1 && tpc != 2) || T % tpc) { std::fprintf(stderr, "tokens_per_ciphertext must be 1 or 2 and divide the token count\n"); return 1; }
    const size_t C = T / tpc;   // ciphertexts per application
    const int lv_attn = ladder ? 4 : 5, lv_up = ladder ? 3 : 5;
    try {
        FheParams p5 = log2n == 15 ? FheParams::n32768(6) : log2n == 14 ? FheParams::n16384(6) : FheParams::n8192_l6();
        const uint64_t special = p5.moduli.back(), special_psi = p5.psi.back();
        p5.moduli.pop_back(); p5.psi.pop_back();
        FheParams pl[6];
        pl[5] = p5; pl[4] = pl[5].drop_last_limb(); pl[3] = pl[4].drop_last_limb(); pl[2] = pl[3].drop_last_limb();
        const size_t n = p5.n();
        std::unique_ptr<Context> ctx[6];
        std::unique_ptr<Evaluator> ev[6];
        for (int l = 2; l <= 5; ++l) { ctx[l].reset(new Context(pl[l], 0)); ev[l].reset(new Evaluator(*ctx[l])); }
        KeyGenerator kg(*ctx[5]);
        std::unique_ptr<SecretKey> sk[6];
        std::unique_ptr<Decryptor> dec[6];
        std::unique_ptr<BatchEncoder> be[6];
        std::unique_ptr<HybridKeySwitcher> hks[6];
        for (int l = 2; l <= 5; ++l) {
            if (l < 5) sk[l].reset(new SecretKey(*ctx[l], kg.secret_key().coefficients()));            // the same secret, seen at that level
            const SecretKey& s = l == 5 ? kg.secret_key() : *sk[l];
            dec[l].reset(new Decryptor(*ctx[l], s));
            be[l].reset(new BatchEncoder(*ctx[l], TM));
            if (l == 5 || l == lv_attn || l == lv_up || l == 2) hks[l].reset(new HybridKeySwitcher(*ctx[l], s, special, special_psi));
        }
        Encryptor enc(*ctx[5], kg.secret_key());
        ExactMultiplier mul(*ctx[5], *ctx[2], TM);

        std::vector<uint64_t> Wqkv(3 * D * D), Wo(D * D), Wu(H * D), Wd(D * H), x(T * D);
        fill8(Wqkv); fill8(Wo); fill8(Wu); fill8(Wd); fill8(x);
        // plaintext forward of every token
        std::vector<uint64_t> qkv(T * 3 * D), h1(T * D), u(T * H), act(T * H), h2(T * D), tmp(H);
        for (size_t tk = 0; tk < T; ++tk) {
            matvec(Wqkv, 3 * D, D, &x[tk * D], &qkv[tk * 3 * D]);
            matvec(Wo, D, D, &qkv[tk * 3 * D + 2 * D], tmp.data());                      // attention over one position: its output is v
            for (size_t r = 0; r < D; ++r) h1[tk * D + r] = (x[tk * D + r] + tmp[r]) % TM;
            matvec(Wu, H, D, &h1[tk * D], &u[tk * H]);
            for (size_t r = 0; r < H; ++r) act[tk * H + r] = (uint64_t)((unsigned __int128)u[tk * H + r] * u[tk * H + r] % TM);
            matvec(Wd, D, H, &act[tk * H], tmp.data());
            for (size_t r = 0; r < D; ++r) h2[tk * D + r] = (h1[tk * D + r] + tmp[r]) % TM;
        }

        auto t0 = std::chrono::steady_clock::now();
        PackedLinear lqkv(*ctx[5], *be[5], *hks[5], Wqkv.data(), 3 * D, D, tpc);
        PackedLinear lo(*ctx[lv_attn], *be[lv_attn], *hks[lv_attn], Wo.data(), D, D, tpc);
        PackedLinear lup(*ctx[lv_up], *be[lv_up], *hks[lv_up], Wu.data(), H, D, tpc);
        PackedLinear ldown(*ctx[2], *be[2], *hks[2], Wd.data(), D, H, tpc);
        PackedSelect take_v(*ctx[lv_attn], *be[lv_attn], *hks[lv_attn], 2 * D, D, lo.input_period(), tpc);
        const uint32_t row_swap = (uint32_t)(2 * n - 1);
        if (tpc == 1) hks[lv_up]->add_galois_element(row_swap);
        // W_up leaves its 3072 outputs in slots 0 .. 3071 of row 0; W_down reads its input replicated with period 4096 over BOTH slot rows.  The row swap
        // fills row 1; a row longer than that period (N = 16384: 8192 slots) also needs the copies inside the row: one more rotation per doubling
        std::vector<uint32_t> spread;
        for (size_t sft = ldown.input_period(); sft < n / 2; sft <<= 1) { spread.push_back(be[lv_up]->galois_element(-(int)sft)); hks[lv_up]->add_galois_element(spread.back()); }
        const double setup_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

        std::vector<uint64_t> slots(n);
        std::vector<int64_t> coeffs(C * n);
        for (size_t c = 0; c < C; ++c) {   // ciphertext c carries token c (one per ciphertext) or tokens 2 c | 2 c + 1 in its two slot rows
            if (tpc == 1) lqkv.pack_input(&x[c * D], slots.data());
            else lqkv.pack_input_rows(&x[(2 * c) * D], &x[(2 * c + 1) * D], slots.data());
            be[5]->encode(slots.data(), &coeffs[c * n]);
        }
        // one set of buffers per level; down(from, to, in) walks `in` down the ladder through them and returns the ciphertext at level `to`
        std::unique_ptr<Ciphertext> lad_a[6], lad_b[6], lad_c[6];
        for (int l = 2; l <= 5; ++l) { lad_a[l].reset(new Ciphertext(*ctx[l], 2, C)); lad_b[l].reset(new Ciphertext(*ctx[l], 2, C)); lad_c[l].reset(new Ciphertext(*ctx[l], 2, C)); }
        auto down = [&](const Ciphertext& in, int from, int to, std::unique_ptr<Ciphertext> (&buf)[6]) -> const Ciphertext& {
            const Ciphertext* cur = &in;
            for (int l = from; l > to; --l) { ev[l]->rescale(*cur, *buf[l - 1]); cur = buf[l - 1].get(); }
            return *cur;
        };
        Ciphertext cx(*ctx[5], 2, C), cqkv(*ctx[5], 2, C);
        Ciphertext ca(*ctx[lv_attn], 2, C), co(*ctx[lv_attn], 2, C), ch1(*ctx[lv_attn], 2, C);
        Ciphertext cu(*ctx[lv_up], 2, C), cus(*ctx[lv_up], 2, C), cur(*ctx[lv_up], 2, C);
        Ciphertext sq3(*ctx[2], 3, C), sq(*ctx[2], 2, C), cdn(*ctx[2], 2, C), ch2(*ctx[2], 2, C);
        enc.encrypt_exact(coeffs.data(), TM, cx);
        const std::vector<uint32_t> swaps(C, row_swap);
        const Ciphertext* u2 = nullptr;
        const Ciphertext* w_in = nullptr;   // W_up's outputs in W_down's input packing (at W_up's level)
        auto block = [&] {
            lqkv.apply(cx, cqkv);                                          // q | k | v at slots 0 .. 3d-1 of row 0, five limbs               (gpt_model.cpp:793)
            const Ciphertext& qkv_l = down(cqkv, 5, lv_attn, lad_a);       // (ladder: to four limbs)
            const Ciphertext& x_l = down(cx, 5, lv_attn, lad_b);
            take_v.apply(qkv_l, ca);                                       // attention over one position: v, re-packed as a layer input        (one mask level)
            lo.apply(ca, co);
            ev[lv_attn]->add(x_l, co, ch1);                                // h1 = x + W_o a
            const Ciphertext& h1_l = down(ch1, lv_attn, lv_up, lad_c);     // (ladder: to three limbs)
            lup.apply(h1_l, cu);                                           // W_up h1                                                            (gpt_model.cpp:848)
            Ciphertext *packed = &cur, *spare = &cu;
            if (tpc == 1) {
                hks[lv_up]->apply_galois_many(cu, swaps, cus);
                ev[lv_up]->add(cu, cus, cur);                              // W_down's input packing: both rows
            } else {
                packed = &cu; spare = &cur;                                // two tokens per ciphertext: every row already holds ITS token's W_up outputs
            }
            for (uint32_t e : spread) {                                    // (N >= 16384 only: the period-4096 copies inside a slot row)
                hks[lv_up]->apply_galois_many(*packed, std::vector<uint32_t>(C, e), cus);
                ev[lv_up]->add(*packed, cus, *spare);
                std::swap(packed, spare);
            }
            w_in = packed;
            u2 = &down(*packed, lv_up, 2, lad_a);                          // modulus switch to two limbs
            mul.multiply(*u2, *u2, sq3);                                   // the activation (exact multiply around the fused ct x ct kernel)
            hks[2]->relinearize(sq3, sq);
            ldown.apply(sq, cdn);                                          // W_down on two limbs
            const Ciphertext& h1_2 = down(ch1, lv_attn, 2, lad_b);         // the residual's operand at that level
            ev[2]->add(h1_2, cdn, ch2);                                    // h2 = h1 + W_down (W_up h1)^2
        };
        block();
        ctx[5]->synchronize();
        t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < reps; ++i) block();
        ctx[5]->synchronize();
        const double ms_per_token = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3 / reps / (double)T;

        std::vector<uint64_t> dm(C * n), got(n), expect(n), yv(D), yw(D);
        size_t bad_h1 = 0, bad_act = 0, bad = 0;
        dec[lv_attn]->decrypt_exact(ch1, TM, dm.data());
        for (size_t c = 0; c < C; ++c) {
            be[lv_attn]->decode(dm.data() + c * n, got.data());
            if (tpc == 1) lup.pack_input(&h1[c * D], expect.data());
            else lup.pack_input_rows(&h1[(2 * c) * D], &h1[(2 * c + 1) * D], expect.data());
            for (size_t i = 0; i < n; ++i) bad_h1 += got[i] != expect[i];
        }
        dec[2]->decrypt_exact(sq, TM, dm.data());
        for (size_t c = 0; c < C; ++c) {
            be[2]->decode(dm.data() + c * n, got.data());
            if (tpc == 1) ldown.pack_input(&act[c * H], expect.data());
            else ldown.pack_input_rows(&act[(2 * c) * H], &act[(2 * c + 1) * H], expect.data());
            for (size_t i = 0; i < n; ++i) bad_act += got[i] != expect[i];
        }
        dec[2]->decrypt_exact(ch2, TM, dm.data());
        for (size_t c = 0; c < C; ++c) {
            be[2]->decode(dm.data() + c * n, got.data());
            if (tpc == 1) {
                ldown.unpack_output(got.data(), yv.data());
                for (size_t r = 0; r < D; ++r) bad += yv[r] != h2[c * D + r];
            } else {
                ldown.unpack_output_rows(got.data(), yv.data(), yw.data());
                for (size_t r = 0; r < D; ++r) bad += (yv[r] != h2[(2 * c) * D + r]) + (yw[r] != h2[(2 * c + 1) * D + r]);
            }
        }
        const double b[8] = {dec[5]->noise_budget_bits(cx, TM), dec[5]->noise_budget_bits(cqkv, TM), dec[lv_attn]->noise_budget_bits(ca, TM), dec[lv_attn]->noise_budget_bits(ch1, TM),
                             dec[lv_up]->noise_budget_bits(*w_in, TM), dec[2]->noise_budget_bits(*u2, TM), dec[2]->noise_budget_bits(sq, TM), dec[2]->noise_budget_bits(ch2, TM)};
        const size_t ks = lqkv.key_switches_per_apply() + take_v.key_switches_per_apply() + lo.key_switches_per_apply() + lup.key_switches_per_apply() + 1 +
                          ldown.key_switches_per_apply() + (tpc == 1 ? 1 : 0);
        const bool ok = !(bad || bad_act || bad_h1);
        char levels[96];
        std::snprintf(levels, sizeof levels, "qkv 5, v + W_o %d, W_up %d, square + W_down 2 limbs", lv_attn, lv_up);
        if (json)
            std::printf("{\"block\": \"transformer_block_square_activation\", \"hidden\": %zu, \"inner\": %zu, \"log2_n\": %d, \"modulus_bits_under_key_switching\": 360, \"he_standard_128bit_budget_bits\": %d, \"levels\": \"%s\", "
                        "\"plain_modulus\": %llu, \"tokens\": %zu, \"tokens_per_ciphertext\": %zu, \"key_switches_per_token\": %zu, \"ct_ct_multiplies_per_token\": 1, \"setup_s\": %.2f, \"ms_per_token\": %.3f, "
                        "\"budget_bits\": [%.0f, %.0f, %.0f, %.0f, %.0f, %.0f, %.0f, %.0f], \"correct\": %s}\n",
                        D, H, log2n, log2n == 15 ? 881 : log2n == 14 ? 438 : 218, levels, (unsigned long long)TM, T, tpc, ks, setup_s, ms_per_token, b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], ok ? "true" : "false");
        else
            std::printf("transformer block with a square activation (%s), %zu token(s) per application, %zu key switches + one ct x ct multiply per token; setup %.2f s, %.3f ms per token\n"
                        "  noise budget (bits): fresh %.0f -> qkv %.0f -> v hand-over %.0f -> h1 %.0f -> W_up hand-over %.0f -> 2 limbs %.0f -> squared %.0f -> h2 %.0f\n"
                        "  h1 %s, activation %s, h2 %s\n", levels, T, ks, setup_s, ms_per_token, b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7],
                        bad_h1 ? "MISMATCH" : "ok", bad_act ? "MISMATCH" : "ok", bad ? "MISMATCH" : "decrypts to h1 + W_down (W_up h1)^2 mod t");
        std::printf(ok ? "OK\n" : "FAILED\n");
        return ok ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
}
