// GPU test of re-randomised results in the C++ facade (Rerandomizer): a fresh exact ciphertext keeps its message, gets a new c1 and lands on the
// derived noise budget; two OS-seeded calls differ; the output of a biased 768 x 768 PackedLinear at N = 8192 is re-randomised with the bound
// flood_bits_for gives, compacted and still decrypts to (W x + b) mod t exactly; the argument checks.  Built and run by
// tests/test_gpu_rerandomize.py (-m gpu).  Exit code 0 = all checks passed.
#include <cmath>
#include <cstdio>
#include <sstream>
#include <string>
#include <vector>

#include "facade_test.h"

using namespace deeppowers::fhe;
using namespace facade_test;

static Lcg rnd{4321};
static uint64_t small8() { return rnd.small8(); }

static double log2_q(const FheParams& p) {
    double s = 0;
    for (uint64_t q : p.moduli) s += std::log2((double)q);
    return s;
}

// ---- (a), (b), (d): a fresh exact ciphertext at N = 4096, four pinned limbs ------------------------------------------------------------
static void fresh() {
    const FheParams p = FheParams::n4096_l4();
    const size_t n = p.n(), L = p.n_limbs(), B = 2;
    Context ctx(p, 0);
    KeyGenerator kg(ctx, TestSeed{111});
    PublicKey pk(ctx);
    kg.create_public_key(pk);
    Encryptor enc(ctx, kg.secret_key(), TestSeed{112});
    Decryptor dec(ctx, kg.secret_key());
    std::vector<int64_t> m(B * n);
    for (auto& v : m) v = (int64_t)rnd(T_MOD);
    Ciphertext ct(ctx, 2, B);
    enc.encrypt_exact(m.data(), T_MOD, ct);
    const std::vector<uint64_t> before = words(ct);
    const double fresh_budget = dec.noise_budget_bits(ct, T_MOD);

    // (a) flood_bits = 100 under a TestSeed
    Rerandomizer rr(ctx, pk, TestSeed{113});
    rr.rerandomize(ct, T_MOD, 100);
    ctx.synchronize();
    const std::vector<uint64_t> after = words(ct);
    std::vector<uint64_t> got(B * n);
    dec.decrypt_exact(ct, T_MOD, got.data());
    size_t bad = 0, c1_changed = 0, c0_changed = 0;
    for (size_t i = 0; i < B * n; ++i) bad += got[i] != (uint64_t)m[i];
    for (size_t b = 0; b < B; ++b)
        for (size_t i = 0; i < L * n; ++i) {
            c0_changed += before[(b * 2 + 0) * L * n + i] != after[(b * 2 + 0) * L * n + i];
            c1_changed += before[(b * 2 + 1) * L * n + i] != after[(b * 2 + 1) * L * n + i];
        }
    CHECK(bad == 0);
    CHECK(2 * c1_changed > B * L * n);
    CHECK(2 * c0_changed > B * L * n);
    // The budget.  Decryption sees phase = floor(Q/t) m + v, so t phase = Q m + w with w = t v - (Q mod t) m, and the budget is
    // log2(Q/2) - log2 max |w|.  The mask adds u e_pk + e0 + e1 s to v: |u e_pk| <= 21 N and |e1 s| <= 21 N (ternary u, s; |e| <= 21), |e0| <= 2^100,
    // and the fresh error is at most 21, so |v| <= 2^100 + 42 N + 21 and, with (Q mod t) m < t^2,
    //     |w| <= t (2^100 + 42 N + 21 + t) = t 2^100 (1 + 2^-82)   ->  budget >= B0 - 2^-81,  B0 = log2 Q - 1 - log2 t - 100:    margin 0.01.
    // The largest |e0| among B N uniform values is at least 2^99 except with probability 2^-(B N), so max |v| >= 2^99 - 42 N - 21 and
    //     max |w| >= t (2^99 - 42 N - 21 - t) = t 2^99 (1 - 2^-81)      ->  budget <= B0 + 1 + 2^-80:                              margin 0.01.
    // (noise_budget_bits counts whole bits: floor(log2 Q) - floor(log2 max |w|) - 1.  Here floor(log2 Q) = 239 and log2 t = 16.00002, so it reads 123,
    //  inside the window, unless max |v| > 2^100 (1 - 2^-16), which the largest of these 8192 values does with probability 1/8 and does not
    //  under this seed - it would read 122.)
    const double budget = dec.noise_budget_bits(ct, T_MOD), b0 = log2_q(p) - 1 - std::log2((double)T_MOD) - 100;
    std::printf("fresh N = 4096 L = 4, flood_bits 100: budget %.2f -> %.2f bits, window [%.2f, %.2f]; c1 words changed %zu of %zu\n", fresh_budget, budget,
                b0 - 0.01, b0 + 1.01, c1_changed, B * L * n);
    CHECK(budget >= b0 - 0.01 && budget <= b0 + 1.01);

    // (b) OS-seeded: two calls on copies of one ciphertext give different words and the same plaintext
    Rerandomizer os_rr(ctx, pk);
    Ciphertext x(ctx, 2, B), y(ctx, 2, B);
    x.copy_from_host(before.data());
    y.copy_from_host(before.data());
    os_rr.rerandomize(x, T_MOD, 100);
    os_rr.rerandomize(y, T_MOD, 100);
    ctx.synchronize();
    const std::vector<uint64_t> wx = words(x), wy = words(y);
    size_t differ = 0;
    for (size_t i = 0; i < wx.size(); ++i) differ += wx[i] != wy[i];
    CHECK(2 * differ > wx.size());
    std::vector<uint64_t> gx(B * n), gy(B * n);
    dec.decrypt_exact(x, T_MOD, gx.data());
    dec.decrypt_exact(y, T_MOD, gy.data());
    CHECK(gx == got && gy == got);
    // a smaller batch reuses the work buffer; the same object serves it
    Ciphertext one(ctx, 2, 1);
    one.copy_from_host(before.data());
    os_rr.rerandomize(one, T_MOD, 64);
    ctx.synchronize();
    std::vector<uint64_t> g1(n);
    dec.decrypt_exact(one, T_MOD, g1.data());
    CHECK(std::equal(g1.begin(), g1.end(), got.begin()));

    // (d) the rejections
    Ciphertext three(ctx, 3, B), ntt(ctx, 2, B, /*is_ntt=*/true);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { rr.rerandomize(three, T_MOD, 100); }, "3-component input");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { rr.rerandomize(ntt, T_MOD, 100); }, "NTT-domain input");
    CHECK(rr.max_flood_bits(T_MOD) == 239 - 17 - 4);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { rr.rerandomize(x, T_MOD, 239 - 17 - 4 + 1); }, "flood_bits above floor(log2 Q) - ceil(log2 t) - 4");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { rr.rerandomize(x, T_MOD, 0); }, "flood_bits 0");
    Context other(p, 0);
    PublicKey pk_other(other);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { Rerandomizer bad(ctx, pk_other); }, "public key of another context");
    Ciphertext ct_other(other, 2, B);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { rr.rerandomize(ct_other, T_MOD, 100); }, "ciphertext of another context");
    rr.rerandomize(x, T_MOD, 239 - 17 - 4 - 100);   // the second mask still fits: (2^100 + 2^118) t < Q / 2
    ctx.synchronize();
    dec.decrypt_exact(x, T_MOD, gx.data());
    CHECK(gx == got);
    CHECK(Rerandomizer::flood_bits_for(82.3, 13) == 83 + 40 + 13);
    CHECK(Rerandomizer::flood_bits_for(82.0, 12, 64) == 82 + 64 + 12);
}

// ---- (c) a biased 768 x 768 PackedLinear at N = 8192, five data limbs: evaluate -> rerandomize -> compact -> decrypt ------------------------
static void linear768() {
    FheParams p = FheParams::n8192(6);
    const uint64_t special = p.moduli.back(), special_psi = p.psi.back();
    p.moduli.pop_back(); p.psi.pop_back();
    const size_t n = p.n(), d = 768, T = 2;
    Context ctx(p, 0);
    Evaluator ev(ctx);
    KeyGenerator kg(ctx, TestSeed{91});
    PublicKey pk(ctx);
    kg.create_public_key(pk);
    Encryptor enc(ctx, kg.secret_key(), TestSeed{92});
    Decryptor dec(ctx, kg.secret_key());
    BatchEncoder be(ctx, T_MOD);
    HybridKeySwitcher hks(ctx, kg.secret_key(), special, special_psi, TestSeed{93});
    std::vector<uint64_t> W(d * d), bias(d), x(T * d), slots(n);
    for (auto& v : W) v = small8();
    for (auto& v : bias) v = rnd(T_MOD);
    for (auto& v : x) v = small8();
    PackedLinear lin(ctx, be, hks, W.data(), d, d, 1, bias.data());
    const size_t outs = lin.output_ciphertexts();
    std::vector<int64_t> cx(T * n);
    for (size_t tk = 0; tk < T; ++tk) {
        lin.pack_input(&x[tk * d], slots.data());
        be.encode(slots.data(), &cx[tk * n]);
    }
    Ciphertext ct(ctx, 2, T), cy(ctx, 2, outs * T);
    enc.encrypt_exact(cx.data(), T_MOD, ct);
    lin.apply(ct, cy);
    ctx.synchronize();
    // the client reads the budget of this circuit once; the server uses the bound from then on
    const double b = dec.noise_budget_bits(cy, T_MOD), lq = log2_q(p), noise_bits = lq - 1 - std::log2((double)T_MOD) - b;
    const unsigned flood_bits = Rerandomizer::flood_bits_for(noise_bits, 13);
    const std::vector<uint64_t> c_before = words(cy);
    Rerandomizer rr(ctx, pk, TestSeed{94});
    CHECK(flood_bits <= rr.max_flood_bits(T_MOD));
    rr.rerandomize(cy, T_MOD, flood_bits);
    ctx.synchronize();
    const std::vector<uint64_t> c_after = words(cy);
    size_t changed = 0;
    for (size_t i = 0; i < c_after.size(); ++i) changed += c_after[i] != c_before[i];
    CHECK(2 * changed > c_after.size());
    const double b_after = dec.noise_budget_bits(cy, T_MOD);
    const auto w = CompactCiphertext::recommended_bits(p.log2_n, T_MOD);
    CompactCiphertext cc(ctx, cy.batch(), w.first, w.second);
    ev.compact(cy, cc);
    ctx.synchronize();
    std::vector<uint64_t> dm(cy.batch() * n), got(outs * n), y(d);
    dec.decrypt_exact(cc, T_MOD, dm.data());
    size_t bad = 0;
    for (size_t tk = 0; tk < T; ++tk) {
        for (size_t o = 0; o < outs; ++o) be.decode(&dm[(o * T + tk) * n], &got[o * n]);
        lin.unpack_output(got.data(), y.data());
        bad += y != affine(W, bias.data(), d, d, &x[tk * d], T_MOD);
    }
    CHECK(bad == 0);
    CHECK(b_after >= 2);
    // the mask dominates: the budget is what flood_bits leaves, within the two bits of the derivation in fresh()
    CHECK(b_after >= lq - 1 - std::log2((double)T_MOD) - flood_bits - 1.01 && b_after <= lq - 1 - std::log2((double)T_MOD) - flood_bits + 2.01);
    std::printf("biased 768 x 768 PackedLinear, N = 8192, L = 5: budget %.1f bits, noise bound %.1f bits, flood_bits %u, budget after %.1f bits (compact %.1f)\n", b,
                noise_bits, flood_bits, b_after, dec.noise_budget_bits(cc, T_MOD));
}

int main() {
    try {
        fresh();
        linear768();
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    return finish("rerandomize C++ facade OK");
}
