// GPU test of compact result ciphertexts in the C++ facade (CompactCiphertext, Evaluator::compact, the Decryptor overloads): a fresh exact
// ciphertext, the output of a biased 768 x 768 PackedLinear at N = 8192 and of an activated FFN with biases at N = 16384 all decrypt from compact
// form, after save / load, to exactly the plaintext result.  Built and run by tests/test_gpu_compact.py (-m gpu).  Exit code 0 = all checks passed.
#include <cstdio>
#include <sstream>
#include <string>
#include <vector>

#include "facade_test.h"

using namespace deeppowers::fhe;
using namespace facade_test;

static Lcg rnd{1234};
static uint64_t small8() { return rnd.small8(); }

// compact at the recommended widths, save, load into a fresh object, decrypt: the messages mod t, and the budget
static std::vector<uint64_t> compact_round_trip(const Context& ctx, const Evaluator& ev, Decryptor& dec, const Ciphertext& ct, double& budget) {
    const FheParams& p = ctx.params();
    const auto w = CompactCiphertext::recommended_bits(p.log2_n, T_MOD);
    CompactCiphertext cc(ctx, ct.batch(), w.first, w.second), back(ctx, ct.batch(), w.first, w.second);
    ev.compact(ct, cc);
    ctx.synchronize();
    std::stringstream s;
    cc.save(s);
    const std::string blob = s.str();
    CHECK(blob.size() == 32 + ct.batch() * p.n() * (w.first + w.second) / 8);
    CHECK(blob.size() == 32 + cc.bytes());
    std::stringstream full;
    ct.save(full);
    if (p.n_limbs() >= 2) CHECK(4 * blob.size() < full.str().size());
    std::istringstream in(blob);
    back.load(in);
    std::vector<uint64_t> m(ct.batch() * p.n());
    dec.decrypt_exact(back, T_MOD, m.data());
    budget = dec.noise_budget_bits(back, T_MOD);
    return m;
}

// ---- a fresh exact ciphertext: round trip, widths, argument checks ------------------------------------------------------------------
static void fresh() {
    const FheParams p = FheParams::n8192(5);
    const size_t n = p.n(), B = 3;
    Context ctx(p, 0);
    Evaluator ev(ctx);
    KeyGenerator kg(ctx, TestSeed{81});
    Encryptor enc(ctx, kg.secret_key(), TestSeed{82});
    Decryptor dec(ctx, kg.secret_key());
    std::vector<int64_t> m(B * n);
    for (auto& v : m) v = (int64_t)rnd(T_MOD);
    Ciphertext ct(ctx, 2, B);
    enc.encrypt_exact(m.data(), T_MOD, ct);
    double budget = 0;
    const std::vector<uint64_t> got = compact_round_trip(ctx, ev, dec, ct, budget);
    size_t bad = 0;
    for (size_t i = 0; i < B * n; ++i) bad += got[i] != (uint64_t)m[i];
    CHECK(bad == 0);
    CHECK(budget >= 1);
    std::printf("fresh N = 8192 L = 5: widths (%u, %u), compact budget %.1f bits, full budget %.1f bits\n", CompactCiphertext::recommended_bits(13, T_MOD).first,
                CompactCiphertext::recommended_bits(13, T_MOD).second, budget, dec.noise_budget_bits(ct, T_MOD));
    // widths of the issue: (19, 27) at 2^11, (19, 28) at 2^12 and 2^13, (19, 29) at 2^14
    CHECK(CompactCiphertext::recommended_bits(11, T_MOD) == std::make_pair(19u, 27u));
    CHECK(CompactCiphertext::recommended_bits(12, T_MOD) == std::make_pair(19u, 28u));
    CHECK(CompactCiphertext::recommended_bits(13, T_MOD) == std::make_pair(19u, 28u));
    CHECK(CompactCiphertext::recommended_bits(14, T_MOD) == std::make_pair(19u, 29u));
    // a c1 of 17 bits: the rounding error times the secret swamps the tolerance
    CompactCiphertext narrow(ctx, B, 19, 17);
    ev.compact(ct, narrow);
    ctx.synchronize();
    std::vector<uint64_t> wrong(B * n);
    dec.decrypt_exact(narrow, T_MOD, wrong.data());
    size_t off = 0;
    for (size_t i = 0; i < B * n; ++i) off += wrong[i] != (uint64_t)m[i];
    std::printf("widths (19, 17): %zu of %zu coefficients decrypt wrong\n", off, B * n);
    CHECK(off > B * n / 2);
    // arguments
    CompactCiphertext cc(ctx, B, 19, 28);
    Ciphertext ntt(ctx, 2, B, /*is_ntt=*/true), three(ctx, 3, B), one(ctx, 2, 1);
    expect_error(ErrorCode::INVALID_STATE, [&] { ev.compact(ntt, cc); }, "NTT-domain input");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ev.compact(three, cc); }, "3-component input");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ev.compact(one, cc); }, "batch mismatch");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { CompactCiphertext bad(ctx, B, 7, 28); }, "width 7");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { CompactCiphertext bad(ctx, B, 19, 61); }, "width 61");
    std::stringstream s;
    cc.save(s);
    CompactCiphertext other_bits(ctx, B, 19, 29), other_batch(ctx, B + 1, 19, 28);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { std::istringstream in(s.str()); other_bits.load(in); }, "load: other widths");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { std::istringstream in(s.str()); other_batch.load(in); }, "load: other batch");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { std::istringstream in(s.str().substr(0, s.str().size() - 1)); cc.load(in); }, "load: truncated");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { std::stringstream f; ct.save(f); cc.load(f); }, "load: a DPFHEv1 stream");
}

// ---- a biased 768 x 768 PackedLinear at N = 8192, five data limbs ---------------------------------------------------------------------
static void linear768() {
    FheParams p = FheParams::n8192(6);
    const uint64_t special = p.moduli.back(), special_psi = p.psi.back();
    p.moduli.pop_back(); p.psi.pop_back();
    const size_t n = p.n(), d = 768, T = 2;
    Context ctx(p, 0);
    Evaluator ev(ctx);
    KeyGenerator kg(ctx, TestSeed{91});
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
    double budget = 0;
    const std::vector<uint64_t> dm = compact_round_trip(ctx, ev, dec, cy, budget);
    std::vector<uint64_t> full(dm.size()), got(outs * n), y(d);
    dec.decrypt_exact(cy, T_MOD, full.data());
    CHECK(dm == full);
    size_t bad = 0;
    for (size_t tk = 0; tk < T; ++tk) {
        for (size_t o = 0; o < outs; ++o) be.decode(&dm[(o * T + tk) * n], &got[o * n]);
        lin.unpack_output(got.data(), y.data());
        bad += y != affine(W, bias.data(), d, d, &x[tk * d], T_MOD);
    }
    CHECK(bad == 0);
    CHECK(budget >= 1);
    std::printf("biased 768 x 768 PackedLinear, N = 8192, L = 5: compact budget %.1f bits (full %.1f)\n", budget, dec.noise_budget_bits(cy, T_MOD));
}

// ---- activated FFN with biases at N = 16384: W_down (W_up x + b_up)^2 + b_down, modulus switch 5 -> 2 limbs, compact result ---------------
static void ffn_act16384() {
    FheParams p5 = FheParams::n16384(6);
    const uint64_t special = p5.moduli.back(), special_psi = p5.psi.back();
    p5.moduli.pop_back(); p5.psi.pop_back();
    const FheParams p4 = p5.drop_last_limb(), p3 = p4.drop_last_limb(), p2 = p3.drop_last_limb();
    // h > N / 4: W_down's padded input dimension is a whole slot row (N / 2), the hand-over below fills it
    const size_t n = p5.n(), d = 64, h = 4200, T = 2;
    Context ctx5(p5, 0), ctx4(p4, 0), ctx3(p3, 0), ctx2(p2, 0);
    Evaluator ev5(ctx5), ev4(ctx4), ev3(ctx3), ev2(ctx2);
    KeyGenerator kg(ctx5, TestSeed{101});
    SecretKey sk2(ctx2, kg.secret_key().coefficients());
    Encryptor enc(ctx5, kg.secret_key(), TestSeed{102});
    Decryptor dec2(ctx2, sk2);
    BatchEncoder be5(ctx5, T_MOD), be2(ctx2, T_MOD);
    HybridKeySwitcher hks5(ctx5, kg.secret_key(), special, special_psi, TestSeed{103}), hks2(ctx2, sk2, special, special_psi, TestSeed{104});
    ExactMultiplier mul(ctx5, ctx2, T_MOD);
    std::vector<uint64_t> Wu(h * d), Wd(d * h), bu(h), bd(d), x(T * d);
    for (auto* v : {&Wu, &Wd, &x})
        for (auto& e : *v) e = small8();
    for (auto& e : bu) e = rnd(T_MOD);
    for (auto& e : bd) e = rnd(T_MOD);
    PackedLinear up(ctx5, be5, hks5, Wu.data(), h, d, 1, bu.data()), down(ctx2, be2, hks2, Wd.data(), d, h, 1, bd.data());
    const uint32_t row_swap = (uint32_t)(2 * n - 1);
    hks5.add_galois_element(row_swap);
    std::vector<uint64_t> slots(n);
    std::vector<int64_t> coeffs(T * n);
    for (size_t tk = 0; tk < T; ++tk) {
        up.pack_input(&x[tk * d], slots.data());
        be5.encode(slots.data(), &coeffs[tk * n]);
    }
    Ciphertext cx(ctx5, 2, T), c1(ctx5, 2, T), c1s(ctx5, 2, T), c1r(ctx5, 2, T), u4(ctx4, 2, T), u3(ctx3, 2, T), u2(ctx2, 2, T);
    Ciphertext sq3(ctx2, 3, T), sq(ctx2, 2, T), cy(ctx2, 2, T);
    enc.encrypt_exact(coeffs.data(), T_MOD, cx);
    up.apply(cx, c1);
    hks5.apply_galois_many(c1, std::vector<uint32_t>(T, row_swap), c1s);
    ev5.add(c1, c1s, c1r);
    ev5.rescale(c1r, u4); ev4.rescale(u4, u3); ev3.rescale(u3, u2);
    mul.multiply(u2, u2, sq3);
    hks2.relinearize(sq3, sq);
    down.apply(sq, cy);
    ctx5.synchronize();
    ctx2.synchronize();
    double budget = 0;
    const std::vector<uint64_t> dm = compact_round_trip(ctx2, ev2, dec2, cy, budget);
    std::vector<uint64_t> full(T * n), got(n), y(d);
    dec2.decrypt_exact(cy, T_MOD, full.data());
    CHECK(dm == full);                                         // compact and full words decrypt alike
    size_t bad = 0;
    for (size_t tk = 0; tk < T; ++tk) {
        std::vector<uint64_t> u = affine(Wu, bu.data(), h, d, &x[tk * d], T_MOD);
        for (auto& v : u) v = (uint64_t)((unsigned __int128)v * v % T_MOD);
        be2.decode(&dm[tk * n], got.data());
        down.unpack_output(got.data(), y.data());
        bad += y != affine(Wd, bd.data(), d, h, u.data(), T_MOD);
    }
    CHECK(bad == 0);
    CHECK(budget >= 1);
    std::printf("activated FFN with biases, N = 16384, L = 2: compact budget %.1f bits (full %.1f)\n", budget, dec2.noise_budget_bits(cy, T_MOD));
}

int main() {
    try {
        fresh();
        linear768();
        ffn_act16384();
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    return finish("compact C++ facade OK");
}
