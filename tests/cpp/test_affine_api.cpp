// GPU test of exact plaintext addition in the C++ facade (ExactPlaintext, Evaluator::add_plain_exact / sub_plain_exact) and of the biased
// packed layers built on it (PackedLinear with a bias, PackedTransformerBlock with four biases, an activated FFN with biases).  Every case
// decrypts to exactly the plaintext computation mod t.  Built and run by tests/test_gpu_plain_add.py (-m gpu).  Exit code 0 = all checks passed.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "facade_test.h"

using namespace deeppowers::fhe;
using namespace facade_test;

static Lcg rnd{99};
static uint64_t small8() { return rnd.small8(); }

// ---- add / sub of a plaintext, budget, 3-component products ---------------------------------------------------------------------
static void plain_add() {
    FheParams p5 = FheParams::n8192(5);
    FheParams p2 = p5;
    p2.moduli.resize(2); p2.psi.resize(2);
    const size_t n = p5.n(), B = 3;
    Context ctx5(p5, 0), ctx2(p2, 0);
    Evaluator ev5(ctx5), ev2(ctx2);
    KeyGenerator kg(ctx5, TestSeed{41});
    SecretKey sk2(ctx2, kg.secret_key().coefficients());
    Encryptor enc(ctx5, kg.secret_key(), TestSeed{42}), enc2(ctx2, sk2, TestSeed{43});
    Decryptor dec(ctx5, kg.secret_key()), dec2(ctx2, sk2);
    const uint64_t t = T_MOD;
    std::vector<int64_t> m(B * n), b(B * n);
    for (auto& v : m) v = (int64_t)rnd(t);
    for (size_t i = 0; i < B * n; ++i) b[i] = (int64_t)rnd(t) - (int64_t)(t / 2);   // centred coefficients
    b[0] = 0; b[1] = (int64_t)t - 1; b[2] = -(int64_t)t / 2;
    Ciphertext ct(ctx5, 2, B), sum(ctx5, 2, B);
    enc.encrypt_exact(m.data(), t, ct);
    const double before = dec.noise_budget_bits(ct, t);
    std::vector<uint64_t> dm(B * n);
    for (size_t items : {(size_t)1, B}) {
        ExactPlaintext pt(ctx5, t, items);
        CHECK(pt.items() == items && pt.plain_modulus() == t && pt.ring_degree() == n);
        pt.set_coefficients(b.data());
        auto bm = [&](size_t i, size_t k) { return ((b[(items == 1 ? 0 : i) * n + k] % (int64_t)t) + (int64_t)t) % (int64_t)t; };
        ev5.add_plain_exact(ct, pt, sum);
        dec.decrypt_exact(sum, t, dm.data());
        size_t bad = 0;
        for (size_t i = 0; i < B; ++i)
            for (size_t k = 0; k < n; ++k) bad += dm[i * n + k] != (uint64_t)((m[i * n + k] + bm(i, k)) % (int64_t)t);
        CHECK(bad == 0);
        const double after = dec.noise_budget_bits(sum, t);
        CHECK(before - after < 1.0);
        ev5.sub_plain_exact(sum, pt, sum);   // in place: back to m
        dec.decrypt_exact(sum, t, dm.data());
        bad = 0;
        for (size_t i = 0; i < B * n; ++i) bad += dm[i] != (uint64_t)m[i];
        CHECK(bad == 0);
        ev5.sub_plain_exact(ct, pt, sum);
        dec.decrypt_exact(sum, t, dm.data());
        bad = 0;
        for (size_t i = 0; i < B; ++i)
            for (size_t k = 0; k < n; ++k) bad += dm[i * n + k] != (uint64_t)((m[i * n + k] - bm(i, k) + (int64_t)t) % (int64_t)t);
        CHECK(bad == 0);
        CHECK(before - dec.noise_budget_bits(sum, t) < 1.0);
    }
    // the other components are untouched (out of place: copied)
    {
        ExactPlaintext pt(ctx5, t, 1);
        pt.set_coefficients(b.data());
        ev5.add_plain_exact(ct, pt, sum);
        const std::vector<uint64_t> a = words(ct), s = words(sum);
        const size_t per = p5.n_limbs() * n;
        size_t diff = 0;
        for (size_t i = 0; i < B; ++i) diff += std::memcmp(&a[(2 * i + 1) * per], &s[(2 * i + 1) * per], per * 8) != 0;
        CHECK(diff == 0);
    }
    // a 3-component ExactMultiplier product plus b, decrypted before relinearisation; the plaintext from slots
    {
        BatchEncoder be2(ctx2, t);
        ExactMultiplier mul(ctx5, ctx2, t);
        std::vector<uint64_t> sx(B * n), sb(B * n), got(n), dd(B * n);
        std::vector<int64_t> cx(B * n);
        for (auto& v : sx) v = rnd(t);
        for (auto& v : sb) v = rnd(t);
        for (size_t i = 0; i < B; ++i) be2.encode(&sx[i * n], &cx[i * n]);
        Ciphertext a(ctx2, 2, B), sq(ctx2, 3, B), out(ctx2, 3, B);
        enc2.encrypt_exact(cx.data(), t, a);
        mul.multiply(a, a, sq);
        ExactPlaintext pb(ctx2, t, B);
        pb.set_slots(be2, sb.data());
        const double b3 = dec2.noise_budget_bits(sq, t);
        ev2.add_plain_exact(sq, pb, out);
        ctx2.synchronize();
        dec2.decrypt_exact(out, t, dd.data());
        size_t bad = 0;
        for (size_t i = 0; i < B; ++i) {
            be2.decode(&dd[i * n], got.data());
            for (size_t k = 0; k < n; ++k) bad += got[k] != (uint64_t)(((unsigned __int128)sx[i * n + k] * sx[i * n + k] + sb[i * n + k]) % t);
        }
        CHECK(bad == 0);
        CHECK(b3 - dec2.noise_budget_bits(out, t) < 1.0);
        ev2.add_plain_exact(sq, pb, sq);   // in place on three components
        CHECK(words(sq) == words(out));
    }
    // rejections
    ExactPlaintext pt(ctx5, t, 2);
    Ciphertext c3(ctx5, 2, 3), c4(ctx5, 2, 4), c4o(ctx5, 3, 4), cn(ctx5, 2, 4, /*is_ntt=*/true);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ev5.add_plain_exact(c3, pt, c3); }, "batch not a multiple of the plaintext items");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ev5.add_plain_exact(c4, pt, c4o); }, "output shape differs");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ev5.sub_plain_exact(cn, pt, cn); }, "NTT-domain input");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ExactPlaintext bad(ctx5, 65536); }, "even plaintext modulus");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ExactPlaintext bad(ctx5, (1ull << 32) + 1); }, "plaintext modulus >= 2^32");
    Context small(FheParams::n4096_l4(), 0);
    ExactPlaintext other(small, t, 1);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ev5.add_plain_exact(c4, other, c4); }, "plaintext of another ring degree");
    std::printf("plain add: budget %.1f bits fresh\n", before);
}

// ---- PackedLinear with a bias ------------------------------------------------------------------------------------------------------
static void packed_bias(const FheParams& p, uint64_t special, uint64_t special_psi, const std::vector<std::vector<size_t>>& shapes) {
    const size_t n = p.n(), row = n / 2, T = 8;
    Context ctx(p, 0);
    KeyGenerator kg(ctx, TestSeed{51});
    Encryptor enc(ctx, kg.secret_key(), TestSeed{52});
    Decryptor dec(ctx, kg.secret_key());
    BatchEncoder be(ctx, T_MOD);
    HybridKeySwitcher hks(ctx, kg.secret_key(), special, special_psi, TestSeed{53});
    for (const auto& sh : shapes) {
        const size_t out = sh[0], in = sh[1], tpc = sh[2];
        std::vector<uint64_t> W(out * in), bias(out), x(T * in);
        for (auto& v : W) v = small8();
        for (auto& v : bias) v = rnd(T_MOD);
        for (auto& v : x) v = small8();
        PackedLinear lin(ctx, be, hks, W.data(), out, in, tpc, bias.data());
        CHECK(lin.has_bias());
        const size_t outs = lin.output_ciphertexts(), C = T / tpc;
        std::vector<uint64_t> slots(n);
        std::vector<int64_t> cx(C * n);
        for (size_t c = 0; c < C; ++c) {
            if (tpc == 1) lin.pack_input(&x[c * in], slots.data());
            else lin.pack_input_rows(&x[2 * c * in], &x[(2 * c + 1) * in], slots.data());
            be.encode(slots.data(), &cx[c * n]);
        }
        Ciphertext cxt(ctx, 2, C), cy(ctx, 2, outs * C);
        enc.encrypt_exact(cx.data(), T_MOD, cxt);
        lin.apply(cxt, cy);
        ctx.synchronize();
        std::vector<uint64_t> dm(outs * C * n), got(outs * n), y0(out), y1(out);
        dec.decrypt_exact(cy, T_MOD, dm.data());
        size_t bad = 0, bad_period = 0;
        for (size_t c = 0; c < C; ++c) {
            for (size_t o = 0; o < outs; ++o) be.decode(&dm[(o * C + c) * n], &got[o * n]);
            const std::vector<uint64_t> w0 = affine(W, bias.data(), out, in, &x[tpc * c * in], T_MOD);
            const std::vector<uint64_t> w1 = tpc == 2 ? affine(W, bias.data(), out, in, &x[(2 * c + 1) * in], T_MOD) : w0;
            if (tpc == 1) lin.unpack_output(got.data(), y0.data());
            else lin.unpack_output_rows(got.data(), y0.data(), y1.data());
            bad += y0 != w0;
            if (tpc == 2) bad += y1 != w1;
            // one output block: the output (bias included) repeats with period dim() - a valid input of the next layer
            if (outs == 1 && out <= lin.dim())
                for (size_t s = 0; s < n; ++s) {
                    const size_t r = (s % row) % lin.dim();
                    const std::vector<uint64_t>& w = (tpc == 2 && s >= row) ? w1 : w0;
                    bad_period += got[s] != (r < out ? w[r] : 0);
                }
        }
        if (bad || bad_period) std::printf("  shape out %zu in %zu tpc %zu: %zu wrong outputs, %zu wrong periodic slots\n", out, in, tpc, bad, bad_period);
        CHECK(bad == 0 && bad_period == 0);
        // a null bias is the old layer, word for word
        if (sh.size() > 3) {
            PackedLinear plain(ctx, be, hks, W.data(), out, in, tpc), nul(ctx, be, hks, W.data(), out, in, tpc, nullptr);
            CHECK(!plain.has_bias() && !nul.has_bias());
            Ciphertext ya(ctx, 2, outs * C), yb(ctx, 2, outs * C);
            plain.apply(cxt, ya);
            nul.apply(cxt, yb);
            ctx.synchronize();
            CHECK(words(ya) == words(yb));
        }
    }
    std::vector<uint64_t> W(16 * 16, 1), bias(16, T_MOD);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { PackedLinear bad(ctx, be, hks, W.data(), 16, 16, 1, bias.data()); }, "bias >= t");
    std::printf("packed bias at N = %zu: %zu shapes\n", n, shapes.size());
}

// ---- PackedTransformerBlock with all four biases -------------------------------------------------------------------------------------
static void block_bias() {
    uint64_t special = 0, special_psi = 0;
    const FheParams p = ring(11, 5, special, special_psi);
    const size_t n = p.n(), row = n / 2, d = 16, h = 520, T = 3, pd = 16;
    Context ctx(p, 0);
    KeyGenerator kg(ctx, TestSeed{61});
    Encryptor enc(ctx, kg.secret_key(), TestSeed{62});
    Decryptor dec(ctx, kg.secret_key());
    BatchEncoder be(ctx, T_MOD);
    HybridKeySwitcher hks(ctx, kg.secret_key(), special, special_psi, TestSeed{63});
    std::vector<uint64_t> Wqkv(3 * d * d), Wo(d * d), Wu(h * d), Wd(d * h), bqkv(3 * d), bo(d), bu(h), bd(d), x(T * d);
    for (auto* v : {&Wqkv, &Wo, &Wu, &Wd, &x})
        for (auto& e : *v) e = small8();
    for (auto* v : {&bqkv, &bo, &bu, &bd})
        for (auto& e : *v) e = rnd(T_MOD);
    PackedTransformerBlock blk(ctx, be, hks, Wqkv.data(), Wo.data(), Wu.data(), Wd.data(), d, h, bqkv.data(), bo.data(), bu.data(), bd.data());
    std::vector<uint64_t> slots(n);
    std::vector<int64_t> cx(T * n);
    for (size_t tk = 0; tk < T; ++tk) {
        blk.pack_input(&x[tk * d], slots.data());
        be.encode(slots.data(), &cx[tk * n]);
    }
    Ciphertext cxt(ctx, 2, T), cy(ctx, 2, T);
    enc.encrypt_exact(cx.data(), T_MOD, cxt);
    blk.apply(cxt, cy);
    ctx.synchronize();
    std::vector<uint64_t> dm(T * n), got(n);
    size_t bad[5] = {0, 0, 0, 0, 0};
    for (int st = 0; st < 5; ++st) {
        dec.decrypt_exact(blk.stage(st), T_MOD, dm.data());
        for (size_t tk = 0; tk < T; ++tk) {
            const uint64_t* xt = &x[tk * d];
            const std::vector<uint64_t> qkv = affine(Wqkv, bqkv.data(), 3 * d, d, xt, T_MOD);
            const std::vector<uint64_t> o = affine(Wo, bo.data(), d, d, &qkv[2 * d], T_MOD);
            std::vector<uint64_t> h1(d), h2(d);
            for (size_t i = 0; i < d; ++i) h1[i] = (xt[i] + o[i]) % T_MOD;
            const std::vector<uint64_t> u = affine(Wu, bu.data(), h, d, h1.data(), T_MOD);
            const std::vector<uint64_t> dn = affine(Wd, bd.data(), d, h, u.data(), T_MOD);
            for (size_t i = 0; i < d; ++i) h2[i] = (h1[i] + dn[i]) % T_MOD;
            be.decode(&dm[tk * n], got.data());
            for (size_t s = 0; s < n; ++s) {
                uint64_t want;
                if (st == 0) want = s < 3 * d ? qkv[s] : 0;                        // q | k | v at slots 0 .. 3d - 1 of row 0
                else if (st == 3) want = (s % row) < h ? u[s % row] : 0;           // W_up h1 + b_up with period N/2 on both rows
                else {                                                             // v + b_v, h1, h2: period pd on both rows
                    const size_t c = (s % row) % pd;
                    const uint64_t* w = st == 1 ? &qkv[2 * d] : st == 2 ? h1.data() : h2.data();
                    want = c < d ? w[c] : 0;
                }
                bad[st] += got[s] != want;
            }
        }
    }
    for (int st = 0; st < 5; ++st) {
        if (bad[st]) std::printf("  block stage %d: %zu wrong slots\n", st, bad[st]);
        CHECK(bad[st] == 0);
    }
    CHECK(words(cy) == words(blk.stage(4)));
    std::printf("block with biases: budget after h2 %.1f bits\n", dec.noise_budget_bits(cy, T_MOD));
}

// ---- activated FFN with biases: W_down (W_up x + b_up)^2 + b_down, modulus switch 5 -> 2 limbs (examples/encrypted_gpt2_ffn_act.cpp) ----------
static void ffn_act_bias() {
    FheParams p5 = FheParams::n8192_l6();
    const uint64_t special = p5.moduli.back(), special_psi = p5.psi.back();
    p5.moduli.pop_back(); p5.psi.pop_back();
    const FheParams p4 = p5.drop_last_limb(), p3 = p4.drop_last_limb(), p2 = p3.drop_last_limb();
    const size_t n = p5.n(), d = 64, h = 2100, T = 2;
    Context ctx5(p5, 0), ctx4(p4, 0), ctx3(p3, 0), ctx2(p2, 0);
    Evaluator ev5(ctx5), ev4(ctx4), ev3(ctx3);
    KeyGenerator kg(ctx5, TestSeed{71});
    SecretKey sk2(ctx2, kg.secret_key().coefficients());
    Encryptor enc(ctx5, kg.secret_key(), TestSeed{72});
    Decryptor dec2(ctx2, sk2);
    BatchEncoder be5(ctx5, T_MOD), be2(ctx2, T_MOD);
    HybridKeySwitcher hks5(ctx5, kg.secret_key(), special, special_psi, TestSeed{73}), hks2(ctx2, sk2, special, special_psi, TestSeed{74});
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
    up.apply(cx, c1);                                          // W_up x + b_up: outputs at slot r of row 0
    hks5.apply_galois_many(c1, std::vector<uint32_t>(T, row_swap), c1s);
    ev5.add(c1, c1s, c1r);                                     // down's input packing (period N/2 on both rows)
    ev5.rescale(c1r, u4); ev4.rescale(u4, u3); ev3.rescale(u3, u2);
    mul.multiply(u2, u2, sq3);
    hks2.relinearize(sq3, sq);
    down.apply(sq, cy);
    ctx5.synchronize();
    ctx2.synchronize();
    std::vector<uint64_t> dm(T * n), got(n), y(d);
    dec2.decrypt_exact(cy, T_MOD, dm.data());
    size_t bad = 0;
    for (size_t tk = 0; tk < T; ++tk) {
        std::vector<uint64_t> u = affine(Wu, bu.data(), h, d, &x[tk * d], T_MOD);
        for (auto& v : u) v = (uint64_t)((unsigned __int128)v * v % T_MOD);
        const std::vector<uint64_t> want = affine(Wd, bd.data(), d, h, u.data(), T_MOD);
        be2.decode(&dm[tk * n], got.data());
        down.unpack_output(got.data(), y.data());
        bad += y != want;
    }
    CHECK(bad == 0);
    std::printf("activated FFN with biases: budget %.1f bits\n", dec2.noise_budget_bits(cy, T_MOD));
}

int main() {
    try {
        plain_add();
        {
            const FheParams full = FheParams::n8192(5);
            FheParams p = full;
            p.moduli.pop_back(); p.psi.pop_back();
            const size_t N = p.n();
            // {out, in, tokens per ciphertext[, compare with the unbiased constructor]}: square | several output ciphertexts | wide input (folded)
            packed_bias(p, full.moduli.back(), full.psi.back(),
                        {{64, 64, 1, 1}, {64, 64, 2}, {N + 40, 16, 1, 1}, {N + 40, 16, 2}, {16, 128, 1, 1}, {16, 128, 2}, {77, 24, 1}});
        }
        {
            const FheParams full = FheParams::n16384(4);
            FheParams p = full;
            p.moduli.pop_back(); p.psi.pop_back();
            packed_bias(p, full.moduli.back(), full.psi.back(), {{256, 256, 2, 1}});
        }
        block_bias();
        ffn_act_bias();
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    return finish("affine C++ facade OK");
}
