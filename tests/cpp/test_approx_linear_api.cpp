// GPU test of the approximate packed layer in the C++ facade (ApproxPackedLinear, Evaluator::add_plain / sub_plain): every unpacked output of every shape
// lies within ApproxPackedLinear::error_bound of the float64 W x + b, that bound is at most 2^-10 and the reference has max|y| >= 1 on every case (a
// wrong diagonal, rotation, scale or level gives errors of order max|y|); apply() returns while its stream is held (the gate of tests/cpp/facade_test.h) and
// gives the same words there.  Built and run by tests/test_gpu_approx_linear.py (-m gpu).
// `test_approx_linear_api ref` only draws the cases and prints max|y| of each (no device).  Exit code 0 = all checks passed.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#define FACADE_TEST_GATE
#include "facade_test.h"

using namespace deeppowers::fhe;
using namespace facade_test;
typedef std::complex<double> cplx;

static SplitMix64 g_rng;   // every case sets its state
static double uni() { return g_rng.sym(); }
static const uint64_t kSeed = 7;
static const double kInputScale = std::ldexp(1.0, 50), kWeightScale = std::ldexp(1.0, 58);

struct Shape { unsigned log2n; size_t out_dim, in_dim, T, tpc; const char* what; };
static const Shape kShapes[] = {
    {11, 16, 16, 3, 1, "16 x 16: one block, replicated output; odd T"},
    {11, 77, 24, 3, 1, "77 x 24: ragged, several blocks; odd T"},
    {11, 12, 100, 8, 2, "12 x 100: wide input, fold rotations; two tokens per ciphertext"},
    {10, 600, 200, 2, 1, "600 x 200 at N = 1024: two output ciphertexts"},
};

// one case: W, bias, the T * tpc input vectors and the float64 reference, drawn from (kSeed, shape index, with_bias) alone
struct Case {
    std::vector<double> W, b, x, y;   // x: [T * tpc][in_dim], y: [T * tpc][out_dim]
    double ymax = 0;
    Case(const Shape& s, size_t index, bool with_bias) {
        g_rng.state = kSeed * 1000 + index * 2 + (with_bias ? 1 : 0);
        const size_t tokens = s.T * s.tpc;
        W.resize(s.out_dim * s.in_dim); b.resize(s.out_dim); x.resize(tokens * s.in_dim); y.resize(tokens * s.out_dim);
        for (auto& v : W) v = uni();
        for (auto& v : b) v = uni();
        for (auto& v : x) v = uni();
        for (size_t t = 0; t < tokens; ++t)
            for (size_t r = 0; r < s.out_dim; ++r) {
                double acc = with_bias ? b[r] : 0.0;
                for (size_t c = 0; c < s.in_dim; ++c) acc += W[r * s.in_dim + c] * x[t * s.in_dim + c];
                y[t * s.out_dim + r] = acc;
                ymax = std::max(ymax, std::fabs(acc));
            }
    }
};

struct Rig {
    uint64_t special = 0, special_psi = 0;
    FheParams p, pn;
    Context ctx, next;
    KeyGenerator kg;
    SecretKey sk_next;
    HybridKeySwitcher hks;
    ComplexEncoder cenc;
    Encryptor enc;
    Decryptor dec;
    explicit Rig(unsigned log2n)
        : p(ring(log2n, 3, special, special_psi)), pn(p.drop_last_limb()), ctx(p, 0), next(pn, 0), kg(ctx, TestSeed{11}),
          sk_next(next, kg.secret_key().coefficients()), hks(ctx, kg.secret_key(), special, special_psi, TestSeed{12}), cenc(ctx),
          enc(ctx, kg.secret_key(), TestSeed{13}), dec(next, sk_next) {}
};

// encrypts the case's tokens, applies the layer, returns the decoded slots [passes * T][N/2]
static std::vector<cplx> run_layer(Rig& r, const Shape& s, const Case& c, const ApproxPackedLinear& lin, Ciphertext& cx, Ciphertext& cy, Stream* stream = nullptr) {
    const size_t N = r.p.n(), row = N / 2, passes = lin.output_ciphertexts();
    std::vector<int64_t> msg(s.T * N);
    std::vector<cplx> slots(row);
    for (size_t t = 0; t < s.T; ++t) {
        if (s.tpc == 2) lin.pack_input_pair(&c.x[(2 * t) * s.in_dim], &c.x[(2 * t + 1) * s.in_dim], slots.data());
        else lin.pack_input(&c.x[t * s.in_dim], slots.data());
        r.cenc.encode(slots.data(), kInputScale, &msg[t * N]);
    }
    r.enc.encrypt(msg.data(), 0, cx);
    lin.apply(cx, cy, stream);
    if (stream) (void)hipStreamSynchronize(static_cast<hipStream_t>(stream));
    r.next.synchronize();
    CHECK(!cy.is_ntt() && cy.batch() == passes * s.T && cy.size() == 2 && cy.words() == passes * s.T * 2 * r.pn.n_limbs() * N);   // coefficient domain on next_ctx
    std::vector<int64_t> out(passes * s.T * N);
    r.dec.decrypt(cy, 0, out.data());
    std::vector<cplx> z(passes * s.T * row);
    for (size_t i = 0; i < passes * s.T; ++i) r.cenc.decode(&out[i * N], lin.output_scale(), &z[i * row]);
    return z;
}

static void run_shape(Rig& r, const Shape& s, size_t index, bool with_bias) {
    const Case c(s, index, with_bias);
    const size_t N = r.p.n(), row = N / 2;
    ApproxPackedLinear lin(r.ctx, r.next, r.cenc, r.hks, c.W.data(), s.out_dim, s.in_dim, kWeightScale, kInputScale, s.tpc, with_bias ? c.b.data() : nullptr);
    const size_t passes = lin.output_ciphertexts();
    CHECK(lin.has_bias() == with_bias && lin.tokens_per_ciphertext() == s.tpc && lin.baby_steps() * lin.giant_steps() == lin.dim());
    CHECK(std::fabs(lin.output_scale() - kInputScale * kWeightScale / (double)r.p.moduli.back()) <= lin.output_scale() * 1e-15);
    Ciphertext cx(r.ctx, 2, s.T), cy(r.next, 2, passes * s.T);
    const std::vector<cplx> z = run_layer(r, s, c, lin, cx, cy);
    // the fresh ciphertext's phase error: the sampler's |e| <= 21, the rounding 1/2 and the encoder's E at input_scale (slots of modulus <= sqrt(tpc))
    const double xmax = 1.0, e_x = 8.0 * s.log2n * std::ldexp(1.0, -53) * kInputScale * xmax * std::sqrt((double)s.tpc);
    const double bound = lin.error_bound(xmax, 21.0 + 0.5 + e_x);
    double worst = 0;
    size_t checked = 0;
    // every slot that holds a row (so every periodic copy of a replicated or folded output), every token, both parts with two tokens per ciphertext
    for (size_t o = 0; o < passes; ++o)
        for (size_t t = 0; t < s.T; ++t)
            for (size_t sl = 0; sl < row; ++sl) {
                const size_t R = lin.row_of_slot(o, sl);
                if (R == (size_t)-1) continue;
                const cplx v = z[(o * s.T + t) * row + sl];
                for (size_t part = 0; part < s.tpc; ++part) {
                    const double want = c.y[(t * s.tpc + part) * s.out_dim + R];
                    worst = std::max(worst, std::fabs((part ? v.imag() : v.real()) - want));
                    ++checked;
                }
                if (s.tpc == 1) worst = std::max(worst, std::fabs(v.imag()));   // one token: the imaginary parts decode to zero
            }
    // ... and through unpack_output: every row is found
    std::vector<double> ya(s.out_dim, 1e300), yb(s.out_dim, 1e300);
    std::vector<cplx> tok(passes * row);
    for (size_t t = 0; t < s.T; ++t) {
        for (size_t o = 0; o < passes; ++o) std::memcpy(&tok[o * row], &z[(o * s.T + t) * row], row * sizeof(cplx));
        if (s.tpc == 2) lin.unpack_output_pair(tok.data(), ya.data(), yb.data());
        else lin.unpack_output(tok.data(), ya.data());
        for (size_t R = 0; R < s.out_dim; ++R) {
            worst = std::max(worst, std::fabs(ya[R] - c.y[(t * s.tpc) * s.out_dim + R]));
            if (s.tpc == 2) worst = std::max(worst, std::fabs(yb[R] - c.y[(t * s.tpc + 1) * s.out_dim + R]));
        }
    }
    std::printf("%-70s bias %d: passes %zu, n1 x n2 = %zu x %zu, %zu key switches; max|y| %.3f, max error 2^%.2f, error_bound 2^%.2f (%zu slots)\n", s.what,
                (int)with_bias, passes, lin.baby_steps(), lin.giant_steps(), lin.key_switches_per_apply(), c.ymax, std::log2(worst), std::log2(bound), checked);
    CHECK(bound <= std::ldexp(1.0, -10));
    CHECK(c.ymax >= 1.0);
    CHECK(checked >= s.out_dim * s.T * s.tpc);
    CHECK(worst <= bound);
}

// a null bias gives the words of the bias-less constructor; apply() behind the gate returns while the stream is held and gives the same words
static void words_and_stream(Rig& r, Gate& gate) {
    const Shape& s = kShapes[1];
    const Case c(s, 1, false);
    ApproxPackedLinear a(r.ctx, r.next, r.cenc, r.hks, c.W.data(), s.out_dim, s.in_dim, kWeightScale, kInputScale);
    ApproxPackedLinear b(r.ctx, r.next, r.cenc, r.hks, c.W.data(), s.out_dim, s.in_dim, kWeightScale, kInputScale, 1, nullptr);
    CHECK(!a.has_bias() && !b.has_bias());
    Ciphertext cx(r.ctx, 2, s.T), ya(r.next, 2, a.output_ciphertexts() * s.T), yb(r.next, 2, b.output_ciphertexts() * s.T);
    run_layer(r, s, c, a, cx, ya);
    const std::vector<uint64_t> wa = words(ya);
    b.apply(cx, yb);
    r.next.synchronize();
    CHECK(words(yb) == wa);
    // the gate, with the full protocol: the warm-up (keys packed, scratch at its size) and the gate on zero words in the input buffer, the encrypted tokens
    // copied in on S behind the gate, the output wiped on S behind it; the call comes back with the event pending, within G / 4, with the same words
    Ciphertext gx(r.ctx, 2, s.T), zero(r.ctx, 2, s.T);
    HIP(hipMemset(zero.data(), 0, zero.words() * 8));
    const double t_enqueue = gate.gated("ApproxPackedLinear::apply", {late(gx, zero, cx)}, {out_of(yb)}, [&](Stream* st) { b.apply(gx, yb, st); });
    CHECK(words(yb) == wa);
    std::printf("ApproxPackedLinear::apply behind the gate: t_enqueue %.3f ms, G %.1f ms\n", t_enqueue * 1e3, gate.G * 1e3);

    // Evaluator::add_plain / sub_plain on the layer's output: back to the input's words; both domains; the domain flags must agree
    Evaluator ev(r.next);
    const size_t poly = r.pn.n_limbs() * r.pn.n();
    for (size_t items : {(size_t)1, (size_t)s.T}) {
        Plaintext pt(r.next, items);
        std::vector<uint64_t> pw(items * poly);
        g_rng.state = 99 + items;
        for (size_t i = 0; i < pw.size(); ++i) {
            const uint64_t q = r.pn.moduli[(i / r.pn.n()) % r.pn.n_limbs()];
            pw[i] = (i % 5 == 0) ? q - 1 : (uint64_t)((uni() + 1.0) / 2.0 * (double)(q - 1));
        }
        pt.copy_from_host(pw.data());
        Ciphertext sum(r.next, 2, ya.batch());
        ev.add_plain(ya, pt, sum);
        r.next.synchronize();
        const std::vector<uint64_t> ws = words(sum);
        size_t c0_changed = 0, c1_changed = 0;
        for (size_t i = 0; i < ya.batch(); ++i) {
            c0_changed += std::memcmp(&ws[(2 * i) * poly], &wa[(2 * i) * poly], poly * 8) != 0;
            c1_changed += std::memcmp(&ws[(2 * i + 1) * poly], &wa[(2 * i + 1) * poly], poly * 8) != 0;
        }
        CHECK(c0_changed == ya.batch() && c1_changed == 0 && !sum.is_ntt());
        ev.sub_plain(sum, pt, sum);   // in place
        r.next.synchronize();
        CHECK(words(sum) == wa);
        pt.set_ntt(true);
        expect_error(ErrorCode::INVALID_STATE, [&] { ev.add_plain(ya, pt, sum); }, "add_plain, domains differ");
        expect_error(ErrorCode::INVALID_STATE, [&] { ev.sub_plain(ya, pt, sum); }, "sub_plain, domains differ");
        sum.set_ntt(true);            // (flags only: the entry adds words as they are)
        ev.add_plain(sum, pt, sum);
        CHECK(sum.is_ntt());
        sum.set_ntt(false);
    }
    Plaintext three(r.next, 2);
    Ciphertext out(r.next, 2, ya.batch()), small(r.next, 2, 1), full(r.ctx, 2, ya.batch());
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ev.add_plain(ya, three, out); }, "add_plain, batch not a multiple of the plaintext's items");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { Plaintext one(r.next, 1); ev.add_plain(ya, one, small); }, "add_plain, output shape");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { Plaintext one(r.next, 1); ev.add_plain(full, one, full); }, "add_plain, ciphertext of another context");
}

static void rejections(Rig& r) {
    const Shape& s = kShapes[0];
    Case c(s, 0, true);
    auto build = [&](const Context& next, const double* W, const double* b, double ws, double xs, size_t tpc) {
        ApproxPackedLinear lin(r.ctx, next, r.cenc, r.hks, W, s.out_dim, s.in_dim, ws, xs, tpc, b);
    };
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.ctx, c.W.data(), nullptr, kWeightScale, kInputScale, 1); }, "next_ctx = data_ctx");
    {
        FheParams other = r.pn;
        std::swap(other.moduli[0], other.moduli[1]); std::swap(other.psi[0], other.psi[1]);
        Context wrong(other, 0);
        expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(wrong, c.W.data(), nullptr, kWeightScale, kInputScale, 1); }, "next_ctx with other limbs");
    }
    std::vector<double> W = c.W;
    W[5] = 16.0;   // 2^58 * 16 = 2^62
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.next, W.data(), nullptr, kWeightScale, kInputScale, 1); }, "weight at the clamp");
    W[5] = std::nan("");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.next, W.data(), nullptr, kWeightScale, kInputScale, 1); }, "NaN weight");
    W[5] = INFINITY;
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.next, W.data(), nullptr, kWeightScale, kInputScale, 1); }, "infinite weight");
    std::vector<double> b = c.b;
    b[3] = std::nan("");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.next, c.W.data(), b.data(), kWeightScale, kInputScale, 1); }, "NaN bias");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.next, c.W.data(), nullptr, 0.0, kInputScale, 1); }, "weight_scale 0");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.next, c.W.data(), nullptr, kWeightScale, std::nan(""), 1); }, "input_scale NaN");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.next, c.W.data(), nullptr, kWeightScale, kInputScale, 3); }, "three tokens per ciphertext");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.next, nullptr, nullptr, kWeightScale, kInputScale, 1); }, "null matrix");
    // apply: the output must sit on next_ctx
    ApproxPackedLinear lin(r.ctx, r.next, r.cenc, r.hks, c.W.data(), s.out_dim, s.in_dim, kWeightScale, kInputScale);
    Ciphertext cx(r.ctx, 2, 1), same_level(r.ctx, 2, 1), two(r.next, 2, 2);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { lin.apply(cx, same_level); }, "apply, output on data_ctx");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { lin.apply(cx, two); }, "apply, output batch");
}

int main(int argc, char** argv) {
    const size_t n_shapes = sizeof kShapes / sizeof kShapes[0];
    if (argc > 1 && std::string(argv[1]) == "ref") {
        for (size_t i = 0; i < n_shapes; ++i)
            for (int bias = 0; bias < 2; ++bias) std::printf("%s, bias %d: max|y| = %.4f\n", kShapes[i].what, bias, Case(kShapes[i], i, bias != 0).ymax);
        return 0;
    }
    const double G = argc > 1 ? std::atof(argv[1]) : 0.040;
    try {
        Gate gate(G);
        if (!gate.ok()) { std::printf("no non-blocking stream\n"); return 2; }
        {
            Rig r11(11);
            for (size_t i = 0; i < 3; ++i)
                for (int bias = 0; bias < 2; ++bias) run_shape(r11, kShapes[i], i, bias != 0);
            words_and_stream(r11, gate);
            rejections(r11);
        }
        {
            Rig r10(10);
            for (int bias = 0; bias < 2; ++bias) run_shape(r10, kShapes[3], 3, bias != 0);
        }
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    return finish("approximate packed layer C++ facade OK");
}
