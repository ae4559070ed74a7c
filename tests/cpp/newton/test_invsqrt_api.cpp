// GPU test of the Newton step and the inverse square root in the C++ facade (ScalarWeights, HybridKeySwitcher::multiply_lincomb_rescale_range,
// ApproxInvSqrt): on ENCRYPTED inputs every decoded slot of every token lies within the stated error bound of the float64 iteration
// y <- 1.5 y - 0.5 (v y)(y y) from the values encrypted, the bound is at most 2^-10 of min|Y_K| >= 1/2 (a wrong weight, scale, level or term gives errors of
// the order of the output); one fused product-plus-term-plus-constant within the bound of its own recurrence; both calls return while their stream is held
// (the gate of tests/cpp/facade_test.h) and give the same words there; the constructors' and the calls' rejections.  Built and run by
// tests/test_gpu_invsqrt.py (-m gpu).
// `test_invsqrt_api ref` only draws the cases and prints min|Y_K| and ApproxInvSqrt::error_bound of each (no device).  Exit code 0 = all passed.
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
#include "../facade_test.h"

using namespace deeppowers::fhe;
using namespace facade_test;
typedef std::complex<double> cplx;

static SplitMix64 g_rng;   // every case sets its state

static const unsigned kLog2N = 12;
static const size_t kSteps = 2, kDataLimbs = 2 * kSteps + 2, kTokens = 3;   // two limbs are left at the output
static const double kVScale = std::ldexp(1.0, 60), kVMin = 0.1, kVMax = 1.0, kGuessOff = 0.1;
static const double kU = std::ldexp(1.0, -53);

// one case: v uniform on [kVMin, kVMax], the guess (1 + d) / sqrt(v) with d uniform on [-kGuessOff, kGuessOff]; the float64 iteration
struct Case {
    size_t K;
    std::vector<double> v, y0, y;   // [kTokens][N/2]
    double vmax = 0, ymax = 0, ymin = 1e300, y0max = 0;
    explicit Case(size_t steps) : K(steps) {
        g_rng.state = 9000 + steps;
        const size_t row = ((size_t)1 << kLog2N) / 2;
        v.resize(kTokens * row); y0.resize(v.size()); y.resize(v.size());
        for (size_t i = 0; i < v.size(); ++i) {
            v[i] = kVMin + (kVMax - kVMin) * g_rng.unit();
            y0[i] = (1.0 + kGuessOff * g_rng.sym()) / std::sqrt(v[i]);
            double yn = y0[i];
            ymax = std::max(ymax, std::fabs(yn));
            for (size_t n = 0; n < K; ++n) {
                yn = 1.5 * yn - 0.5 * ((v[i] * yn) * (yn * yn));
                ymax = std::max(ymax, std::fabs(yn));
            }
            y[i] = yn;
            vmax = std::max(vmax, v[i]); y0max = std::max(y0max, std::fabs(y0[i])); ymin = std::min(ymin, std::fabs(yn));
        }
        ymax *= 1 + std::ldexp(1.0, -40);   // a bound on the real iterates too
    }
};

static double fresh_noise_bound(double scale, double X) { return 21.0 + 0.5 + 8.0 * kLog2N * kU * scale * X; }

struct Rig {
    uint64_t special = 0, special_psi = 0;
    std::vector<FheParams> params;
    std::vector<std::unique_ptr<Context>> ctx;                 // level 0 .. kDataLimbs - 1
    std::unique_ptr<KeyGenerator> kg;
    std::vector<std::unique_ptr<SecretKey>> sk;
    std::vector<std::unique_ptr<HybridKeySwitcher>> hks;       // level 0 .. 2 kSteps - 1
    std::unique_ptr<ComplexEncoder> cenc;
    std::unique_ptr<Encryptor> enc;
    double guess_scale = 0;
    Rig() {
        params.push_back(ring(kLog2N, kDataLimbs, special, special_psi));
        for (size_t r = 0; r + 1 < kDataLimbs; ++r) params.push_back(params.back().drop_last_limb());
        for (const FheParams& p : params) ctx.emplace_back(new Context(p, 0));
        kg.reset(new KeyGenerator(*ctx[0], TestSeed{11}));
        for (size_t r = 0; r < ctx.size(); ++r) sk.emplace_back(new SecretKey(*ctx[r], kg->secret_key().coefficients()));
        for (size_t r = 0; r < 2 * kSteps; ++r) hks.emplace_back(new HybridKeySwitcher(*ctx[r], *sk[r], special, special_psi, TestSeed{12 + r}));
        cenc.reset(new ComplexEncoder(*ctx[0]));
        enc.reset(new Encryptor(*ctx[0], kg->secret_key(), TestSeed{13}));
        guess_scale = ApproxInvSqrt::balanced_guess_scale(kVScale, params[0].moduli[kDataLimbs - 1], params[0].moduli[kDataLimbs - 2]);
    }
    std::vector<HybridKeySwitcher*> levels(size_t count) const {
        std::vector<HybridKeySwitcher*> v;
        for (size_t r = 0; r < count; ++r) v.push_back(hks[r].get());
        return v;
    }
    void encrypt(const double* slots, size_t items, double scale, Ciphertext& out) const {   // real slots [items][N/2]
        const size_t N = params[0].n(), row = N / 2;
        std::vector<int64_t> msg(items * N);
        std::vector<cplx> z(row);
        for (size_t t = 0; t < items; ++t) {
            for (size_t i = 0; i < row; ++i) z[i] = cplx(slots[t * row + i], 0.0);
            cenc->encode(z.data(), scale, &msg[t * N]);
        }
        enc->encrypt(msg.data(), 0, out);
    }
    std::vector<cplx> decrypt(const Ciphertext& ct, size_t level, double scale) const {
        const size_t N = params[0].n(), row = N / 2;
        Decryptor dec(*ctx[level], *sk[level]);
        std::vector<int64_t> out(ct.batch() * N);
        dec.decrypt(ct, 0, out.data());
        std::vector<cplx> z(ct.batch() * row);
        for (size_t i = 0; i < ct.batch(); ++i) cenc->decode(&out[i * N], scale, &z[i * row]);
        return z;
    }
};

static void run_invsqrt(Rig& r, size_t K) {
    const Case c(K);
    const size_t row = r.params[0].n() / 2;
    const FheParams& p0 = r.params[0];
    ApproxInvSqrt inv(r.levels(2 * K), *r.ctx[2 * K], kVScale, r.guess_scale);
    CHECK(inv.iterations() == K && inv.depth() == 2 * K && inv.scale(0) == r.guess_scale);
    {   // the scale rule, in its double operations
        const double q_a = (double)p0.moduli[kDataLimbs - 1], q_b = (double)p0.moduli[kDataLimbs - 2], s0 = r.guess_scale;
        const double top = 2.0 * (((kVScale * s0) / q_a) * ((s0 * s0) / q_a));
        CHECK(inv.weight(0) == std::llround(1.5 * (top / s0)) && inv.scale(1) == top / q_b);
        CHECK(std::fabs(inv.scale(K) / s0 - 1) < std::ldexp(1.0, -20));   // balanced
    }
    Ciphertext v(*r.ctx[0], 2, kTokens), y0(*r.ctx[0], 2, kTokens), y(*r.ctx[2 * K], 2, kTokens);
    r.encrypt(c.v.data(), kTokens, kVScale, v);
    r.encrypt(c.y0.data(), kTokens, r.guess_scale, y0);
    inv.apply(v, y0, y);
    r.ctx[0]->synchronize();
    CHECK(!y.is_ntt());
    const std::vector<cplx> z = r.decrypt(y, 2 * K, inv.scale(K));
    const double bound = inv.error_bound(c.vmax, c.ymax, fresh_noise_bound(kVScale, c.vmax), fresh_noise_bound(r.guess_scale, c.y0max));
    double worst = 0, newton = 0;
    for (size_t i = 0; i < kTokens * row; ++i) {
        worst = std::max(worst, std::max(std::fabs(z[i].real() - c.y[i]), std::fabs(z[i].imag())));
        newton = std::max(newton, std::fabs(c.y[i] * std::sqrt(c.v[i]) - 1));
    }
    std::printf("%zu Newton steps, %zu tokens, depth %zu: min|Y_K| %.3f, max error 2^%.2f, error_bound 2^%.2f (%zu slots); Y_K is within %.2e of 1/sqrt(v)\n", K,
                kTokens, inv.depth(), c.ymin, std::log2(worst), std::log2(bound), kTokens * row, newton);
    CHECK(c.ymin >= 0.5);
    CHECK(bound <= std::ldexp(1.0, -10) * c.ymin);
    CHECK(worst <= bound);
}

// round((a b + w_1 z + constant) / q) on encrypted inputs: the slot error by the header's recurrence for one fused step from fresh inputs, and the gate
static void run_multiply_lincomb(Rig& r, Gate& gate) {
    const size_t N = r.params[0].n(), row = N / 2, T = 2;
    const double sx = std::ldexp(1.0, 59), X = 2.0, konst = -1.25;
    g_rng.state = 4343;
    std::vector<double> xa(T * row), xb(T * row), xz(T * row);
    for (auto& v : xa) v = X * g_rng.sym();
    for (auto& v : xb) v = X * g_rng.sym();
    for (auto& v : xz) v = X * g_rng.sym();
    Ciphertext a(*r.ctx[0], 2, T), b(*r.ctx[0], 2, T), z(*r.ctx[0], 2, T), out(*r.ctx[1], 2, T);
    r.encrypt(xa.data(), T, sx, a);
    r.encrypt(xb.data(), T, sx, b);
    r.encrypt(xz.data(), T, sx, z);
    const double q = (double)r.params[0].moduli.back(), S = (sx * sx) / q;       // the output's scale
    const int64_t w1 = std::llround((sx * sx) / sx), c_out = std::llround(konst * S);
    ScalarWeights weights(*r.ctx[0], 1, {w1}, c_out);
    CHECK(weights.terms() == 1 && &weights.context() == r.ctx[0].get() && weights.data() != nullptr);
    r.hks[0]->multiply_lincomb_rescale_range(a, 0, b, 0, T, weights, {LincombTerm{&z, 0}}, out, 0);
    r.ctx[0]->synchronize();
    CHECK(!out.is_ntt());
    const double Nd = (double)N, H = (Nd + 1) / 2;
    uint64_t qmax = 0;
    for (uint64_t m : r.params[0].moduli) qmax = std::max(qmax, m);
    const double Kks = 21.0 * (double)kDataLimbs * Nd * ((double)qmax / (double)r.special), D1 = Nd * fresh_noise_bound(sx, X);
    const double R1 = 0.5 + 4 * kU * (double)w1;
    // the product of the phases, its relinearisation, the term's error under its weight, the weight's and the constant's roundings, all divided by q;
    // then the rescale's rounding and the scale's own
    const double E = (2 * sx * X * D1 + D1 * D1 + Nd * (Kks + H) + ((double)w1 + R1) * D1 + R1 * sx * X) / q + 0.5 + 2 * kU * std::fabs(konst) * S + Nd * H +
                     4 * kU * S * (X * X + X);
    const double big_bound = X * X + X + std::fabs(konst), pre = E / S, bound = pre + 8.0 * kLog2N * kU * Nd * (big_bound + pre);
    const std::vector<cplx> zz = r.decrypt(out, 1, S);
    double worst = 0, big = 0;
    for (size_t i = 0; i < T * row; ++i) {
        const double want = xa[i] * xb[i] + xz[i] + konst;
        worst = std::max(worst, std::max(std::fabs(zz[i].real() - want), std::fabs(zz[i].imag())));
        big = std::max(big, std::fabs(want));
    }
    std::printf("multiply_lincomb_rescale, %zu items: max|a b + z + c| %.3f, max error 2^%.2f, bound 2^%.2f\n", T, big, std::log2(worst), std::log2(bound));
    CHECK(big >= 1.0 && bound <= std::ldexp(1.0, -10) && worst <= bound);
    // without terms and with weight one it is multiply_rescale, word for word
    {
        Ciphertext plain(*r.ctx[1], 2, T), fused(*r.ctx[1], 2, T);
        ScalarWeights one(*r.ctx[0], 1, {}, 0);
        r.hks[0]->multiply_rescale(a, b, plain);
        r.hks[0]->multiply_lincomb_rescale_range(a, 0, b, 0, T, one, {}, fused, 0);
        r.ctx[0]->synchronize();
        CHECK(words(plain) == words(fused));
    }
    // ranges: item 1 of a times item 0 of b plus item 1 of z into item 1 of a fresh output; the other item stays
    Ciphertext part(*r.ctx[1], 2, T);
    CHECK(hipMemset(part.data(), 0, part.words() * 8) == hipSuccess);
    r.hks[0]->multiply_lincomb_rescale_range(a, 1, b, 0, 1, weights, {LincombTerm{&z, 1}}, part, 1);
    r.ctx[0]->synchronize();
    const std::vector<cplx> zp = r.decrypt(part, 1, S);
    double wp = 0;
    for (size_t i = 0; i < row; ++i) wp = std::max(wp, std::max(std::fabs(zp[row + i].real() - (xa[row + i] * xb[i] + xz[row + i] + konst)), std::abs(zp[i])));
    CHECK(wp <= bound);

    // the gate, with the full protocol: zero words in the three input buffers during the warm-up and the gate, the inputs copied in on S behind it, the
    // output wiped on S behind it; the call comes back with the event pending, within G / 4, and gives the words of the idle stream
    const std::vector<uint64_t> want = words(out);
    Ciphertext ga(*r.ctx[0], 2, T), gb(*r.ctx[0], 2, T), gz(*r.ctx[0], 2, T), zero(*r.ctx[0], 2, T);
    HIP(hipMemset(zero.data(), 0, zero.words() * 8));
    const double t_enqueue = gate.gated("HybridKeySwitcher::multiply_lincomb_rescale_range", {late(ga, zero, a), late(gb, zero, b), late(gz, zero, z)}, {out_of(out)},
                                        [&](Stream* s) { r.hks[0]->multiply_lincomb_rescale_range(ga, 0, gb, 0, T, weights, {LincombTerm{&gz, 0}}, out, 0, s); });
    CHECK(words(out) == want);
    std::printf("HybridKeySwitcher::multiply_lincomb_rescale_range behind the gate: t_enqueue %.3f ms, G %.1f ms\n", t_enqueue * 1e3, gate.G * 1e3);
}

static void invsqrt_behind_the_gate(Rig& r, Gate& gate) {
    const Case c(kSteps);
    ApproxInvSqrt inv(r.levels(2 * kSteps), *r.ctx[2 * kSteps], kVScale, r.guess_scale);
    Ciphertext v(*r.ctx[0], 2, kTokens), y0(*r.ctx[0], 2, kTokens), rv(*r.ctx[0], 2, kTokens), ry(*r.ctx[0], 2, kTokens), zero(*r.ctx[0], 2, kTokens),
        y(*r.ctx[2 * kSteps], 2, kTokens);
    r.encrypt(c.v.data(), kTokens, kVScale, rv);
    r.encrypt(c.y0.data(), kTokens, r.guess_scale, ry);
    HIP(hipMemset(zero.data(), 0, zero.words() * 8));
    inv.apply(rv, ry, y);
    r.ctx[0]->synchronize();
    const std::vector<uint64_t> want = words(y);
    const double t_enqueue = gate.gated("ApproxInvSqrt::apply", {late(v, zero, rv), late(y0, zero, ry)}, {out_of(y)}, [&](Stream* s) { inv.apply(v, y0, y, s); });
    CHECK(words(y) == want);
    std::printf("ApproxInvSqrt::apply behind the gate: t_enqueue %.3f ms, G %.1f ms\n", t_enqueue * 1e3, gate.G * 1e3);
}

static void rejections(Rig& r) {
    auto build = [&](const std::vector<HybridKeySwitcher*>& lv, const Context& out, double vs, double gs) { ApproxInvSqrt inv(lv, out, vs, gs); };
    const double gs = r.guess_scale;
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build({}, *r.ctx[0], kVScale, gs); }, "no levels");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.levels(3), *r.ctx[3], kVScale, gs); }, "an odd number of levels");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.levels(2), *r.ctx[1], kVScale, gs); }, "out_ctx one level too high");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.levels(2), *r.ctx[3], kVScale, gs); }, "out_ctx one level too low");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build({r.hks[1].get(), r.hks[0].get()}, *r.ctx[2], kVScale, gs); }, "levels out of order");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build({r.hks[0].get(), nullptr}, *r.ctx[2], kVScale, gs); }, "null level");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.levels(2), *r.ctx[2], 0.0, gs); }, "v_scale 0");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.levels(2), *r.ctx[2], kVScale, INFINITY); }, "guess_scale infinite");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.levels(2), *r.ctx[2], kVScale, std::ldexp(1.0, 19)); }, "s_0 below 2^20");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.levels(2), *r.ctx[2], kVScale, std::ldexp(1.0, 62)); }, "s_0 at 2^62");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.levels(2), *r.ctx[2], kVScale, 4 * gs); }, "a guess scale 4 times the balance: s_1 = 64 s_0 is out of range");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.levels(4), *r.ctx[4], kVScale, gs / 32); }, "a guess scale 1/32 of the balance: s_2 = 2^-45 of it is below 2^20");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.levels(2), *r.ctx[2], std::ldexp(1.0, 66), std::ldexp(1.0, 61)); }, "|w_0| above 2^62");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)ApproxInvSqrt::balanced_guess_scale(-1.0, 3, 5); }, "balanced_guess_scale, negative scale");
    ApproxInvSqrt inv(r.levels(2), *r.ctx[2], kVScale, gs);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)inv.scale(2); }, "scale(2) of one iteration");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)inv.weight(1); }, "weight(1) of one iteration");
    Ciphertext v(*r.ctx[0], 2, 2), y0(*r.ctx[0], 2, 2), y(*r.ctx[2], 2, 2), one(*r.ctx[2], 2, 1), high(*r.ctx[1], 2, 2), low(*r.ctx[1], 2, 2), three(*r.ctx[0], 3, 2);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { inv.apply(v, y0, high); }, "apply, output one level too high");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { inv.apply(v, y0, one); }, "apply, output batch");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { inv.apply(v, low, y); }, "apply, guess one level down");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { inv.apply(three, y0, y); }, "apply, 3 components");
    // ScalarWeights and the fused step
    const int64_t big = (int64_t)1 << 62;
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ScalarWeights w(*r.ctx[0], 1, std::vector<int64_t>(16, 1), 0); }, "ScalarWeights, 16 terms");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ScalarWeights w(*r.ctx[0], big, {}, 0); }, "ScalarWeights, product weight 2^62");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ScalarWeights w(*r.ctx[0], 1, {-big}, 0); }, "ScalarWeights, term weight -2^62");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ScalarWeights w(*r.ctx[0], 1, {}, big); }, "ScalarWeights, constant 2^62");
    expect_error(ErrorCode::INVALID_STATE, [&] { ScalarWeights w(*r.ctx[kDataLimbs - 1], 1, {}, 0); }, "ScalarWeights, one limb");
    ScalarWeights w0(*r.ctx[0], -1, {3}, 0), w1(*r.ctx[1], -1, {3}, 0), none(*r.ctx[0], 1, {}, 0), many(*r.ctx[0], 1, std::vector<int64_t>(15, big - 1), 1 - big);
    Ciphertext a(*r.ctx[0], 2, 2), o1(*r.ctx[1], 2, 2), o0(*r.ctx[0], 2, 2), z1(*r.ctx[1], 2, 2), zn(*r.ctx[0], 2, 2, true);
    auto step = [&](HybridKeySwitcher& ks, const Ciphertext& x, size_t first, size_t count, const ScalarWeights& w, const std::vector<LincombTerm>& terms, Ciphertext& out) {
        ks.multiply_lincomb_rescale_range(x, first, x, 0, count, w, terms, out, 0);
    };
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(*r.hks[0], a, 0, 2, w0, {}, o1); }, "fused step, a weight without its term");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(*r.hks[0], a, 0, 2, none, {LincombTerm{&a, 0}}, o1); }, "fused step, a term without its weight");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(*r.hks[0], a, 0, 2, w1, {LincombTerm{&a, 0}}, o1); }, "fused step, weights of another level");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(*r.hks[0], a, 0, 2, w0, {LincombTerm{&z1, 0}}, o1); }, "fused step, a term one level down");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(*r.hks[0], a, 0, 2, w0, {LincombTerm{nullptr, 0}}, o1); }, "fused step, null term");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(*r.hks[0], a, 0, 2, w0, {LincombTerm{&zn, 0}}, o1); }, "fused step, NTT-domain term");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(*r.hks[0], a, 0, 2, w0, {LincombTerm{&three, 0}}, o1); }, "fused step, 3-component term");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(*r.hks[0], a, 0, 2, w0, {LincombTerm{&a, 1}}, o1); }, "fused step, term range past the end");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(*r.hks[0], a, 1, 2, w0, {LincombTerm{&a, 0}}, o1); }, "fused step, operand range past the end");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(*r.hks[0], a, 0, 2, w0, {LincombTerm{&a, 0}}, o0); }, "fused step, output on the data context");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(*r.hks[1], a, 0, 2, w1, {LincombTerm{&a, 0}}, o1); }, "fused step, operands of another level");
    CHECK(many.terms() == 15);
    // a term one level UP is read in place; count 0 is a no-op
    Ciphertext o2(*r.ctx[2], 2, 2);
    HIP(hipMemset(z1.data(), 0, z1.words() * 8));
    HIP(hipMemset(a.data(), 0, a.words() * 8));
    step(*r.hks[1], z1, 0, 2, w1, {LincombTerm{&a, 0}}, o2);
    step(*r.hks[1], z1, 0, 0, w1, {LincombTerm{&a, 0}}, o2);
    r.ctx[0]->synchronize();
    const std::vector<uint64_t> zeros = words(o2);
    CHECK(std::all_of(zeros.begin(), zeros.end(), [](uint64_t x) { return x == 0; }));
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "ref") {
        uint64_t special = 0, special_psi = 0;
        const FheParams p = ring(kLog2N, kDataLimbs, special, special_psi);
        const double gs = ApproxInvSqrt::balanced_guess_scale(kVScale, p.moduli[kDataLimbs - 1], p.moduli[kDataLimbs - 2]);
        for (size_t K = 1; K <= kSteps; ++K) {
            const Case c(K);
            const double bound = ApproxInvSqrt::error_bound(kLog2N, p.moduli, std::vector<uint64_t>(2 * K, special), kVScale, gs, c.vmax, c.ymax,
                                                            fresh_noise_bound(kVScale, c.vmax), fresh_noise_bound(gs, c.y0max));
            std::printf("steps %zu: min|Y_K| = %.4f error_bound = 2^%.2f ratio = 2^%.2f guess_scale = 2^%.3f\n", K, c.ymin, std::log2(bound), std::log2(bound / c.ymin),
                        std::log2(gs));
        }
        return 0;
    }
    const double G = argc > 1 ? std::atof(argv[1]) : 0.040;
    try {
        Gate gate(G);
        if (!gate.ok()) { std::printf("no non-blocking stream\n"); return 2; }
        Rig r;
        for (size_t K = 1; K <= kSteps; ++K) run_invsqrt(r, K);
        run_multiply_lincomb(r, gate);
        invsqrt_behind_the_gate(r, gate);
        rejections(r);
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    return finish("inverse square root C++ facade OK");
}
