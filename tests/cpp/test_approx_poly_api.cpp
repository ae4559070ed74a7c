// GPU test of the approximate family's activations in the C++ facade (HybridKeySwitcher::multiply_rescale, ApproxPolynomial): on ENCRYPTED inputs every
// decoded slot of every token lies within the stated error bound of the float64 product / polynomial, the bound is at most 2^-10 of max|p(x)| >= 1 (a wrong
// power, scale, weight or level gives errors of order max|p|); both calls return while their stream is held (the gate of tests/cpp/facade_test.h)
// and give the same words there; the constructor's and apply()'s rejections.  Built and run by tests/test_gpu_approx_poly.py (-m gpu).
// `test_approx_poly_api ref` only draws the cases and prints max|p(x)| and ApproxPolynomial::error_bound of each (no device).  Exit code 0 = all passed.
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

static const unsigned kLog2N = 12;
static const size_t kDataLimbs = 5, kTokens = 3;
static const double kInputScale = std::ldexp(1.0, 59), kOutputScale = std::ldexp(1.0, 50), kX = 2.0;
static const size_t kDegrees[] = {2, 3, 4, 7};

static size_t ceil_log2(size_t k) { size_t r = 0; while (((size_t)1 << r) < k) ++r; return r; }

// one case: a_0 = 2 and sum_{k >= 1} |a_k| X^k <= 0.9, so 1.1 <= p(x) <= 2.9 on [-X, X]; the tokens' slots uniform on [-X, X]; the float64 p(x)
struct Case {
    size_t d;
    std::vector<double> a, x, y;   // x, y: [kTokens][N/2]
    double pmax = 0;
    explicit Case(size_t degree) : d(degree) {
        g_rng.state = 7000 + degree;
        const size_t row = ((size_t)1 << kLog2N) / 2;
        a.assign(d + 1, 2.0);
        for (size_t k = 1; k <= d; ++k) {
            const double mag = 0.75 + 0.25 * uni(), sign = uni() < 0 ? -1.0 : 1.0;
            a[k] = sign * mag * 0.9 / ((double)d * std::pow(kX, (double)k));
        }
        x.resize(kTokens * row); y.resize(kTokens * row);
        for (size_t i = 0; i < x.size(); ++i) {
            x[i] = kX * uni();
            double acc = 0;
            for (size_t k = d + 1; k-- > 0;) acc = acc * x[i] + a[k];
            y[i] = acc;
            pmax = std::max(pmax, std::fabs(acc));
        }
    }
};

static double fresh_noise_bound() { return 21.0 + 0.5 + 8.0 * kLog2N * std::ldexp(1.0, -53) * kInputScale * kX; }

struct Rig {
    uint64_t special = 0, special_psi = 0;
    std::vector<FheParams> params;
    std::vector<std::unique_ptr<Context>> ctx;                 // depth 0 .. 4
    std::unique_ptr<KeyGenerator> kg;
    std::vector<std::unique_ptr<SecretKey>> sk;
    std::vector<std::unique_ptr<HybridKeySwitcher>> hks;       // depth 0 .. 2
    std::unique_ptr<ComplexEncoder> cenc;
    std::unique_ptr<Encryptor> enc;
    Rig() {
        params.push_back(ring(kLog2N, kDataLimbs, special, special_psi));
        for (size_t r = 0; r + 1 < kDataLimbs; ++r) params.push_back(params.back().drop_last_limb());
        for (const FheParams& p : params) ctx.emplace_back(new Context(p, 0));
        kg.reset(new KeyGenerator(*ctx[0], TestSeed{11}));
        for (size_t r = 0; r < ctx.size(); ++r) sk.emplace_back(new SecretKey(*ctx[r], kg->secret_key().coefficients()));
        for (size_t r = 0; r < 3; ++r) hks.emplace_back(new HybridKeySwitcher(*ctx[r], *sk[r], special, special_psi, TestSeed{12 + r}));
        cenc.reset(new ComplexEncoder(*ctx[0]));
        enc.reset(new Encryptor(*ctx[0], kg->secret_key(), TestSeed{13}));
    }
    std::vector<HybridKeySwitcher*> levels(size_t count) const {
        std::vector<HybridKeySwitcher*> v;
        for (size_t r = 0; r < count; ++r) v.push_back(hks[r].get());
        return v;
    }
    void encrypt(const double* slots, size_t items, Ciphertext& out) const {   // real slots [items][N/2] at kInputScale
        const size_t N = params[0].n(), row = N / 2;
        std::vector<int64_t> msg(items * N);
        std::vector<cplx> z(row);
        for (size_t t = 0; t < items; ++t) {
            for (size_t i = 0; i < row; ++i) z[i] = cplx(slots[t * row + i], 0.0);
            cenc->encode(z.data(), kInputScale, &msg[t * N]);
        }
        enc->encrypt(msg.data(), 0, out);
    }
    std::vector<cplx> decrypt(const Ciphertext& ct, size_t depth, double scale) const {
        const size_t N = params[0].n(), row = N / 2;
        Decryptor dec(*ctx[depth], *sk[depth]);
        std::vector<int64_t> out(ct.batch() * N);
        dec.decrypt(ct, 0, out.data());
        std::vector<cplx> z(ct.batch() * row);
        for (size_t i = 0; i < ct.batch(); ++i) cenc->decode(&out[i * N], scale, &z[i * row]);
        return z;
    }
};

static void run_polynomial(Rig& r, size_t d) {
    const Case c(d);
    const size_t rstar = ceil_log2(d), row = r.params[0].n() / 2;
    ApproxPolynomial poly(r.levels(rstar), *r.ctx[rstar], *r.ctx[rstar + 1], c.a, kInputScale, kOutputScale);
    CHECK(poly.degree() == d && poly.depth() == rstar + 1 && poly.output_scale() == kOutputScale && poly.power_scale(1) == kInputScale);
    CHECK(poly.power_scale(2) == (kInputScale * kInputScale) / (double)r.params[0].moduli.back());
    Ciphertext x(*r.ctx[0], 2, kTokens), y(*r.ctx[rstar + 1], 2, kTokens);
    r.encrypt(c.x.data(), kTokens, x);
    poly.apply(x, y);
    r.ctx[0]->synchronize();
    CHECK(!y.is_ntt());
    const std::vector<cplx> z = r.decrypt(y, rstar + 1, kOutputScale);
    const double bound = poly.error_bound(kX, fresh_noise_bound());
    double worst = 0;
    for (size_t i = 0; i < kTokens * row; ++i) worst = std::max(worst, std::max(std::fabs(z[i].real() - c.y[i]), std::fabs(z[i].imag())));
    std::printf("degree %zu, %zu tokens, depth %zu: max|p(x)| %.3f, max error 2^%.2f, error_bound 2^%.2f (%zu slots)\n", d, kTokens, poly.depth(), c.pmax,
                std::log2(worst), std::log2(bound), kTokens * row);
    CHECK(c.pmax >= 1.0);
    CHECK(bound <= std::ldexp(1.0, -10) * c.pmax);
    CHECK(worst <= bound);
}

// a x b on encrypted inputs: the slot error of one product by the header's recurrence (D_2 with two different operands of modulus <= X), and the gate
static void run_multiply_rescale(Rig& r, Gate& gate) {
    const size_t N = r.params[0].n(), row = N / 2, T = 2;
    g_rng.state = 4242;
    std::vector<double> xa(T * row), xb(T * row);
    for (auto& v : xa) v = kX * uni();
    for (auto& v : xb) v = kX * uni();
    Ciphertext a(*r.ctx[0], 2, T), b(*r.ctx[0], 2, T), out(*r.ctx[1], 2, T), sq(*r.ctx[1], 2, T);
    r.encrypt(xa.data(), T, a);
    r.encrypt(xb.data(), T, b);
    r.hks[0]->multiply_rescale(a, b, out);
    r.hks[0]->multiply_rescale(a, a, sq);      // the same object twice: a square
    r.ctx[0]->synchronize();
    const double q = (double)r.params[0].moduli.back(), s2 = (kInputScale * kInputScale) / q, Nd = (double)N, H = (Nd + 1) / 2;
    uint64_t qmax = 0;
    for (uint64_t m : r.params[0].moduli) qmax = std::max(qmax, m);
    const double K = 21.0 * (double)kDataLimbs * Nd * ((double)qmax / (double)r.special), D1 = Nd * fresh_noise_bound();
    const double D2 = (2 * kInputScale * kX * D1 + D1 * D1 + Nd * (K + H)) / q + Nd * H + 4 * std::ldexp(1.0, -53) * s2 * kX * kX;
    const double pre = D2 / s2, bound = pre + 8.0 * kLog2N * std::ldexp(1.0, -53) * Nd * (kX * kX + pre);
    const std::vector<cplx> z = r.decrypt(out, 1, s2), zs = r.decrypt(sq, 1, s2);
    double worst = 0, big = 0;
    for (size_t i = 0; i < T * row; ++i) {
        worst = std::max(worst, std::max(std::fabs(z[i].real() - xa[i] * xb[i]), std::fabs(z[i].imag())));
        worst = std::max(worst, std::max(std::fabs(zs[i].real() - xa[i] * xa[i]), std::fabs(zs[i].imag())));
        big = std::max(big, std::fabs(xa[i] * xb[i]));
    }
    std::printf("multiply_rescale, %zu items: max|a b| %.3f, max error 2^%.2f, bound 2^%.2f\n", T, big, std::log2(worst), std::log2(bound));
    CHECK(big >= 1.0 && bound <= std::ldexp(1.0, -10) && worst <= bound);
    // ranges: items 1 of a and 0 of b into item 1 of a fresh output; the other item stays
    Ciphertext part(*r.ctx[1], 2, T);
    CHECK(hipMemset(part.data(), 0, part.words() * 8) == hipSuccess);
    r.hks[0]->multiply_rescale_range(a, 1, b, 0, 1, part, 1);
    r.ctx[0]->synchronize();
    const std::vector<cplx> zp = r.decrypt(part, 1, s2);
    double wp = 0;
    for (size_t i = 0; i < row; ++i) wp = std::max(wp, std::max(std::fabs(zp[row + i].real() - xa[row + i] * xb[i]), std::abs(zp[i])));
    CHECK(wp <= bound);

    // the gate, with the full protocol: zero words in both operand buffers during the warm-up and the gate, the operands copied in on S behind it, the
    // output wiped on S behind it; the call comes back with the event pending, within G / 4, and gives the words of the idle stream
    const std::vector<uint64_t> want = words(out);
    Ciphertext ga(*r.ctx[0], 2, T), gb(*r.ctx[0], 2, T), zero(*r.ctx[0], 2, T);
    HIP(hipMemset(zero.data(), 0, zero.words() * 8));
    const double t_enqueue = gate.gated("HybridKeySwitcher::multiply_rescale", {late(ga, zero, a), late(gb, zero, b)}, {out_of(out)},
                                        [&](Stream* s) { r.hks[0]->multiply_rescale(ga, gb, out, s); });
    CHECK(words(out) == want);
    std::printf("HybridKeySwitcher::multiply_rescale behind the gate: t_enqueue %.3f ms, G %.1f ms\n", t_enqueue * 1e3, gate.G * 1e3);
}

static void polynomial_behind_the_gate(Rig& r, Gate& gate) {
    const Case c(7);
    ApproxPolynomial poly(r.levels(3), *r.ctx[3], *r.ctx[4], c.a, kInputScale, kOutputScale);
    Ciphertext x(*r.ctx[0], 2, kTokens), real(*r.ctx[0], 2, kTokens), zero(*r.ctx[0], 2, kTokens), y(*r.ctx[4], 2, kTokens);
    r.encrypt(c.x.data(), kTokens, real);
    HIP(hipMemset(zero.data(), 0, zero.words() * 8));
    poly.apply(real, y);
    r.ctx[0]->synchronize();
    const std::vector<uint64_t> want = words(y);
    const double t_enqueue = gate.gated("ApproxPolynomial::apply", {late(x, zero, real)}, {out_of(y)}, [&](Stream* s) { poly.apply(x, y, s); });
    CHECK(words(y) == want);
    std::printf("ApproxPolynomial::apply behind the gate: t_enqueue %.3f ms, G %.1f ms\n", t_enqueue * 1e3, gate.G * 1e3);
}

static void rejections(Rig& r) {
    const Case c(4);
    auto build = [&](size_t n_levels, const Context& sum, const Context& out, const std::vector<double>& a, double xs, double ys) {
        ApproxPolynomial poly(r.levels(n_levels), sum, out, a, xs, ys);
    };
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(1, *r.ctx[1], *r.ctx[2], std::vector<double>{1.0, 1.0}, kInputScale, kOutputScale); }, "degree 1");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(3, *r.ctx[3], *r.ctx[4], std::vector<double>(17, 0.01), kInputScale, kOutputScale); }, "degree 16");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(1, *r.ctx[1], *r.ctx[2], c.a, kInputScale, kOutputScale); }, "one level for degree 4");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(3, *r.ctx[3], *r.ctx[4], c.a, kInputScale, kOutputScale); }, "three levels for degree 4");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(2, *r.ctx[1], *r.ctx[2], c.a, kInputScale, kOutputScale); }, "sum_ctx one level too high");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(2, *r.ctx[2], *r.ctx[2], c.a, kInputScale, kOutputScale); }, "out_ctx = sum_ctx");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(2, *r.ctx[2], *r.ctx[4], c.a, kInputScale, kOutputScale); }, "out_ctx two limbs below");
    {
        std::vector<HybridKeySwitcher*> swapped{r.hks[1].get(), r.hks[0].get()};
        expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ApproxPolynomial p(swapped, *r.ctx[2], *r.ctx[3], c.a, kInputScale, kOutputScale); }, "levels out of order");
    }
    std::vector<double> a = c.a;
    a[2] = 1e6;     // c_2 = 1e6 * 2^50 q* / s_2, about 2^72
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(2, *r.ctx[2], *r.ctx[3], a, kInputScale, kOutputScale); }, "|c_2| too large");
    a = c.a; a[0] = 8192.0;   // llround(a_0 S) = 2^63
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(2, *r.ctx[2], *r.ctx[3], a, kInputScale, kOutputScale); }, "constant too large");
    a = c.a; a[1] = std::nan("");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(2, *r.ctx[2], *r.ctx[3], a, kInputScale, kOutputScale); }, "NaN coefficient");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(2, *r.ctx[2], *r.ctx[3], c.a, 0.0, kOutputScale); }, "input_scale 0");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(2, *r.ctx[2], *r.ctx[3], c.a, kInputScale, INFINITY); }, "output_scale infinite");
    ApproxPolynomial poly(r.levels(2), *r.ctx[2], *r.ctx[3], c.a, kInputScale, kOutputScale);
    Ciphertext x(*r.ctx[0], 2, 2), same(*r.ctx[2], 2, 2), one(*r.ctx[3], 2, 1), lower(*r.ctx[1], 2, 2), y(*r.ctx[3], 2, 2);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { poly.apply(x, same); }, "apply, output on sum_ctx");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { poly.apply(x, one); }, "apply, output batch");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { poly.apply(lower, y); }, "apply, input one level down");
    // multiply_rescale: shapes and levels
    Ciphertext a0(*r.ctx[0], 2, 2), b1(*r.ctx[0], 2, 1), o0(*r.ctx[0], 2, 2), o1(*r.ctx[1], 2, 2), three(*r.ctx[0], 3, 2);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { r.hks[0]->multiply_rescale(a0, b1, o1); }, "multiply_rescale, batches differ");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { r.hks[0]->multiply_rescale(a0, a0, o0); }, "multiply_rescale, output on the data context");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { r.hks[0]->multiply_rescale(three, three, o1); }, "multiply_rescale, 3 components");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { r.hks[1]->multiply_rescale(a0, a0, o1); }, "multiply_rescale, operands of another level");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { r.hks[0]->multiply_rescale_range(a0, 1, a0, 0, 2, o1, 0); }, "multiply_rescale_range, range past the end");
    CHECK(&r.hks[1]->data_context() == r.ctx[1].get());
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "ref") {
        uint64_t special = 0, special_psi = 0;
        const FheParams p = ring(kLog2N, kDataLimbs, special, special_psi);
        for (size_t d : kDegrees) {
            const Case c(d);
            const double bound = ApproxPolynomial::error_bound(kLog2N, p.moduli, std::vector<uint64_t>(ceil_log2(d), special), c.a, kInputScale, kOutputScale, kX,
                                                               fresh_noise_bound());
            std::printf("degree %zu: max|p(x)| = %.4f error_bound = 2^%.2f ratio = 2^%.2f\n", d, c.pmax, std::log2(bound), std::log2(bound / c.pmax));
        }
        return 0;
    }
    const double G = argc > 1 ? std::atof(argv[1]) : 0.040;
    try {
        Gate gate(G);
        if (!gate.ok()) { std::printf("no non-blocking stream\n"); return 2; }
        Rig r;
        for (size_t d : kDegrees) run_polynomial(r, d);
        run_multiply_rescale(r, gate);
        polynomial_behind_the_gate(r, gate);
        rejections(r);
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    return finish("approximate polynomial C++ facade OK");
}
