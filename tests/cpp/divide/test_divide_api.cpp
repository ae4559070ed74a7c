// GPU test of the Goldschmidt step and the division in the C++ facade (ComplementConstant, HybridKeySwitcher::multiply_complement_rescale_range, ApproxDivide),
// on ENCRYPTED inputs on 60-bit fold primes with the special prime.  Built and run by tests/test_gpu_divide.py (-m gpu), one process per case.
//   test_divide_api run <log2 N> <K> [gate seconds]
//       G = 2 groups of T = 3 numerators, K steps: every decoded slot within error_bound of the float64 iteration F = 2 - D; n = n F; D = D F from the values
//       encrypted, the bound below the largest quotient, and every slot within error_bound + |n / D| |1 - D_0|^(2^K) of the true quotient;
//       one step word for word against Evaluator::negate, Evaluator::add_plain of the constant and multiply_rescale_range against the factor copied out per
//       item; the step and ApproxDivide::apply return while their stream is held (the gate of tests/cpp/facade_test.h) and give the words of the idle stream;
//       the rejections.
//   test_divide_api ref
//       no device: per case the chain, the drawn magnitudes and ApproxDivide::error_bound's static form, doubles by their bits, for tests/test_divide_model_cpu.py
//       to recompute; guess and residual; every INVALID_ARGUMENT condition of the scales.
// Exit code 0 = all passed.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#define FACADE_TEST_GATE
#include "../facade_test.h"

using namespace deeppowers::fhe;
using namespace facade_test;
typedef std::complex<double> cplx;

static SplitMix64 g_rng;   // every case sets its state

static const size_t kGroups = 2, kTerms = 3;
static const double kNumScale = std::ldexp(1.0, 50), kDLo = 0.6, kDHi = 1.4, kNumMax = 1.0;
static const double kU = std::ldexp(1.0, -53);

// one case: D_0 uniform on [kDLo, kDHi] (the denominator as read at den_scale: the constant guess folded in), numerators uniform on [-kNumMax, kNumMax]; the
// float64 iteration
struct Case {
    unsigned log2n;
    size_t K, row;
    std::vector<double> den, num, y, closed;   // [G][row], [G][T][row], the iteration's n_K, the residual |1 - D_0|^(2^K) per [G][row]
    double dmax = 0, xmax = 0, qmax = 0, d0max = 0, n0max = 0;
    Case(unsigned log2n_, size_t steps) : log2n(log2n_), K(steps), row(((size_t)1 << log2n_) / 2) {
        g_rng.state = 7000 + 16 * log2n + steps;
        den.resize(kGroups * row); num.resize(kGroups * kTerms * row); y.resize(num.size()); closed.resize(den.size());
        for (auto& v : den) v = kDLo + (kDHi - kDLo) * g_rng.unit();
        for (auto& v : num) v = kNumMax * g_rng.sym();
        for (size_t g = 0; g < kGroups; ++g)
            for (size_t i = 0; i < row; ++i) {
                double D = den[g * row + i], r = std::fabs(1.0 - D), n[kTerms];
                for (size_t j = 0; j < kTerms; ++j) n[j] = num[(g * kTerms + j) * row + i];
                d0max = std::max(d0max, D);
                dmax = std::max(dmax, std::fabs(D));
                for (size_t j = 0; j < kTerms; ++j) { xmax = std::max(xmax, std::fabs(n[j])); n0max = std::max(n0max, std::fabs(n[j])); qmax = std::max(qmax, std::fabs(n[j] / D)); }
                for (size_t s = 0; s < K; ++s) {
                    const double F = 2.0 - D;
                    for (size_t j = 0; j < kTerms; ++j) { n[j] = n[j] * F; xmax = std::max(xmax, std::fabs(n[j])); }
                    D = D * F;
                    dmax = std::max(dmax, std::fabs(D));
                    r = r * r;
                }
                for (size_t j = 0; j < kTerms; ++j) y[(g * kTerms + j) * row + i] = n[j];
                closed[g * row + i] = r;
            }
        dmax *= 1 + std::ldexp(1.0, -40);   // bounds on the real iterates too
        xmax *= 1 + std::ldexp(1.0, -40);
    }
};

static double fresh_noise_bound(unsigned log2n, double scale, double X) { return 21.0 + 0.5 + 8.0 * log2n * kU * scale * X; }

struct Rig {
    unsigned log2n;
    size_t K, limbs;
    uint64_t special = 0, special_psi = 0;
    std::vector<FheParams> params;
    std::vector<std::unique_ptr<Context>> ctx;                 // level 0 .. K
    std::unique_ptr<KeyGenerator> kg;
    std::vector<std::unique_ptr<SecretKey>> sk;
    std::vector<std::unique_ptr<HybridKeySwitcher>> hks;       // level 0 .. K - 1
    std::unique_ptr<ComplexEncoder> cenc;
    std::unique_ptr<Encryptor> enc;
    double den_scale = 0;
    Rig(unsigned log2n_, size_t steps) : log2n(log2n_), K(steps), limbs(steps + 2) {   // two limbs are left at the output
        params.push_back(ring(log2n, limbs, special, special_psi));
        for (size_t r = 0; r < K; ++r) params.push_back(params.back().drop_last_limb());
        for (const FheParams& p : params) ctx.emplace_back(new Context(p, 0));
        kg.reset(new KeyGenerator(*ctx[0], TestSeed{11}));
        for (size_t r = 0; r < ctx.size(); ++r) sk.emplace_back(new SecretKey(*ctx[r], kg->secret_key().coefficients()));
        for (size_t r = 0; r < K; ++r) hks.emplace_back(new HybridKeySwitcher(*ctx[r], *sk[r], special, special_psi, TestSeed{12 + r}));
        cenc.reset(new ComplexEncoder(*ctx[0]));
        enc.reset(new Encryptor(*ctx[0], kg->secret_key(), TestSeed{13}));
        den_scale = (double)params[0].moduli.back();   // at the primes, where sigma_n stays
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

static void run_divide(Rig& r, const Case& c) {
    const size_t K = r.K, row = c.row, G = kGroups, T = kTerms;
    ApproxDivide div(r.levels(K), *r.ctx[K], kNumScale, r.den_scale);
    CHECK(div.iterations() == K && div.depth() == K && div.den_scale(0) == r.den_scale && div.num_scale(0) == kNumScale);
    {   // the scale rule, in its double operations
        const double q0 = (double)r.params[0].moduli.back();
        CHECK(div.kappa(0) == std::llround(2.0 * r.den_scale) && div.den_scale(1) == (r.den_scale * r.den_scale) / q0 && div.num_scale(1) == (kNumScale * r.den_scale) / q0);
        CHECK(std::fabs(div.den_scale(K) / r.den_scale - 1) < std::ldexp(1.0, -16));   // at the primes it stays there
    }
    Ciphertext num(*r.ctx[0], 2, G * T), den(*r.ctx[0], 2, G), y(*r.ctx[K], 2, G * T);
    r.encrypt(c.num.data(), G * T, kNumScale, num);
    r.encrypt(c.den.data(), G, r.den_scale, den);
    div.apply(num, den, y);
    r.ctx[0]->synchronize();
    CHECK(!y.is_ntt());
    const std::vector<cplx> z = r.decrypt(y, K, div.num_scale(K));
    const double bound = div.error_bound(c.dmax, c.xmax, fresh_noise_bound(r.log2n, r.den_scale, c.d0max), fresh_noise_bound(r.log2n, kNumScale, c.n0max));
    double worst = 0, worst_true = 0, slack = 0, residual = 0;
    for (size_t g = 0; g < G; ++g)
        for (size_t j = 0; j < T; ++j)
            for (size_t i = 0; i < row; ++i) {
                const size_t at = (g * T + j) * row + i;
                const double quotient = c.num[at] / c.den[g * row + i], allowed = bound + std::fabs(quotient) * c.closed[g * row + i];
                worst = std::max(worst, std::max(std::fabs(z[at].real() - c.y[at]), std::fabs(z[at].imag())));
                const double off = std::fabs(z[at].real() - quotient);
                if (off > allowed) slack = std::max(slack, off - allowed);
                worst_true = std::max(worst_true, off);
                residual = std::max(residual, c.closed[g * row + i]);
            }
    std::printf("%zu Goldschmidt steps at N = %zu, %zu x %zu: max|n/D| %.3f, max error 2^%.2f, error_bound 2^%.2f (%zu slots); within 2^%.2f of the quotient, residual 2^%.2f\n", K,
                2 * row, G, T, c.qmax, std::log2(worst), std::log2(bound), G * T * row, std::log2(worst_true), std::log2(residual));
    CHECK(c.qmax >= 1.0);
    CHECK(bound < c.qmax);
    CHECK(worst <= bound);
    CHECK(slack == 0);
    CHECK(residual <= ApproxDivide::residual(kDLo, kDHi, K) * (1 + 1e-12));
}

// one step at level 0, word for word: negate, add_plain of kappa X^0, the factor copied out per item, multiply_rescale_range
static void run_step_words(Rig& r, const Case& c) {
    const size_t G = kGroups, T = kTerms, N = r.params[0].n(), Ld = r.params[0].n_limbs();
    Evaluator ev(*r.ctx[0]);
    Ciphertext num(*r.ctx[0], 2, G * T), den(*r.ctx[0], 2, G);
    r.encrypt(c.num.data(), G * T, kNumScale, num);
    r.encrypt(c.den.data(), G, r.den_scale, den);
    const int64_t kappa = std::llround(2.0 * r.den_scale);
    ComplementConstant kc(*r.ctx[0], kappa);
    CHECK(kc.value() == kappa && &kc.context() == r.ctx[0].get() && kc.data() != nullptr);
    Plaintext constant(*r.ctx[0], 1, false);
    {
        std::vector<uint64_t> host(Ld * N, 0);
        for (size_t l = 0; l < Ld; ++l) host[l * N] = (uint64_t)kappa % r.params[0].moduli[l];
        constant.copy_from_host(host.data());
    }
    Ciphertext factor(*r.ctx[0], 2, G), lhs(*r.ctx[0], 2, G * T + G), rhs(*r.ctx[0], 2, G * T + G), want(*r.ctx[1], 2, G * T + G), got(*r.ctx[1], 2, G * T + G);
    ev.negate(den, factor);
    factor.set_ntt(false);
    ev.add_plain(factor, constant, factor);
    r.ctx[0]->synchronize();
    const size_t item = 2 * Ld * N * 8;
    for (size_t g = 0; g < G; ++g) {
        for (size_t j = 0; j <= T; ++j) {   // j == T: the self product, after all numerators
            const size_t at = j < T ? g * T + j : G * T + g;
            HIP(hipMemcpy((char*)lhs.data() + at * item, j < T ? (const char*)num.data() + (g * T + j) * item : (const char*)den.data() + g * item, item, hipMemcpyDeviceToDevice));
            HIP(hipMemcpy((char*)rhs.data() + at * item, (const char*)factor.data() + g * item, item, hipMemcpyDeviceToDevice));
        }
    }
    r.hks[0]->multiply_rescale_range(lhs, 0, rhs, 0, G * T + G, want, 0);
    HIP(hipMemset(got.data(), 0xA5, got.words() * 8));
    r.hks[0]->multiply_complement_rescale_range(num, 0, den, 0, G, T, true, kc, got, 0);
    r.ctx[0]->synchronize();
    CHECK(!got.is_ntt() && words(got) == words(want));
    // without the self product: the numerators' words alone, the rest of the buffer untouched; ranges that do not start at 0
    Ciphertext part(*r.ctx[1], 2, G * T + G);
    HIP(hipMemset(part.data(), 0xA5, part.words() * 8));
    r.hks[0]->multiply_complement_rescale_range(num, T, den, 1, 1, T, false, kc, part, 1);
    r.ctx[0]->synchronize();
    const std::vector<uint64_t> w = words(want), p = words(part);
    const size_t out_item = w.size() / (G * T + G);
    CHECK(std::equal(p.begin() + out_item, p.begin() + (1 + T) * out_item, w.begin() + T * out_item));
    CHECK(std::all_of(p.begin(), p.begin() + out_item, [](uint64_t x) { return x == 0xA5A5A5A5A5A5A5A5ull; }) &&
          std::all_of(p.begin() + (1 + T) * out_item, p.end(), [](uint64_t x) { return x == 0xA5A5A5A5A5A5A5A5ull; }));
    // the denominators alone
    HIP(hipMemset(part.data(), 0xA5, part.words() * 8));
    r.hks[0]->multiply_complement_rescale_range(num, 0, den, 0, G, 0, true, kc, part, 0);
    r.ctx[0]->synchronize();
    const std::vector<uint64_t> d = words(part);
    CHECK(std::equal(d.begin(), d.begin() + G * out_item, w.begin() + G * T * out_item));
    std::printf("multiply_complement_rescale_range, %zu x %zu with self: the words of negate, add_plain and multiply_rescale_range\n", G, T);
}

static void behind_the_gate(Rig& r, const Case& c, Gate& gate) {
    const size_t G = kGroups, T = kTerms, K = r.K;
    ApproxDivide div(r.levels(K), *r.ctx[K], kNumScale, r.den_scale);
    ComplementConstant kc(*r.ctx[0], div.kappa(0));
    Ciphertext rn(*r.ctx[0], 2, G * T), rd(*r.ctx[0], 2, G), n(*r.ctx[0], 2, G * T), d(*r.ctx[0], 2, G), zn(*r.ctx[0], 2, G * T), zd(*r.ctx[0], 2, G), y(*r.ctx[K], 2, G * T),
        step(*r.ctx[1], 2, G * T + G);
    r.encrypt(c.num.data(), G * T, kNumScale, rn);
    r.encrypt(c.den.data(), G, r.den_scale, rd);
    HIP(hipMemset(zn.data(), 0, zn.words() * 8));
    HIP(hipMemset(zd.data(), 0, zd.words() * 8));
    struct Form { const char* what; PolyBuffer* out; std::function<void(Stream*)> idle, held; };
    const Form forms[] = {
        {"HybridKeySwitcher::multiply_complement_rescale_range", &step, [&](Stream* s) { r.hks[0]->multiply_complement_rescale_range(rn, 0, rd, 0, G, T, true, kc, step, 0, s); },
         [&](Stream* s) { r.hks[0]->multiply_complement_rescale_range(n, 0, d, 0, G, T, true, kc, step, 0, s); }},
        {"ApproxDivide::apply", &y, [&](Stream* s) { div.apply(rn, rd, y, s); }, [&](Stream* s) { div.apply(n, d, y, s); }},
    };
    for (const Form& f : forms) {
        f.idle(nullptr);
        r.ctx[0]->synchronize();
        const std::vector<uint64_t> want = words(*f.out);
        const double t_enqueue = gate.gated(f.what, {late(n, zn, rn), late(d, zd, rd)}, {out_of(*f.out)}, f.held);
        CHECK(words(*f.out) == want);
        std::printf("%s behind the gate: t_enqueue %.3f ms, G %.1f ms\n", f.what, t_enqueue * 1e3, gate.G * 1e3);
    }
    CHECK(gate.gated_calls == 2);
}

static void rejections(Rig& r) {
    const size_t K = r.K;
    auto build = [&](const std::vector<HybridKeySwitcher*>& lv, const Context& out, double ns, double ds) { ApproxDivide div(lv, out, ns, ds); };
    const double ds = r.den_scale;
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build({}, *r.ctx[0], kNumScale, ds); }, "no levels");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.levels(2), *r.ctx[1], kNumScale, ds); }, "out_ctx one level too high");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.levels(2), *r.ctx[3], kNumScale, ds); }, "out_ctx one level too low");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build({r.hks[1].get(), r.hks[0].get()}, *r.ctx[2], kNumScale, ds); }, "levels out of order");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build({r.hks[0].get(), nullptr}, *r.ctx[2], kNumScale, ds); }, "null level");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.levels(2), *r.ctx[2], 0.0, ds); }, "num_scale 0");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.levels(2), *r.ctx[2], kNumScale, INFINITY); }, "den_scale infinite");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.levels(2), *r.ctx[2], kNumScale, std::ldexp(1.0, 61)); }, "kappa_0 = 2^62");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.levels(2), *r.ctx[2], std::ldexp(1.0, 19), ds); }, "nu_0 below 2^20");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(r.levels(K), *r.ctx[K], kNumScale, ds / 64); }, "a den_scale 1/64 of the primes: sigma_2 = 2^-24 of them, nu_3 below 2^20");
    ApproxDivide div(r.levels(2), *r.ctx[2], kNumScale, ds);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)div.den_scale(3); }, "den_scale(3) of two steps");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)div.num_scale(3); }, "num_scale(3) of two steps");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)div.kappa(2); }, "kappa(2) of two steps");
    Ciphertext n(*r.ctx[0], 2, 6), d(*r.ctx[0], 2, 2), y(*r.ctx[2], 2, 6), few(*r.ctx[2], 2, 5), high(*r.ctx[1], 2, 6), five(*r.ctx[0], 2, 5), three(*r.ctx[0], 3, 2);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { div.apply(n, d, high); }, "apply, output one level too high");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { div.apply(n, d, few); }, "apply, output batch");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { div.apply(five, d, few); }, "apply, 5 numerators for 2 groups");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { div.apply(n, three, y); }, "apply, 3 components");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { div.apply(n, high, y); }, "apply, denominators one level down");
    // the holder and the step
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ComplementConstant k(*r.ctx[0], -1); }, "ComplementConstant, negative");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ComplementConstant k(*r.ctx[0], (int64_t)1 << 62); }, "ComplementConstant, 2^62");
    ComplementConstant k0(*r.ctx[0], 5), k1(*r.ctx[1], 5);
    Ciphertext o1(*r.ctx[1], 2, 8), o0(*r.ctx[0], 2, 8);
    auto step = [&](const Ciphertext& a, size_t a_first, const Ciphertext& b, size_t G, size_t T, bool self, const ComplementConstant& k, Ciphertext& out, size_t out_first) {
        r.hks[0]->multiply_complement_rescale_range(a, a_first, b, 0, G, T, self, k, out, out_first);
    };
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(n, 0, d, 2, 0, false, k0, o1, 0); }, "step, nothing to compute");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(n, 1, d, 2, 3, true, k0, o1, 0); }, "step, numerator range past the end");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(n, 0, d, 3, 2, true, k0, o1, 0); }, "step, more groups than denominators");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(n, 0, d, 2, 3, true, k0, o1, 1); }, "step, output range past the end");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(n, 0, d, 2, 3, true, k0, o0, 0); }, "step, output on the data context");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(n, 0, d, 2, 3, true, k1, o1, 0); }, "step, kappa of another level");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(n, 0, three, 2, 3, true, k0, o1, 0); }, "step, 3-component denominators");
    step(n, 0, d, 0, 3, true, k0, o1, 0);   // no groups: a no-op
}

static int run_ref() {
    const std::pair<unsigned, size_t> cases[] = {{12, 3}, {13, 4}};
    for (const auto& lk : cases) {
        const unsigned log2n = lk.first;
        const size_t K = lk.second;
        uint64_t special = 0, special_psi = 0;
        const FheParams p = ring(log2n, K + 2, special, special_psi);
        const Case c(log2n, K);
        const double ds = (double)p.moduli.back(), Bd = fresh_noise_bound(log2n, ds, c.d0max), Bn = fresh_noise_bound(log2n, kNumScale, c.n0max);
        const double bound = ApproxDivide::error_bound(log2n, p.moduli, std::vector<uint64_t>(K, special), kNumScale, ds, c.dmax, c.xmax, Bd, Bn);
        std::printf("case log2n %u K %zu special %llu moduli", log2n, K, (unsigned long long)special);
        for (uint64_t q : p.moduli) std::printf(" %llu", (unsigned long long)q);
        std::printf(" args %a %a %a %a %a %a bound %a\n", kNumScale, ds, c.dmax, c.xmax, Bd, Bn, bound);
        std::printf("steps %zu: max|n/D| = %.4f error_bound = 2^%.2f residual = 2^%.2f\n", K, c.qmax, std::log2(bound), std::log2(ApproxDivide::residual(kDLo, kDHi, K)));
        CHECK(c.qmax >= 1.0 && bound < c.qmax);
        // the bound grows with every argument
        CHECK(ApproxDivide::error_bound(log2n, p.moduli, std::vector<uint64_t>(K, special), kNumScale, ds, c.dmax, c.xmax, 2 * Bd, Bn) > bound);
        CHECK(ApproxDivide::error_bound(log2n, p.moduli, std::vector<uint64_t>(K, special), kNumScale, ds, c.dmax, 2 * c.xmax, Bd, Bn) > bound);
    }
    CHECK(ApproxDivide::guess(0.5, 1.5) == 1.0 && ApproxDivide::guess(1.0, 3.0) == 0.5);
    CHECK(ApproxDivide::residual(1.0, 3.0, 0) == 0.5 && ApproxDivide::residual(1.0, 3.0, 2) == 0.0625 && ApproxDivide::residual(2.0, 2.0, 3) == 0.0);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)ApproxDivide::guess(0.0, 1.0); }, "guess: lo = 0");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)ApproxDivide::residual(2.0, 1.0, 1); }, "residual: hi < lo");
    // the constructor's conditions on the scales, through the static bound (the same rule, no device)
    uint64_t special = 0, special_psi = 0;
    const FheParams p = ring(12, 5, special, special_psi);
    const double q = (double)p.moduli.back(), ns = kNumScale;
    auto bound = [&](size_t K, double num_scale, double den_scale) { return ApproxDivide::error_bound(12, p.moduli, std::vector<uint64_t>(K, special), num_scale, den_scale, 1, 1, 1, 1); };
    CHECK(bound(3, ns, q) > 0);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)bound(0, ns, q); }, "scales: no steps");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)bound(5, ns, q); }, "scales: more steps than limbs to drop");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)bound(3, 0.0, q); }, "scales: num_scale 0");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)bound(3, -ns, q); }, "scales: num_scale negative");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)bound(3, ns, NAN); }, "scales: den_scale NaN");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)bound(3, INFINITY, q); }, "scales: num_scale infinite");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)bound(1, ns, std::ldexp(1.0, 61)); }, "scales: kappa_0 = 2^62");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)bound(1, ns, std::ldexp(1.0, 62)); }, "scales: sigma_0 = 2^62");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)bound(1, std::ldexp(1.0, 19), q); }, "scales: nu_0 below 2^20");
    CHECK(bound(1, ns, 1.5 * q) > 0);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)bound(2, ns, 1.5 * q); }, "scales: kappa_1 = 4.5 q reaches 2^62");
    CHECK(bound(2, ns, q / 64) > 0);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)bound(3, ns, q / 64); }, "scales: sigma_3 = 2^-48 q is below 2^20");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)ApproxDivide::error_bound(12, p.moduli, std::vector<uint64_t>(3, special), ns, q, -1, 1, 1, 1); }, "error_bound: negative magnitude");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)ApproxDivide::error_bound(12, p.moduli, std::vector<uint64_t>(3, special), ns, q, 2.5, 1, 1, 1); }, "error_bound: a denominator above 2");
    return finish("division reference OK");
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "ref") return run_ref();
    if (mode != "run" || argc < 4) { std::printf("usage: test_divide_api run <log2 N> <K> [gate seconds] | ref\n"); return 2; }
    const unsigned log2n = (unsigned)std::atoi(argv[2]);
    const size_t K = (size_t)std::atoi(argv[3]);
    if (log2n < 10 || log2n > 13 || K < 3 || K > 6) { std::printf("usage: log2 N in [10, 13], K in [3, 6]\n"); return 2; }
    try {
        Gate gate(argc > 4 ? std::atof(argv[4]) : 0.040);
        if (!gate.ok()) { std::printf("no non-blocking stream\n"); return 2; }
        Rig r(log2n, K);
        const Case c(log2n, K);
        run_divide(r, c);
        run_step_words(r, c);
        behind_the_gate(r, c, gate);
        rejections(r);
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    return finish("division C++ facade OK");
}
