// GPU test of the sums of products in the C++ facade (Evaluator::multiply_sum, HybridKeySwitcher::multiply_sum_rescale_range and
// multiply_sum_lincomb_rescale_range, ApproxProductSum), on ENCRYPTED inputs at N = 4096 on four data limbs.  Built and run by tests/test_gpu_product_sum.py.
//   product_sum_words words   terms in {1, 3, 8} x groups in {1, 2}, the second operand per group and shared, word for word:
//                             - multiply_sum_rescale_range against the facade's own Evaluator::multiply per pair, Evaluator::add over the pairs on 3 components,
//                               HybridKeySwitcher::relinearize and Evaluator::rescale; Evaluator::multiply_sum against the same 3-component sum;
//                             - multiply_sum_lincomb_rescale_range against that sum relinearised and fed, with the addend, to dpfhe_lincomb_rescale under the same
//                               weights (include/dpfhe.h: the identity dpfhe_relinearize_lincomb_rescale_hybrid is stated by);
//                             - the calls' rejections.
//   product_sum_words bound   ApproxProductSum, terms = 8, shared second operand, 3 groups: every decoded slot within error_bound of the float64 sum, and the
//                             bound at most 2^-10 of max|y| >= 1 (a bound above the signal proves nothing).
//   product_sum_words gate    the two range methods and ApproxProductSum::apply return while their stream is held (the gate of tests/cpp/facade_test.h: zero
//                             inputs during the warm-up and the gate, the real ones copied in behind it) and give the words of the idle stream.
//   product_sum_words ref     no device: the case of `bound` drawn, the bound's arithmetic recomputed term by term from the header's text and compared.
// Exit code 0 = all passed.
#include <hip/hip_runtime_api.h>

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
#include "dpfhe.h"

using namespace deeppowers::fhe;
using namespace facade_test;
typedef std::complex<double> cplx;

static SplitMix64 g_rng;

static const unsigned kLog2N = 12;
static const size_t kDataLimbs = 4;
static const double kU = std::ldexp(1.0, -53);
static const double kScaleA = std::ldexp(1.0, 59), kScaleB = std::ldexp(1.0, 59);
static const size_t kBoundTerms = 8, kBoundGroups = 3;
static const double kMaxA = 1.0, kMaxB = 2.0;

static double fresh_noise_bound(double scale, double X) { return 21.0 + 0.5 + 8.0 * kLog2N * kU * scale * X; }

// the case of `bound`: weights a uniform on [0, kMaxA] (attention weights are not negative), values b on [-kMaxB, kMaxB]; y_g = sum_k a_{g,k} b_k in float64
struct BoundCase {
    std::vector<double> a, b, y;   // [G * K][row], [K][row], [G][row]
    double ymax = 0;
    explicit BoundCase(size_t row) : a(kBoundGroups * kBoundTerms * row), b(kBoundTerms * row), y(kBoundGroups * row, 0.0) {
        g_rng.state = 19019;
        for (auto& v : a) v = kMaxA * g_rng.unit();
        for (auto& v : b) v = kMaxB * g_rng.sym();
        for (size_t g = 0; g < kBoundGroups; ++g)
            for (size_t i = 0; i < row; ++i) {
                double s = 0;
                for (size_t k = 0; k < kBoundTerms; ++k) s += a[(g * kBoundTerms + k) * row + i] * b[k * row + i];
                y[g * row + i] = s;
                ymax = std::max(ymax, std::fabs(s));
            }
    }
};

// ApproxProductSum::error_bound from the header's text, term by term
static double bound_by_hand(const FheParams& p, uint64_t special, size_t terms, double A, double B, double Ba, double Bb) {
    const double N = (double)p.n(), H = (N + 1) / 2, K = (double)terms, q = (double)p.moduli.back();
    uint64_t qmax = 0;
    for (uint64_t m : p.moduli) qmax = std::max(qmax, m);
    const double Kr = 21.0 * (double)p.n_limbs() * N * ((double)qmax / (double)special);
    const double S = (kScaleA * kScaleB) / q, Da = N * Ba, Db = N * Bb;
    const double product_noise = K * (kScaleA * A * Db + kScaleB * B * Da + Da * Db);
    const double key_switch = N * (Kr + H), rescale = N * H, scale_rounding = 4 * kU * S * K * A * B;
    const double E = (product_noise + key_switch) / q + rescale + scale_rounding, pre = E / S;
    return pre + 8.0 * kLog2N * kU * N * (K * A * B + pre) + 2 * K * kU * K * A * B;
}

static int run_ref() {
    uint64_t special = 0, special_psi = 0;
    const FheParams p = ring(kLog2N, kDataLimbs, special, special_psi);
    const BoundCase c(p.n() / 2);
    const double Ba = fresh_noise_bound(kScaleA, kMaxA), Bb = fresh_noise_bound(kScaleB, kMaxB);
    const double bound = ApproxProductSum::error_bound(kLog2N, p.moduli, special, kBoundTerms, kScaleA, kScaleB, kMaxA, kMaxB, Ba, Bb);
    const double hand = bound_by_hand(p, special, kBoundTerms, kMaxA, kMaxB, Ba, Bb);
    std::printf("terms %zu groups %zu: max|y| %.4f, error_bound 2^%.2f, by hand 2^%.2f\n", kBoundTerms, kBoundGroups, c.ymax, std::log2(bound), std::log2(hand));
    CHECK(std::fabs(bound / hand - 1) < 1e-12);
    CHECK(c.ymax >= 1.0 && bound <= std::ldexp(1.0, -10) * c.ymax);
    // the bound grows with every argument, and one key switch is paid once: K terms cost less than K times one term
    const double one = ApproxProductSum::error_bound(kLog2N, p.moduli, special, 1, kScaleA, kScaleB, kMaxA, kMaxB, Ba, Bb);
    CHECK(one < bound && bound < (double)kBoundTerms * one);
    CHECK(ApproxProductSum::error_bound(kLog2N, p.moduli, special, kBoundTerms, kScaleA, kScaleB, kMaxA, kMaxB, 2 * Ba, Bb) > bound);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ApproxProductSum::error_bound(kLog2N, p.moduli, special, 0, kScaleA, kScaleB, 1, 1, 1, 1); }, "error_bound: no terms");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ApproxProductSum::error_bound(kLog2N, {p.moduli[0]}, special, 2, kScaleA, kScaleB, 1, 1, 1, 1); }, "error_bound: one limb");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ApproxProductSum::error_bound(kLog2N, p.moduli, special, 2, kScaleA, kScaleB, -1, 1, 1, 1); }, "error_bound: negative");
    return finish("product sum reference OK");
}

struct Rig {
    uint64_t special = 0, special_psi = 0;
    FheParams p0, p1;
    std::unique_ptr<Context> ctx0, ctx1;
    std::unique_ptr<KeyGenerator> kg;
    std::unique_ptr<SecretKey> sk1;
    std::unique_ptr<HybridKeySwitcher> hks;
    std::unique_ptr<ComplexEncoder> cenc;
    std::unique_ptr<Encryptor> enc;
    Rig() {
        p0 = ring(kLog2N, kDataLimbs, special, special_psi);
        p1 = p0.drop_last_limb();
        ctx0.reset(new Context(p0, 0));
        ctx1.reset(new Context(p1, 0));
        kg.reset(new KeyGenerator(*ctx0, TestSeed{21}));
        sk1.reset(new SecretKey(*ctx1, kg->secret_key().coefficients()));
        hks.reset(new HybridKeySwitcher(*ctx0, kg->secret_key(), special, special_psi, TestSeed{22}));
        cenc.reset(new ComplexEncoder(*ctx0));
        enc.reset(new Encryptor(*ctx0, kg->secret_key(), TestSeed{23}));
    }
    void encrypt(const double* slots, size_t items, double scale, Ciphertext& out) const {   // real slots [items][N/2]
        const size_t N = p0.n(), row = N / 2;
        std::vector<int64_t> msg(items * N);
        std::vector<cplx> z(row);
        for (size_t t = 0; t < items; ++t) {
            for (size_t i = 0; i < row; ++i) z[i] = cplx(slots[t * row + i], 0.0);
            cenc->encode(z.data(), scale, &msg[t * N]);
        }
        enc->encrypt(msg.data(), 0, out);
    }
    void encrypt_random(size_t items, double X, Ciphertext& out) const {
        std::vector<double> v(items * p0.n() / 2);
        for (auto& x : v) x = X * g_rng.sym();
        encrypt(v.data(), items, kScaleA, out);
    }
};

// item `index` of src -> the one item of dst (same context, same components)
static void take_item(const Ciphertext& src, size_t index, Ciphertext& dst) {
    HIP(hipMemcpy(dst.data(), src.data() + index * dst.words(), dst.words() * 8, hipMemcpyDeviceToDevice));
    dst.set_ntt(src.is_ntt());
}

static void run_words(Rig& r) {
    const size_t N = r.p0.n(), Ld = kDataLimbs;
    Evaluator ev(*r.ctx0);
    g_rng.state = 515;
    const size_t Gm = 2, Km = 8;
    Ciphertext a(*r.ctx0, 2, Gm * Km), b(*r.ctx0, 2, Gm * Km), z(*r.ctx0, 2, Gm);
    r.encrypt_random(Gm * Km, 1.5, a);
    r.encrypt_random(Gm * Km, 1.5, b);
    r.encrypt_random(Gm, 1.5, z);
    ScalarWeights weights(*r.ctx0, 3, {-5}, 7);
    for (size_t K : {(size_t)1, (size_t)3, (size_t)8})
        for (size_t G : {(size_t)1, (size_t)2})
            for (int shared = 0; shared < 2; ++shared) {
                // operands of this case: the first G * K items of a; of b the first G * K, or - shared - items 2 .. 2 + K (a range that does not start at 0)
                const size_t b_first = shared ? 2 : 0;
                if (b_first + K > Gm * Km) continue;
                // reference: every pair's product, the sums over each group's pairs on 3 components
                Ciphertext pa(*r.ctx0, 2, 1), pb(*r.ctx0, 2, 1), prod(*r.ctx0, 3, 1), sums(*r.ctx0, 3, G), acc(*r.ctx0, 3, 1);
                for (size_t g = 0; g < G; ++g) {
                    for (size_t k = 0; k < K; ++k) {
                        take_item(a, g * K + k, pa);
                        take_item(b, shared ? b_first + k : g * K + k, pb);
                        if (k == 0) ev.multiply(pa, pb, acc);
                        else { ev.multiply(pa, pb, prod); ev.add(acc, prod, acc); }
                    }
                    r.ctx0->synchronize();
                    HIP(hipMemcpy(sums.data() + g * acc.words(), acc.data(), acc.words() * 8, hipMemcpyDeviceToDevice));
                }
                Ciphertext rel(*r.ctx0, 2, G), want(*r.ctx1, 2, G), got(*r.ctx1, 2, G);
                r.hks->relinearize(sums, rel);
                ev.rescale(rel, want);
                // the 3-component sum itself
                {
                    Ciphertext pa_all(*r.ctx0, 2, G * K), pb_all(*r.ctx0, 2, shared ? K : G * K), sum3(*r.ctx0, 3, G);
                    HIP(hipMemcpy(pa_all.data(), a.data(), pa_all.words() * 8, hipMemcpyDeviceToDevice));
                    HIP(hipMemcpy(pb_all.data(), b.data() + b_first * (2 * Ld * N), pb_all.words() * 8, hipMemcpyDeviceToDevice));
                    ev.multiply_sum(pa_all, pb_all, K, shared != 0, sum3);
                    r.ctx0->synchronize();
                    CHECK(!sum3.is_ntt() && words(sum3) == words(sums));
                }
                HIP(hipMemset(got.data(), 0xA5, got.words() * 8));
                r.hks->multiply_sum_rescale_range(a, 0, b, b_first, shared != 0, G, K, got, 0);
                r.ctx0->synchronize();
                const bool same = !got.is_ntt() && words(got) == words(want);
                if (!same) std::printf("FAIL multiply_sum_rescale_range terms %zu groups %zu shared %d: words differ\n", K, G, shared);
                CHECK(same);
                // the lincomb form: w_0 t + w_1 z + constant, rescaled - t = the relinearised sum, through dpfhe_lincomb_rescale on [t | z]
                Ciphertext x(*r.ctx0, 2, 2 * G), lwant(*r.ctx1, 2, G), lgot(*r.ctx1, 2, G);
                HIP(hipMemcpy(x.data(), rel.data(), rel.words() * 8, hipMemcpyDeviceToDevice));
                HIP(hipMemcpy(x.data() + rel.words(), z.data(), rel.words() * 8, hipMemcpyDeviceToDevice));
                CHECK(dpfhe_lincomb_rescale(static_cast<dpfhe_ctx*>(r.ctx0->handle()), lwant.data(), x.data(), weights.data(), 2, G, nullptr) == 0);
                HIP(hipMemset(lgot.data(), 0xA5, lgot.words() * 8));
                r.hks->multiply_sum_lincomb_rescale_range(a, 0, b, b_first, shared != 0, G, K, weights, {LincombTerm{&z, 0}}, lgot, 0);
                r.ctx0->synchronize();
                const bool lsame = !lgot.is_ntt() && words(lgot) == words(lwant);
                if (!lsame) std::printf("FAIL multiply_sum_lincomb_rescale_range terms %zu groups %zu shared %d: words differ\n", K, G, shared);
                CHECK(lsame);
                CHECK(words(lgot) != words(got));   // (the addend and the weights did something)
            }
    // with one term it is multiply_rescale, word for word
    {
        Ciphertext one(*r.ctx1, 2, 2), mr(*r.ctx1, 2, 2);
        r.hks->multiply_sum_rescale_range(a, 0, b, 0, false, 2, 1, one, 0);
        r.hks->multiply_rescale_range(a, 0, b, 0, 2, mr, 0);
        r.ctx0->synchronize();
        CHECK(words(one) == words(mr));
    }
    // rejections
    Ciphertext out(*r.ctx1, 2, 2), wrong_level(*r.ctx0, 2, 2), three(*r.ctx0, 3, 2);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { r.hks->multiply_sum_rescale_range(a, 0, b, 0, false, 2, 0, out, 0); }, "no terms");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { r.hks->multiply_sum_rescale_range(a, 1, b, 0, false, 2, 8, out, 0); }, "a range past the end");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { r.hks->multiply_sum_rescale_range(a, 0, z, 0, true, 2, 3, out, 0); }, "shared b shorter than terms");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { r.hks->multiply_sum_rescale_range(a, 0, b, 0, false, 3, 1, out, 0); }, "more groups than output items");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { r.hks->multiply_sum_rescale_range(a, 0, b, 0, false, 2, 2, wrong_level, 0); }, "output on the operands' level");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { r.hks->multiply_sum_rescale_range(three, 0, b, 0, false, 1, 1, out, 0); }, "3-component operand");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { r.hks->multiply_sum_lincomb_rescale_range(a, 0, b, 0, false, 2, 2, weights, {}, out, 0); }, "weights without their addend");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { r.hks->multiply_sum_lincomb_rescale_range(a, 0, b, 0, false, 2, 2, weights, {LincombTerm{&z, 1}}, out, 0); },
                 "addend range past the end");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ev.multiply_sum(a, b, 3, false, three); }, "16 items are no multiple of 3");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ev.multiply_sum(a, b, 8, true, three); }, "shared b must hold `terms` items");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ApproxProductSum(*r.hks, 0, false, kScaleA, kScaleB); }, "ApproxProductSum: no terms");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ApproxProductSum(*r.hks, 2, false, 0.0, kScaleB); }, "ApproxProductSum: zero scale");
}

static void run_bound(Rig& r) {
    const size_t N = r.p0.n(), row = N / 2, K = kBoundTerms, G = kBoundGroups;
    const BoundCase c(row);
    ApproxProductSum mix(*r.hks, K, true, kScaleA, kScaleB);
    CHECK(mix.terms() == K && mix.b_shared());
    CHECK(mix.output_scale() == (kScaleA * kScaleB) / (double)r.p0.moduli.back());
    Ciphertext a(*r.ctx0, 2, G * K), b(*r.ctx0, 2, K), y(*r.ctx1, 2, G);
    r.encrypt(c.a.data(), G * K, kScaleA, a);
    r.encrypt(c.b.data(), K, kScaleB, b);
    mix.apply(a, b, y);
    r.ctx0->synchronize();
    CHECK(!y.is_ntt());
    Decryptor dec(*r.ctx1, *r.sk1);
    std::vector<int64_t> msg(G * N);
    dec.decrypt(y, 0, msg.data());
    std::vector<cplx> zz(row);
    const double bound = mix.error_bound(kMaxA, kMaxB, fresh_noise_bound(kScaleA, kMaxA), fresh_noise_bound(kScaleB, kMaxB));
    double worst = 0;
    for (size_t g = 0; g < G; ++g) {
        r.cenc->decode(&msg[g * N], mix.output_scale(), zz.data());
        for (size_t i = 0; i < row; ++i) worst = std::max(worst, std::max(std::fabs(zz[i].real() - c.y[g * row + i]), std::fabs(zz[i].imag())));
    }
    std::printf("ApproxProductSum, %zu terms, shared b, %zu groups: max|y| %.4f, max error 2^%.2f, error_bound 2^%.2f (%zu slots)\n", K, G, c.ymax, std::log2(worst),
                std::log2(bound), G * row);
    CHECK(c.ymax >= 1.0);
    CHECK(bound <= std::ldexp(1.0, -10) * c.ymax);
    CHECK(worst <= bound);
    Ciphertext few(*r.ctx0, 2, G * K - 1);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { mix.apply(few, b, y); }, "apply: a does not hold G * terms items");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { mix.apply(a, a, y); }, "apply: shared b holds `terms` items");
}

// the stream contract of multiply_rescale_range: enqueue only once the scratch has its size (the warm-up of the protocol grows it, the stream's arena included)
static void run_gate(Rig& r, Gate& gate) {
    const size_t G = 2, K = 3;
    g_rng.state = 626;
    Ciphertext ra(*r.ctx0, 2, G * K), rb(*r.ctx0, 2, K), rz(*r.ctx0, 2, G), a(*r.ctx0, 2, G * K), b(*r.ctx0, 2, K), z(*r.ctx0, 2, G), zero(*r.ctx0, 2, G * K),
        out(*r.ctx1, 2, G);
    r.encrypt_random(G * K, 1.5, ra);
    r.encrypt_random(K, 1.5, rb);
    r.encrypt_random(G, 1.5, rz);
    HIP(hipMemset(zero.data(), 0, zero.words() * 8));
    ScalarWeights weights(*r.ctx0, 3, {-5}, 7);
    ApproxProductSum mix(*r.hks, K, true, kScaleA, kScaleB);
    struct Form { const char* what; std::function<void(Stream*)> idle, held; };
    const Form forms[] = {
        {"HybridKeySwitcher::multiply_sum_rescale_range", [&](Stream* s) { r.hks->multiply_sum_rescale_range(ra, 0, rb, 0, true, G, K, out, 0, s); },
         [&](Stream* s) { r.hks->multiply_sum_rescale_range(a, 0, b, 0, true, G, K, out, 0, s); }},
        {"HybridKeySwitcher::multiply_sum_lincomb_rescale_range",
         [&](Stream* s) { r.hks->multiply_sum_lincomb_rescale_range(ra, 0, rb, 0, true, G, K, weights, {LincombTerm{&rz, 0}}, out, 0, s); },
         [&](Stream* s) { r.hks->multiply_sum_lincomb_rescale_range(a, 0, b, 0, true, G, K, weights, {LincombTerm{&z, 0}}, out, 0, s); }},
        {"ApproxProductSum::apply", [&](Stream* s) { mix.apply(ra, rb, out, s); }, [&](Stream* s) { mix.apply(a, b, out, s); }},
    };
    for (const Form& f : forms) {
        f.idle(nullptr);
        r.ctx0->synchronize();
        const std::vector<uint64_t> want = words(out);
        const double t_enqueue = gate.gated(f.what, {late(a, zero, ra), late(b, zero, rb), late(z, zero, rz)}, {out_of(out)}, f.held);
        CHECK(words(out) == want);
        std::printf("%s behind the gate: t_enqueue %.3f ms, G %.1f ms\n", f.what, t_enqueue * 1e3, gate.G * 1e3);
    }
    CHECK(gate.gated_calls == 3);
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "ref") return run_ref();
    if (mode != "words" && mode != "bound" && mode != "gate") { std::printf("usage: product_sum_words words | bound | gate [seconds] | ref\n"); return 2; }
    try {
        Rig r;
        if (mode == "words") run_words(r);
        else if (mode == "bound") run_bound(r);
        else {
            Gate gate(argc > 2 ? std::atof(argv[2]) : 0.040);
            if (!gate.ok()) { std::printf("no non-blocking stream\n"); return 2; }
            run_gate(r, gate);
        }
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    return finish(mode == "words" ? "product sum words OK" : mode == "bound" ? "product sum bound OK" : "product sum gate OK");
}
