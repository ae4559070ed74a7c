// GPU test of complex slot encoding in the C++ facade (ComplexEncoder): the device words equal encode + a lift to every limb + an upload word for word,
// from complex and from real slots, also on the extended Q P context of a key switcher; and under encryption at N = 4096 with three 60-bit limbs and a
// special prime, Enc(x at 2^40) (.) a device-encoded w at 2^50, rotated by 5 and rescaled, decrypts and decodes to rot_5(w (.) x) within a tolerance
// computed here from the noise terms.  Built and run by tests/test_gpu_complex_encode.py (-m gpu).  Exit code 0 = all checks passed.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include "facade_test.h"
#include "dpfhe.h"

using namespace deeppowers::fhe;
typedef std::complex<double> cplx;
using namespace facade_test;

static Lcg g_lcg{2026};
static double rnd_unit() { return (double)(int64_t)(g_lcg.step() >> 11) / 4503599627370496.0 - 1.0; }   // uniform in [-1, 1): the top 53 bits of the state

static uint64_t lift(int64_t v, uint64_t q) {
    const int64_t r = (int64_t)((__int128)v % (__int128)q);
    return (uint64_t)(r < 0 ? r + (int64_t)q : r);
}

// encode() + lift + upload (+ the forward transform) of `items` slot vectors on `target`'s context
static std::vector<uint64_t> host_path(const ComplexEncoder& ce, const Context& target, const std::vector<cplx>& slots, size_t items, double scale, bool to_ntt) {
    const FheParams& p = target.params();
    const size_t n = p.n(), L = p.n_limbs();
    std::vector<int64_t> c(n);
    std::vector<uint64_t> h(items * L * n);
    for (size_t i = 0; i < items; ++i) {
        ce.encode(&slots[i * (n / 2)], scale, c.data());
        for (size_t l = 0; l < L; ++l)
            for (size_t k = 0; k < n; ++k) h[(i * L + l) * n + k] = lift(c[k], p.moduli[l]);
    }
    Plaintext pt(target, items, false);
    pt.copy_from_host(h.data());
    if (to_ntt) Evaluator(target).transform_to_ntt_inplace(pt);
    target.synchronize();
    return words(pt);
}

static void word_for_word() {
    FheParams p = FheParams::n8192(3);
    const uint64_t special = p.moduli.back(), special_psi = p.psi.back();
    p.moduli.pop_back(); p.psi.pop_back();
    const size_t n = p.n(), h = n / 2, items = 3;
    Context ctx(p, 0);
    KeyGenerator kg(ctx, TestSeed{7});
    HybridKeySwitcher hks(ctx, kg.secret_key(), special, special_psi, TestSeed{8});
    const Context& ext = hks.extended_context();
    ComplexEncoder ce(ctx);
    CHECK(ce.slot_count() == h && ce.conjugation_element() == 2 * n - 1);
    CHECK(ce.galois_element(0) == 1 && ce.galois_element(1) == 3 && ce.galois_element(2) == 9);
    CHECK((uint64_t)ce.galois_element(-1) * 3 % (2 * n) == 1 && ce.galois_element((int)h) == 1);
    std::vector<cplx> z(items * h), zr(items * h);
    std::vector<double> re(items * h);
    for (size_t i = 0; i < z.size(); ++i) {
        z[i] = cplx(rnd_unit() * 3.0, rnd_unit() * 3.0);
        re[i] = z[i].real();
        zr[i] = cplx(re[i], 0.0);
    }
    double* d_slots = nullptr;
    double* d_real = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void**>(&d_slots), z.size() * 16) == hipSuccess);
    CHECK(hipMalloc(reinterpret_cast<void**>(&d_real), re.size() * 8) == hipSuccess);
    CHECK(hipMemcpy(d_slots, z.data(), z.size() * 16, hipMemcpyHostToDevice) == hipSuccess);
    CHECK(hipMemcpy(d_real, re.data(), re.size() * 8, hipMemcpyHostToDevice) == hipSuccess);
    const Context* targets[] = {&ctx, &ext};
    for (const Context* target : targets)
        for (bool to_ntt : {false, true})
            for (double scale : {1099511627776.0 /* 2^40 */, 288230376151711744.0 /* 2^58 */}) {
                Plaintext from_complex(*target, items), from_real(*target, items);
                ce.encode_device(d_slots, items, scale, from_complex, to_ntt);
                ce.encode_device(d_real, items, scale, from_real, to_ntt, /*real=*/true);
                target->synchronize();
                CHECK(from_complex.is_ntt() == to_ntt && from_real.is_ntt() == to_ntt);
                CHECK(words(from_complex) == host_path(ce, *target, z, items, scale, to_ntt));
                CHECK(words(from_real) == host_path(ce, *target, zr, items, scale, to_ntt));
            }
    Plaintext wrong_batch(ctx, items + 1);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ce.encode_device(d_slots, items, 1024.0, wrong_batch); }, "plaintext of another batch");
    Context small(FheParams::n4096_l4(), 0);
    Plaintext other(small, items), right(ctx, items);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ce.encode_device(d_slots, items, 1024.0, other); }, "plaintext of another ring degree");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ce.encode_device(nullptr, items, 1024.0, right); }, "null slots");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ce.encode_device(d_slots, items, 0.0, right); }, "scale 0");
    (void)hipFree(d_slots);
    (void)hipFree(d_real);
}

// the header's E = 8 log2(N) 2^-53 Delta max|z|
static double encode_bound(unsigned log2n, double scale, double max_abs) { return 8.0 * log2n * std::ldexp(1.0, -53) * scale * max_abs; }

// Enc(x) (.) device-encoded w, rotated left by 5, rescaled: decrypts and decodes to rot_5(w (.) x)
static void multiply_rotate_rescale() {
    FheParams p = FheParams::n4096_l4();
    const uint64_t special = p.moduli.back(), special_psi = p.psi.back();
    p.moduli.pop_back(); p.psi.pop_back();
    const size_t n = p.n(), h = n / 2, L = p.n_limbs();
    const unsigned log2n = (unsigned)p.log2_n;
    CHECK(n == 4096 && L == 3);
    const double dx = std::ldexp(1.0, 40), dw = std::ldexp(1.0, 50);
    const double q_last = (double)p.moduli.back();
    Context ctx(p, 0);
    Context next(p.drop_last_limb(), 0);
    Evaluator ev(ctx);
    KeyGenerator kg(ctx, TestSeed{27});
    Encryptor enc(ctx, kg.secret_key(), TestSeed{28});
    SecretKey sk_next(next, kg.secret_key().coefficients());
    Decryptor dec(next, sk_next);
    HybridKeySwitcher hks(ctx, kg.secret_key(), special, special_psi, TestSeed{29});
    ComplexEncoder ce(ctx);
    const uint32_t g5 = ce.galois_element(5);
    hks.add_galois_element(g5);

    std::vector<cplx> x(h), w(h), got(h);
    double max_x = 0, max_w = 0;
    for (size_t i = 0; i < h; ++i) {
        x[i] = cplx(rnd_unit(), rnd_unit()) * 0.7071;   // |x| <= 1
        w[i] = cplx(rnd_unit(), rnd_unit()) * 0.7071;
        max_x = std::fmax(max_x, std::abs(x[i]));
        max_w = std::fmax(max_w, std::abs(w[i]));
    }
    // client: encode at 2^40, encrypt
    std::vector<int64_t> cx(n), msg(n);
    ce.encode(x.data(), dx, cx.data());
    Ciphertext ct(ctx, 2, 1), prod(ctx, 2, 1), rot(ctx, 2, 1), out(next, 2, 1);
    enc.encrypt(cx.data(), 0, ct);
    // server: w never visits the host encoder
    double* d_w = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void**>(&d_w), h * 16) == hipSuccess);
    CHECK(hipMemcpy(d_w, w.data(), h * 16, hipMemcpyHostToDevice) == hipSuccess);
    Plaintext pw(ctx, 1);
    ce.encode_device(d_w, 1, dw, pw, /*to_ntt=*/true);
    ev.transform_to_ntt_inplace(ct);
    ev.multiply_plain(ct, pw, prod);
    ev.transform_from_ntt_inplace(prod);
    hks.apply_galois(prod, g5, rot);
    ev.rescale(rot, out);
    ctx.synchronize();
    next.synchronize();
    // client: decrypt at the next level, decode at 2^90 / q_last
    dec.decrypt(out, 0, msg.data());
    const double final_scale = dx * dw / q_last;
    ce.decode(msg.data(), final_scale, got.data());

    // The tolerance, from the noise terms.  A polynomial whose coefficients are bounded by B has slot values bounded by N B (a sum of N coefficients times
    // unit factors), and the slots of a product are the products of the slots (the canonical embedding is a ring map).
    const double N = (double)n;
    double s1 = 0;
    for (int8_t c : kg.secret_key().coefficients()) s1 += c ? 1.0 : 0.0;
    const double enc_x = N * (0.5 + encode_bound(log2n, dx, max_x));   // slots of the client's rounding polynomial
    const double enc_w = N * (0.5 + encode_bound(log2n, dw, max_w));   // slots of the server's
    const double slots_w = dw * max_w + enc_w;                          // slots of the encoded w
    const double fresh = N * 21.0 * slots_w;                            // the fresh error (|e_k| <= 21) times w
    const double encoder = enc_x * slots_w + dx * max_x * enc_w;        // the two encodings' own errors in the product
    double max_q = 0;
    for (uint64_t q : p.moduli) max_q = std::fmax(max_q, (double)q);
    // key switching: L digits below q_j times key errors (|e_k| <= 21), a convolution of N terms each, divided by P; then the rounding of the division
    const double key_switch = N * ((double)L * N * max_q * 21.0 / (double)special + (1.0 + s1) / 2.0);
    const double rescale = N * (1.0 + s1) / 2.0;                        // rounding of both components, through s
    double max_msg = 0;
    for (int64_t v : msg) max_msg = std::fmax(max_msg, std::fabs((double)v));
    const double decode = 8.0 * log2n * std::ldexp(1.0, -53) * N * max_msg / final_scale;   // the header's D
    const double tol = (fresh + encoder + key_switch) / (dx * dw) + rescale / final_scale + decode;
    double worst = 0;
    for (size_t i = 0; i < h; ++i) worst = std::fmax(worst, std::abs(got[i] - w[(i + 5) % h] * x[(i + 5) % h]));
    std::printf("multiply, rotate by 5, rescale at N = 4096: largest slot error %.3e, tolerance %.3e (fresh %.2e, encoder %.2e, key switch %.2e, rescale %.2e, "
                "decode %.2e)\n", worst, tol, fresh / (dx * dw), encoder / (dx * dw), key_switch / (dx * dw), rescale / final_scale, decode);
    CHECK(worst <= tol);
    CHECK(tol < 0.05);   // (slot products have modulus up to 1: the tolerance tells a right answer from a wrong one)
    double unrotated = 0;
    for (size_t i = 0; i < h; ++i) unrotated = std::fmax(unrotated, std::abs(got[i] - w[i] * x[i]));
    CHECK(unrotated > 0.1);
    (void)hipFree(d_w);
}

int main() {
    try {
        word_for_word();
        multiply_rotate_rescale();
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    return finish("complex encode C++ facade OK");
}
