// GPU test of slot sums in the C++ facade (HybridKeySwitcher::rotate_add_range, SlotSum) at N = 4096, Ld = 4: on ENCRYPTED inputs of the approximate
// family every decoded slot of every token lies within SlotSum::error_bound of the float64 sum  sum_{j < block} x[(i + j stride) mod N/2]  (blocks 2, 8 and
// 2048 at stride 1, block 8 at stride 4; three tokens), the bound is at most 2^-10 of max|sum| >= 1 (a wrong element, step count or stride gives errors of
// the order of the sums); in the exact family (block 8) the decrypted slots equal the sums mod t in both rows; apply() returns while its stream is held (the
// gate of tests/cpp/facade_test.h) and gives the same words there; the rejections.  Built and run by tests/test_gpu_slot_sum.py (-m gpu), which
// also compares the words this program dumps with the Python mirror's.
// `test_slot_sum_api ref` only draws the cases and prints max|sum| and SlotSum::error_bound of each (no device).  Exit code 0 = all passed.
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

static const unsigned kLog2N = 12;
static const size_t kDataLimbs = 4, kTokens = 3, kN = (size_t)1 << kLog2N, kRow = kN / 2;
static const double kScale = std::ldexp(1.0, 50), kX = 1.0;
static const size_t kCases[][2] = {{2, 1}, {8, 1}, {2048, 1}, {8, 4}};   // (block, stride)
static const uint64_t kT = 65537;

// one case: the tokens' slots uniform on [0.5, 1] (no period: the general statement of the sum), the float64 sums
struct Case {
    size_t block, stride;
    std::vector<double> x, y;   // [kTokens][N/2]
    double smax = 0;
    Case(size_t b, size_t s) : block(b), stride(s) {
        g_rng.state = 9000 + 17 * b + s;
        x.resize(kTokens * kRow); y.resize(kTokens * kRow);
        for (auto& v : x) v = 0.5 + 0.5 * g_rng.unit();
        for (size_t t = 0; t < kTokens; ++t)
            for (size_t i = 0; i < kRow; ++i) {
                double acc = 0;
                for (size_t j = 0; j < block; ++j) acc += x[t * kRow + (i + j * stride) % kRow];
                y[t * kRow + i] = acc;
                smax = std::max(smax, std::fabs(acc));
            }
    }
};

static double fresh_noise_bound() { return 21.0 + 0.5 + 8.0 * kLog2N * std::ldexp(1.0, -53) * kScale * kX; }

struct Rig {
    uint64_t special = 0, special_psi = 0;
    FheParams params;
    std::unique_ptr<Context> ctx;
    std::unique_ptr<KeyGenerator> kg;
    std::unique_ptr<HybridKeySwitcher> ks;
    std::unique_ptr<ComplexEncoder> cenc;
    std::unique_ptr<BatchEncoder> benc;
    std::unique_ptr<Encryptor> enc;
    Rig() : params(ring(kLog2N, kDataLimbs, special, special_psi)) {
        ctx.reset(new Context(params, 0));
        kg.reset(new KeyGenerator(*ctx, TestSeed{21}));
        ks.reset(new HybridKeySwitcher(*ctx, kg->secret_key(), special, special_psi, TestSeed{22}));
        cenc.reset(new ComplexEncoder(*ctx));
        benc.reset(new BatchEncoder(*ctx, kT));
        enc.reset(new Encryptor(*ctx, kg->secret_key(), TestSeed{23}));
    }
    void encrypt(const double* slots, size_t items, Ciphertext& out) const {   // real slots [items][N/2] at kScale
        std::vector<int64_t> msg(items * kN);
        std::vector<cplx> z(kRow);
        for (size_t t = 0; t < items; ++t) {
            for (size_t i = 0; i < kRow; ++i) z[i] = cplx(slots[t * kRow + i], 0.0);
            cenc->encode(z.data(), kScale, &msg[t * kN]);
        }
        enc->encrypt(msg.data(), 0, out);
    }
    std::vector<cplx> decrypt(const Ciphertext& ct) const {
        Decryptor dec(*ctx, kg->secret_key());
        std::vector<int64_t> out(ct.batch() * kN);
        dec.decrypt(ct, 0, out.data());
        std::vector<cplx> z(ct.batch() * kRow);
        for (size_t i = 0; i < ct.batch(); ++i) cenc->decode(&out[i * kN], kScale, &z[i * kRow]);
        return z;
    }
};

static void run_approx(Rig& r, size_t block, size_t stride) {
    const Case c(block, stride);
    SlotSum sum(*r.ks, block, stride);
    size_t log2b = 0;
    while (((size_t)1 << log2b) < block) ++log2b;
    CHECK(sum.block() == block && sum.stride() == stride && sum.steps() == log2b && sum.galois_elements().size() == log2b);
    for (size_t e = 0; e < log2b; ++e) CHECK(sum.galois_elements()[e] == r.cenc->galois_element((int)(stride << e)));
    Ciphertext x(*r.ctx, 2, kTokens), y(*r.ctx, 2, kTokens);
    r.encrypt(c.x.data(), kTokens, x);
    sum.apply(x, y);
    r.ctx->synchronize();
    CHECK(!y.is_ntt());
    const std::vector<cplx> z = r.decrypt(y);
    const double bound = sum.error_bound(kScale, kX, fresh_noise_bound());
    CHECK(bound == SlotSum::error_bound(kLog2N, r.params.moduli, r.special, block, kScale, kX, fresh_noise_bound()));
    double worst = 0;
    for (size_t i = 0; i < kTokens * kRow; ++i) worst = std::max(worst, std::max(std::fabs(z[i].real() - c.y[i]), std::fabs(z[i].imag())));
    std::printf("block %zu stride %zu, %zu tokens: max|sum| %.3f, max error 2^%.2f, error_bound 2^%.2f (%zu slots)\n", block, stride, kTokens, c.smax,
                std::log2(worst), std::log2(bound), kTokens * kRow);
    CHECK(c.smax >= 1.0);
    CHECK(bound <= std::ldexp(1.0, -10) * c.smax);
    CHECK(worst <= bound);
}

// exact family: slot values below t in both rows, block 8; the sums mod t, row by row
static void run_exact(Rig& r) {
    const size_t block = 8, T = 2;
    SlotSum sum(*r.ks, block);
    g_rng.state = 515;
    std::vector<uint64_t> slots(T * kN), got(T * kN), dec(T * kN);
    std::vector<int64_t> msg(T * kN);
    for (auto& v : slots) v = g_rng.next() % kT;
    for (size_t t = 0; t < T; ++t) r.benc->encode(&slots[t * kN], &msg[t * kN]);
    Ciphertext x(*r.ctx, 2, T), y(*r.ctx, 2, T);
    r.enc->encrypt_exact(msg.data(), kT, x);
    sum.apply(x, y);
    r.ctx->synchronize();
    Decryptor d(*r.ctx, r.kg->secret_key());
    d.decrypt_exact(y, kT, dec.data());
    size_t wrong = 0;
    for (size_t t = 0; t < T; ++t) {
        r.benc->decode(&dec[t * kN], &got[t * kN]);
        for (size_t row = 0; row < 2; ++row)
            for (size_t i = 0; i < kRow; ++i) {
                uint64_t acc = 0;
                for (size_t j = 0; j < block; ++j) acc += slots[t * kN + row * kRow + (i + j) % kRow];
                wrong += got[t * kN + row * kRow + i] != acc % kT;
            }
    }
    std::printf("exact family, block %zu, %zu items: %zu wrong slots of %zu, noise budget %.0f bits\n", block, T, wrong, T * kN, d.noise_budget_bits(y, kT));
    CHECK(wrong == 0);
}

// rotate_add_range on item ranges of one buffer, and the same words as apply_galois_grouped + a modular add would give is the C ABI tests' matter; here:
// the range form equals apply() item by item, and untouched items stay
static void run_ranges(Rig& r) {
    const Case c(8, 1);
    SlotSum sum(*r.ks, 8);
    Ciphertext x(*r.ctx, 2, kTokens), y(*r.ctx, 2, kTokens), part(*r.ctx, 2, kTokens + 1);
    r.encrypt(c.x.data(), kTokens, x);
    sum.apply(x, y);
    CHECK(hipMemset(part.data(), 0, part.words() * 8) == hipSuccess);
    r.ks->rotate_add_range(x, 1, 2, sum.galois_elements(), part, 2);
    r.ctx->synchronize();
    const std::vector<uint64_t> wy = words(y), wp = words(part);
    const size_t item = wy.size() / kTokens;
    CHECK(std::equal(wp.begin() + 2 * item, wp.end(), wy.begin() + item));
    CHECK(std::all_of(wp.begin(), wp.begin() + 2 * item, [](uint64_t v) { return v == 0; }));
}

// the gate, with the full protocol: zero words in the input buffer during the warm-up and the gate, the encrypted tokens copied in on S behind it, the
// output wiped on S behind it; the call comes back with the event pending, within G / 4, and gives the words of the idle stream
static void behind_the_gate(Rig& r, Gate& gate, const char* dump) {
    const Case c(2048, 1);
    SlotSum sum(*r.ks, 2048);
    Ciphertext x(*r.ctx, 2, kTokens), real(*r.ctx, 2, kTokens), zero(*r.ctx, 2, kTokens), y(*r.ctx, 2, kTokens);
    r.encrypt(c.x.data(), kTokens, real);
    HIP(hipMemset(zero.data(), 0, zero.words() * 8));
    sum.apply(real, y);
    r.ctx->synchronize();
    const std::vector<uint64_t> want = words(y);
    const double t_enqueue = gate.gated("SlotSum::apply", {late(x, zero, real)}, {out_of(y)}, [&](Stream* s) { sum.apply(x, y, s); });
    CHECK(words(y) == want);
    std::printf("SlotSum::apply behind the gate: t_enqueue %.3f ms, G %.1f ms\n", t_enqueue * 1e3, gate.G * 1e3);
    if (dump) {   // what the Python mirror is compared with: the context, the ladder's elements and packed keys, the input and output words of item 0 and 1
        const FheParams& pe = r.ks->extended_context().params();
        const size_t L = pe.n_limbs(), Ld = L - 1, steps = sum.steps(), T = 2;
        Ciphertext in2(*r.ctx, 2, T), out2(*r.ctx, 2, T);
        CHECK(hipMemcpy(in2.data(), x.data(), in2.words() * 8, hipMemcpyDeviceToDevice) == hipSuccess);
        r.ks->rotate_add_range(in2, 0, T, sum.galois_elements(), out2, 0);
        r.ctx->synchronize();
        std::vector<uint64_t> keys(steps * Ld * 2 * L * kN);
        for (size_t e = 0; e < steps; ++e) r.ks->galois_key(sum.galois_elements()[e]).copy_to_host(&keys[e * Ld * 2 * L * kN]);
        FILE* f = std::fopen(dump, "wb");
        CHECK(f != nullptr);
        if (f) {
            std::vector<uint64_t> head{0x534C4F5453554D31ull, kLog2N, L, steps, T};
            for (uint64_t q : pe.moduli) head.push_back(q);
            for (uint64_t w : pe.psi) head.push_back(w);
            for (uint32_t g : sum.galois_elements()) head.push_back(g);
            const std::vector<uint64_t> wi = words(in2), wo = words(out2);
            CHECK(std::fwrite(head.data(), 8, head.size(), f) == head.size() && std::fwrite(keys.data(), 8, keys.size(), f) == keys.size() &&
                  std::fwrite(wi.data(), 8, wi.size(), f) == wi.size() && std::fwrite(wo.data(), 8, wo.size(), f) == wo.size());
            std::fclose(f);
        }
    }
}

static void rejections(Rig& r) {
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { SlotSum s(*r.ks, 1); }, "block 1");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { SlotSum s(*r.ks, 0); }, "block 0");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { SlotSum s(*r.ks, 6); }, "block 6");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { SlotSum s(*r.ks, 8, 3); }, "stride 3");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { SlotSum s(*r.ks, 8, 0); }, "stride 0");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { SlotSum s(*r.ks, kRow * 2); }, "block N");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { SlotSum s(*r.ks, kRow, 2); }, "block * stride = N");
    SlotSum whole(*r.ks, kRow);   // the largest: block * stride = N / 2
    CHECK(whole.steps() == kLog2N - 1);
    SlotSum sum(*r.ks, 8);
    Ciphertext x(*r.ctx, 2, 2), one(*r.ctx, 2, 1), three(*r.ctx, 3, 2), y(*r.ctx, 2, 2);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { sum.apply(x, one); }, "apply, output batch");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { sum.apply(three, y); }, "apply, 3 components");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { sum.apply(x, x); }, "apply, output is the input");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { r.ks->rotate_add_range(x, 1, 2, sum.galois_elements(), y, 0); }, "rotate_add_range, range past the end");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { r.ks->rotate_add_range(x, 0, 2, std::vector<uint32_t>(), y, 0); }, "rotate_add_range, no element");
    expect_error(ErrorCode::INVALID_STATE, [&] { r.ks->rotate_add_range(x, 0, 2, std::vector<uint32_t>{5, 25}, y, 0); }, "rotate_add_range, element without a key");
    x.set_ntt(true);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { sum.apply(x, y); }, "apply, NTT-domain input");
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "ref") {
        uint64_t special = 0, special_psi = 0;
        const FheParams p = ring(kLog2N, kDataLimbs, special, special_psi);
        for (const auto& bs : kCases) {
            const Case c(bs[0], bs[1]);
            const double bound = SlotSum::error_bound(kLog2N, p.moduli, special, bs[0], kScale, kX, fresh_noise_bound());
            std::printf("block %zu stride %zu: max|sum| = %.4f error_bound = 2^%.2f ratio = 2^%.2f\n", bs[0], bs[1], c.smax, std::log2(bound), std::log2(bound / c.smax));
        }
        return 0;
    }
    const double G = argc > 1 ? std::atof(argv[1]) : 0.040;
    const char* dump = argc > 2 ? argv[2] : nullptr;
    try {
        Gate gate(G);
        if (!gate.ok()) { std::printf("no non-blocking stream\n"); return 2; }
        Rig r;
        for (const auto& bs : kCases) run_approx(r, bs[0], bs[1]);
        run_exact(r);
        run_ranges(r);
        behind_the_gate(r, gate, dump);
        rejections(r);
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    return finish("slot sum C++ facade OK");
}
