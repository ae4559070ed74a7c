// GPU test of hoisted slot sums in the C++ facade (HybridKeySwitcher::rotate_sum_range, SlotSum's radix argument) at N = 4096, five data limbs + P, three tokens,
// cases (block, stride, radix) = (64, 1, 8), (64, 16, 4), (32, 1, 8) - the last with a remainder stage of 4.  Per case: the stages and elements the header
// states; approximate family, every decoded slot within SlotSum::error_bound (both forms agree; at most 2^-10 of max|sum| >= 1) of the float64 sum; exact
// family, the decrypted slots equal the sums mod t in both rows; radix 2 gives the words of rotate_add_range on the ladder's elements.  Then rotate_sum_range
// on an item range, apply() behind the stream gate of tests/cpp/facade_test.h, the rejections.  Built and run by tests/test_gpu_slot_sum_radix.py.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#define FACADE_TEST_GATE
#include "../facade_test.h"

using namespace deeppowers::fhe;
using namespace facade_test;
typedef std::complex<double> cplx;

static const unsigned kLog2N = 12;
static const size_t kDataLimbs = 5, kTokens = 3, kN = (size_t)1 << kLog2N, kRow = kN / 2;
static const double kScale = std::ldexp(1.0, 50), kX = 1.0, kFresh = 21.0 + 0.5 + 8.0 * kLog2N * std::ldexp(1.0, -53) * kScale * kX;
static const size_t kCases[][3] = {{64, 1, 8}, {64, 16, 4}, {32, 1, 8}};   // (block, stride, radix)
static const uint64_t kT = 65537;

struct Rig {
    uint64_t special = 0, special_psi = 0;
    FheParams params;
    Context ctx;
    KeyGenerator kg;
    HybridKeySwitcher ks;
    ComplexEncoder cenc;
    BatchEncoder benc;
    Encryptor enc;
    Decryptor dec;
    Rig() : params(ring(kLog2N, kDataLimbs, special, special_psi)), ctx(params, 0), kg(ctx, TestSeed{31}), ks(ctx, kg.secret_key(), special, special_psi, TestSeed{32}),
            cenc(ctx), benc(ctx, kT), enc(ctx, kg.secret_key(), TestSeed{33}), dec(ctx, kg.secret_key()) {}
};

static uint64_t pow3(uint64_t e) { return modpow(3, e, 2 * kN); }

static void run_case(Rig& r, size_t block, size_t stride, size_t radix) {
    SlotSum sum(r.ks, block, stride, radix), ladder(r.ks, block, stride, 2);
    std::vector<uint32_t> want_elts, ladder_elts;   // stage s: 3^(stride w_s k), k = 1 .. rho_s - 1
    size_t stages = 0;
    for (size_t w = 1; w < block; ++stages) {
        const size_t rho = std::min(radix, block / w);
        for (size_t k = 1; k < rho; ++k) want_elts.push_back((uint32_t)pow3(stride * w * k));
        w *= rho;
    }
    for (size_t b = 1; b < block; b *= 2) ladder_elts.push_back((uint32_t)pow3(stride * b));
    CHECK(sum.radix() == radix && sum.steps() == stages && sum.galois_elements() == want_elts && ladder.galois_elements() == ladder_elts);
    SplitMix64 rng;
    rng.state = 7000 + 17 * block + stride;
    // approximate family: slots uniform on [0.5, 1], no period
    std::vector<double> x(kTokens * kRow);
    std::vector<int64_t> msg(kTokens * kN), out(kTokens * kN);
    std::vector<cplx> z(kRow);
    for (size_t t = 0; t < kTokens; ++t) {
        for (size_t i = 0; i < kRow; ++i) z[i] = cplx(x[t * kRow + i] = 0.5 + 0.5 * rng.unit(), 0.0);
        r.cenc.encode(z.data(), kScale, &msg[t * kN]);
    }
    Ciphertext cx(r.ctx, 2, kTokens), cy(r.ctx, 2, kTokens), cl(r.ctx, 2, kTokens), cr(r.ctx, 2, kTokens);
    r.enc.encrypt(msg.data(), 0, cx);
    sum.apply(cx, cy);
    ladder.apply(cx, cl);
    r.ks.rotate_add_range(cx, 0, kTokens, ladder_elts, cr, 0);
    r.ctx.synchronize();
    CHECK(words(cl) == words(cr) && words(cy) != words(cl));   // radix 2 is today's ladder, word for word
    r.dec.decrypt(cy, 0, out.data());
    const double bound = sum.error_bound(kScale, kX, kFresh);
    CHECK(bound == SlotSum::error_bound(kLog2N, r.params.moduli, r.special, block, kScale, kX, kFresh, radix));
    CHECK(bound < ladder.error_bound(kScale, kX, kFresh));      // fewer roundings than the ladder
    double worst = 0, smax = 0;
    for (size_t t = 0; t < kTokens; ++t) {
        r.cenc.decode(&out[t * kN], kScale, z.data());
        for (size_t i = 0; i < kRow; ++i) {
            double acc = 0;
            for (size_t j = 0; j < block; ++j) acc += x[t * kRow + (i + j * stride) % kRow];
            smax = std::max(smax, acc);
            worst = std::max(worst, std::max(std::fabs(z[i].real() - acc), std::fabs(z[i].imag())));
        }
    }
    std::printf("block %zu stride %zu radix %zu: max|sum| %.3f, max error 2^%.2f, error_bound 2^%.2f\n", block, stride, radix, smax, std::log2(worst), std::log2(bound));
    CHECK(smax >= 1.0 && bound <= std::ldexp(1.0, -10) * smax && worst <= bound);
    // exact family: slot values below t in both rows
    const size_t T = 2;
    std::vector<uint64_t> slots(T * kN), got(T * kN), dw(T * kN);
    for (auto& v : slots) v = rng.next() % kT;
    for (size_t t = 0; t < T; ++t) r.benc.encode(&slots[t * kN], &msg[t * kN]);
    Ciphertext ex(r.ctx, 2, T), ey(r.ctx, 2, T);
    r.enc.encrypt_exact(msg.data(), kT, ex);
    sum.apply(ex, ey);
    r.ctx.synchronize();
    r.dec.decrypt_exact(ey, kT, dw.data());
    size_t wrong = 0;
    for (size_t t = 0; t < T; ++t) {
        r.benc.decode(&dw[t * kN], &got[t * kN]);
        for (size_t i = 0; i < kN; ++i) {
            uint64_t acc = 0;
            for (size_t j = 0; j < block; ++j) acc += slots[t * kN + i / kRow * kRow + (i % kRow + j * stride) % kRow];
            wrong += got[t * kN + i] != acc % kT;
        }
    }
    std::printf("exact family, block %zu stride %zu radix %zu: %zu wrong slots of %zu\n", block, stride, radix, wrong, T * kN);
    CHECK(wrong == 0);
}

// the range form equals the whole-buffer stage item by item and leaves the other items alone; apply() returns while its stream is held and gives the idle
// stream's words; the rejections
static void ranges_gate_rejections(Rig& r, Gate& gate) {
    SlotSum sum(r.ks, 64, 1, 8);
    const std::vector<uint32_t> stage(sum.galois_elements().begin(), sum.galois_elements().begin() + 7);
    Ciphertext x(r.ctx, 2, kTokens), real(r.ctx, 2, kTokens), zero(r.ctx, 2, kTokens), y(r.ctx, 2, kTokens), part(r.ctx, 2, kTokens + 1);
    std::vector<int64_t> msg(kTokens * kN);
    for (size_t i = 0; i < msg.size(); ++i) msg[i] = (int64_t)(i * 2654435761u % 1000003) - 500000;
    r.enc.encrypt(msg.data(), 0, real);
    HIP(hipMemset(zero.data(), 0, zero.words() * 8));
    HIP(hipMemset(part.data(), 0, part.words() * 8));
    r.ks.rotate_sum_range(real, 0, kTokens, stage, y, 0);
    r.ks.rotate_sum_range(real, 1, 2, stage, part, 2);
    r.ctx.synchronize();
    const std::vector<uint64_t> wy = words(y), wp = words(part);
    const size_t item = wy.size() / kTokens;
    CHECK(std::equal(wp.begin() + 2 * item, wp.end(), wy.begin() + item) && std::all_of(wp.begin(), wp.begin() + 2 * item, [](uint64_t v) { return v == 0; }));
    sum.apply(real, y);
    r.ctx.synchronize();
    const std::vector<uint64_t> want = words(y);
    gate.gated("SlotSum::apply, radix 8", {late(x, zero, real)}, {out_of(y)}, [&](Stream* s) { sum.apply(x, y, s); });
    CHECK(words(y) == want);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { SlotSum s(r.ks, 64, 1, 3); }, "radix 3");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { SlotSum s(r.ks, 64, 1, 1); }, "radix 1");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { SlotSum s(r.ks, 256, 1, 128); }, "radix 128");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { r.ks.rotate_sum_range(real, 2, 2, stage, y, 0); }, "rotate_sum_range, range past the end");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { r.ks.rotate_sum_range(real, 0, 2, std::vector<uint32_t>(65, 3), y, 0); }, "rotate_sum_range, 65 elements");
    expect_error(ErrorCode::INVALID_STATE, [&] { r.ks.rotate_sum_range(real, 0, 2, std::vector<uint32_t>{5}, y, 0); }, "rotate_sum_range, element without a key");
}

int main(int argc, char** argv) {
    try {
        Gate gate(argc > 1 ? std::atof(argv[1]) : 0.040);
        if (!gate.ok()) { std::printf("no non-blocking stream\n"); return 2; }
        Rig r;
        for (const auto& c : kCases) run_case(r, c[0], c[1], c[2]);
        ranges_gate_rejections(r, gate);
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    return finish("slot sum radix C++ facade OK");
}
