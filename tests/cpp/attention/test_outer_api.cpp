// GPU test of the all-pairs product step in the C++ facade (HybridKeySwitcher::multiply_outer_rescale_range) on ENCRYPTED inputs on 60-bit fold primes with the
// special prime.  Built and run by tests/test_gpu_outer_rescale.py (-m gpu), one process per case.
//   test_outer_api run <log2 N> [gate seconds]
//       A = 5 queries against B = 6 keys (a ragged tile, a ragged end of the key loop), full, and 5 x 5 causal: word for word multiply_rescale_range on the two
//       pair lists copied out item by item; ranges that do not start at 0 write their pairs alone (the rest of the output keeps its fill); a and b one buffer;
//       every pair decrypts to the slot-wise product of what was encrypted (a transposed or mis-indexed pair cannot: the items' values differ);
//       the step returns while its stream is held (the gate of tests/cpp/facade_test.h) and gives the words of the idle stream; the rejections.
// Exit code 0 = all passed.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#define FACADE_TEST_GATE
#include "../facade_test.h"

using namespace deeppowers::fhe;
using namespace facade_test;
typedef std::complex<double> cplx;

static const size_t kA = 5, kB = 6;
static const double kScale = std::ldexp(1.0, 50);
static const uint64_t kFill = 0xA5A5A5A5A5A5A5A5ull;

struct Rig {
    unsigned log2n;
    uint64_t special = 0, special_psi = 0;
    std::vector<FheParams> params;
    std::vector<std::unique_ptr<Context>> ctx;   // level 0, 1
    std::unique_ptr<KeyGenerator> kg;
    std::vector<std::unique_ptr<SecretKey>> sk;
    std::unique_ptr<HybridKeySwitcher> hks;
    std::unique_ptr<ComplexEncoder> cenc;
    std::unique_ptr<Encryptor> enc;
    explicit Rig(unsigned log2n_) : log2n(log2n_) {
        params.push_back(ring(log2n, 3, special, special_psi));
        params.push_back(params.back().drop_last_limb());
        for (const FheParams& p : params) ctx.emplace_back(new Context(p, 0));
        kg.reset(new KeyGenerator(*ctx[0], TestSeed{21}));
        for (size_t r = 0; r < ctx.size(); ++r) sk.emplace_back(new SecretKey(*ctx[r], kg->secret_key().coefficients()));
        hks.reset(new HybridKeySwitcher(*ctx[0], *sk[0], special, special_psi, TestSeed{22}));
        cenc.reset(new ComplexEncoder(*ctx[0]));
        enc.reset(new Encryptor(*ctx[0], kg->secret_key(), TestSeed{23}));
    }
    size_t row() const { return params[0].n() / 2; }
    // item t holds value(t) + 2^-4 (i / row) in slot i: every item its own level, every slot its own offset
    void encrypt(const std::vector<double>& values, Ciphertext& out) const {
        const size_t N = params[0].n();
        std::vector<int64_t> msg(values.size() * N);
        std::vector<cplx> z(row());
        for (size_t t = 0; t < values.size(); ++t) {
            for (size_t i = 0; i < row(); ++i) z[i] = cplx(values[t] + 0.0625 * (double)i / (double)row(), 0.0);
            cenc->encode(z.data(), kScale, &msg[t * N]);
        }
        enc->encrypt(msg.data(), 0, out);
    }
    std::vector<cplx> decrypt(const Ciphertext& ct, double scale) const {
        const size_t N = params[0].n();
        Decryptor dec(*ctx[1], *sk[1]);
        std::vector<int64_t> out(ct.batch() * N);
        dec.decrypt(ct, 0, out.data());
        std::vector<cplx> z(ct.batch() * row());
        for (size_t i = 0; i < ct.batch(); ++i) cenc->decode(&out[i * N], scale, &z[i * row()]);
        return z;
    }
};

static std::vector<double> levels(size_t count, double first) {
    std::vector<double> v(count);
    for (size_t t = 0; t < count; ++t) v[t] = first + 0.25 * (double)t;
    return v;
}

struct Pair { size_t i, j; };
static std::vector<Pair> pairs_of(size_t A, size_t B, bool causal) {
    std::vector<Pair> p;
    for (size_t i = 0; i < A; ++i)
        for (size_t j = 0; j < B; ++j)
            if (!causal || j <= i) p.push_back(Pair{i, j});
    return p;
}

// multiply_rescale_range on the pair lists copied out item by item
static std::vector<uint64_t> by_pair_lists(Rig& r, const Ciphertext& a, size_t a_first, const Ciphertext& b, size_t b_first, const std::vector<Pair>& pairs) {
    const size_t item = 2 * r.params[0].n_limbs() * r.params[0].n() * 8;
    Ciphertext lhs(*r.ctx[0], 2, pairs.size()), rhs(*r.ctx[0], 2, pairs.size()), want(*r.ctx[1], 2, pairs.size());
    for (size_t k = 0; k < pairs.size(); ++k) {
        HIP(hipMemcpy((char*)lhs.data() + k * item, (const char*)a.data() + (a_first + pairs[k].i) * item, item, hipMemcpyDeviceToDevice));
        HIP(hipMemcpy((char*)rhs.data() + k * item, (const char*)b.data() + (b_first + pairs[k].j) * item, item, hipMemcpyDeviceToDevice));
    }
    r.hks->multiply_rescale_range(lhs, 0, rhs, 0, pairs.size(), want, 0);
    r.ctx[0]->synchronize();
    return words(want);
}

static void run_words(Rig& r) {
    Ciphertext a(*r.ctx[0], 2, kA + 1), b(*r.ctx[0], 2, kB + 1);
    const std::vector<double> va = levels(kA + 1, -0.75), vb = levels(kB + 1, 0.5);
    r.encrypt(va, a);
    r.encrypt(vb, b);
    const double out_scale = (kScale * kScale) / (double)r.params[0].moduli.back();
    for (int causal = 0; causal < 2; ++causal) {
        const size_t A = kA, B = causal ? kA : kB;
        const std::vector<Pair> pairs = pairs_of(A, B, causal != 0);
        const std::vector<uint64_t> want = by_pair_lists(r, a, 1, b, 1, pairs);          // ranges that start at item 1
        Ciphertext got(*r.ctx[1], 2, pairs.size() + 2);
        HIP(hipMemset(got.data(), 0xA5, got.words() * 8));
        r.hks->multiply_outer_rescale_range(a, 1, A, b, 1, B, causal != 0, got, 1);
        r.ctx[0]->synchronize();
        const std::vector<uint64_t> g = words(got);
        const size_t out_item = want.size() / pairs.size();
        CHECK(!got.is_ntt() && g.size() == (pairs.size() + 2) * out_item);
        CHECK(std::equal(want.begin(), want.end(), g.begin() + out_item));
        CHECK(std::all_of(g.begin(), g.begin() + out_item, [](uint64_t x) { return x == kFill; }) &&
              std::all_of(g.begin() + (1 + pairs.size()) * out_item, g.end(), [](uint64_t x) { return x == kFill; }));
        // what the pairs hold: the slot-wise products of the values encrypted, pair by pair
        HIP(hipMemset(got.data(), 0, out_item * 8));
        HIP(hipMemset((char*)got.data() + (1 + pairs.size()) * out_item * 8, 0, out_item * 8));
        const std::vector<cplx> z = r.decrypt(got, out_scale);
        double worst = 0;
        for (size_t k = 0; k < pairs.size(); ++k)
            for (size_t i = 0; i < r.row(); ++i) {
                const double off = 0.0625 * (double)i / (double)r.row(), x = va[1 + pairs[k].i] + off, y = vb[1 + pairs[k].j] + off;
                worst = std::max(worst, std::fabs(z[(1 + k) * r.row() + i].real() - x * y));
            }
        std::printf("multiply_outer_rescale_range, %zu x %zu%s at N = %zu: the words of multiply_rescale_range on %zu pairs; max slot error 2^%.2f\n", A, B,
                    causal ? " causal" : "", r.params[0].n(), pairs.size(), std::log2(worst));
        CHECK(worst < std::ldexp(1.0, -12));          // the items' values are 0.25 apart: a pair that held another pair's product would miss by 2^-3 at least
    }
    {   // one buffer, one range: every product of a list with itself
        const std::vector<Pair> pairs = pairs_of(4, 4, true);
        const std::vector<uint64_t> want = by_pair_lists(r, a, 0, a, 0, pairs);
        Ciphertext got(*r.ctx[1], 2, pairs.size());
        r.hks->multiply_outer_rescale_range(a, 0, 4, a, 0, 4, true, got, 0);
        r.ctx[0]->synchronize();
        CHECK(words(got) == want);
    }
}

static void behind_the_gate(Rig& r, Gate& gate) {
    Ciphertext ra(*r.ctx[0], 2, kA), rb(*r.ctx[0], 2, kA), a(*r.ctx[0], 2, kA), b(*r.ctx[0], 2, kA), za(*r.ctx[0], 2, kA), zb(*r.ctx[0], 2, kA), out(*r.ctx[1], 2, kA * (kA + 1) / 2);
    r.encrypt(levels(kA, -1.0), ra);
    r.encrypt(levels(kA, 0.25), rb);
    HIP(hipMemset(za.data(), 0, za.words() * 8));
    HIP(hipMemset(zb.data(), 0, zb.words() * 8));
    r.hks->multiply_outer_rescale_range(ra, 0, kA, rb, 0, kA, true, out, 0, nullptr);
    r.ctx[0]->synchronize();
    const std::vector<uint64_t> want = words(out);
    const char* what = "HybridKeySwitcher::multiply_outer_rescale_range";
    const double t_enqueue = gate.gated(what, {late(a, za, ra), late(b, zb, rb)}, {out_of(out)}, [&](Stream* s) { r.hks->multiply_outer_rescale_range(a, 0, kA, b, 0, kA, true, out, 0, s); });
    CHECK(words(out) == want);
    std::printf("%s behind the gate: t_enqueue %.3f ms, G %.1f ms\n", what, t_enqueue * 1e3, gate.G * 1e3);
    CHECK(gate.gated_calls == 1);
}

static void rejections(Rig& r) {
    Ciphertext a(*r.ctx[0], 2, 4), b(*r.ctx[0], 2, 4), three(*r.ctx[0], 3, 4), o1(*r.ctx[1], 2, 16), o0(*r.ctx[0], 2, 16), low(*r.ctx[1], 2, 4);
    HIP(hipMemset(a.data(), 0, a.words() * 8));
    HIP(hipMemset(b.data(), 0, b.words() * 8));
    auto step = [&](const Ciphertext& x, size_t xf, size_t xc, const Ciphertext& y, size_t yf, size_t yc, bool causal, Ciphertext& out, size_t of) {
        r.hks->multiply_outer_rescale_range(x, xf, xc, y, yf, yc, causal, out, of);
    };
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(a, 0, 3, b, 0, 4, true, o1, 0); }, "causal, 3 queries and 4 keys");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(a, 2, 3, b, 0, 4, false, o1, 0); }, "query range past the end");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(a, 0, 4, b, 1, 4, false, o1, 0); }, "key range past the end");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(a, 0, 4, b, 0, 4, false, o1, 1); }, "output range past the end");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(a, 0, 4, b, 0, 4, false, o0, 0); }, "output on the data context");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(a, 0, 4, three, 0, 4, false, o1, 0); }, "3-component keys");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { step(low, 0, 4, b, 0, 4, false, o1, 0); }, "queries one level down");
    step(a, 0, 4, b, 0, 4, true, o1, 6);    // 10 pairs fit behind item 6 exactly
    step(a, 0, 0, b, 0, 4, false, o1, 0);   // no queries: a no-op
    step(a, 4, 0, b, 0, 0, true, o1, 16);   // nothing at all, at the very end of every buffer
    r.ctx[0]->synchronize();
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode != "run" || argc < 3) { std::printf("usage: test_outer_api run <log2 N> [gate seconds]\n"); return 2; }
    const unsigned log2n = (unsigned)std::atoi(argv[2]);
    if (log2n < 10 || log2n > 13) { std::printf("usage: log2 N in [10, 13]\n"); return 2; }
    try {
        Gate gate(argc > 3 ? std::atof(argv[3]) : 0.040);
        if (!gate.ok()) { std::printf("no non-blocking stream\n"); return 2; }
        Rig r(log2n);
        run_words(r);
        behind_the_gate(r, gate);
        rejections(r);
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    return finish("outer product C++ facade OK");
}
