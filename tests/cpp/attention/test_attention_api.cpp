// GPU test of the attention scores in the C++ facade (ApproxAttentionScores) on ENCRYPTED queries and keys on 60-bit fold primes with the special prime.  Built
// and run by tests/test_gpu_attention_scores.py (-m gpu), one process per case.
//   test_attention_api run <log2 N> <T> <packing: one | heads> <causal: 0 | 1> [gate seconds]
//       T queries against T keys; packing `one`: one head of 12 values in a block of 16, stride 1; packing `heads`: 3 heads of 8 values interleaved at stride 4
//       (slot dim * 4 + head; the fourth head's slots hold zeros) - the small stand-in for GPT-2's 12 heads of 64 at stride 16; post_factor = 1 / 8.
//       EVERY slot of every pair within error_bound of the float64 score of its residue class (zero in the slots of the absent head); the measured error and
//       the bound are printed; distinct pairs' scores differ by more than four times the bound, so a transposed or mis-indexed pair cannot pass;
//       word for word multiply_rescale_range on the two pair lists copied out item by item followed by SlotSum::apply on the next level;
//       apply() returns while its stream is held (the gate of tests/cpp/facade_test.h) and gives the words of the idle stream; the rejections.
//   test_attention_api ref
//       no device: the static error_bound per case, and that it grows with its arguments.
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

static const double kScale = std::ldexp(1.0, 55), kPost = 0.125, kU = std::ldexp(1.0, -53);

struct Packing {
    size_t block, stride, heads, dims;   // heads * dims values per token; slot s holds value (dim = (s / stride) % block, head = s % stride), zero outside
    static Packing of(const std::string& name) { return name == "one" ? Packing{16, 1, 1, 12} : Packing{8, 4, 3, 8}; }
};

// the values of one side: [T][heads][dims], uniform on [-1, 1], and what a slot of token t holds
struct Side {
    Packing p;
    std::vector<double> v;
    Side(const Packing& pk, size_t T, uint64_t seed) : p(pk), v(T * pk.heads * pk.dims) {
        SplitMix64 rng;
        rng.state = seed;
        for (auto& x : v) x = rng.sym();
    }
    double at(size_t t, size_t head, size_t dim) const { return v[(t * p.heads + head) * p.dims + dim]; }
    double slot(size_t t, size_t s) const {
        const size_t head = s % p.stride, dim = (s / p.stride) % p.block;
        return head < p.heads && dim < p.dims ? at(t, head, dim) : 0.0;
    }
    double max_abs() const { double m = 0; for (double x : v) m = std::max(m, std::fabs(x)); return m; }
};

// post_factor <q_i, k_j> of one head in float64, dims ascending
static double score(const Side& q, const Side& k, size_t i, size_t j, size_t head) {
    double s = 0;
    for (size_t d = 0; d < q.p.dims; ++d) s += q.at(i, head, d) * k.at(j, head, d);
    return kPost * s;
}

static double fresh_noise_bound(unsigned log2n, double scale, double X) { return 21.0 + 0.5 + 8.0 * log2n * kU * scale * X; }

struct Rig {
    unsigned log2n;
    uint64_t special = 0, special_psi = 0;
    std::vector<FheParams> params;
    std::vector<std::unique_ptr<Context>> ctx;   // level 0, 1
    std::unique_ptr<KeyGenerator> kg;
    std::vector<std::unique_ptr<SecretKey>> sk;
    std::vector<std::unique_ptr<HybridKeySwitcher>> hks;
    std::unique_ptr<ComplexEncoder> cenc;
    std::unique_ptr<Encryptor> enc;
    explicit Rig(unsigned log2n_) : log2n(log2n_) {
        params.push_back(ring(log2n, 3, special, special_psi));
        params.push_back(params.back().drop_last_limb());
        for (const FheParams& p : params) ctx.emplace_back(new Context(p, 0));
        kg.reset(new KeyGenerator(*ctx[0], TestSeed{31}));
        for (size_t r = 0; r < ctx.size(); ++r) sk.emplace_back(new SecretKey(*ctx[r], kg->secret_key().coefficients()));
        for (size_t r = 0; r < ctx.size(); ++r) hks.emplace_back(new HybridKeySwitcher(*ctx[r], *sk[r], special, special_psi, TestSeed{32 + r}));
        cenc.reset(new ComplexEncoder(*ctx[0]));
        enc.reset(new Encryptor(*ctx[0], kg->secret_key(), TestSeed{34}));
    }
    size_t row() const { return params[0].n() / 2; }
    void encrypt(const Side& side, size_t T, Ciphertext& out) const {
        const size_t N = params[0].n();
        std::vector<int64_t> msg(T * N);
        std::vector<cplx> z(row());
        for (size_t t = 0; t < T; ++t) {
            for (size_t s = 0; s < row(); ++s) z[s] = cplx(side.slot(t, s), 0.0);
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

struct Pair { size_t i, j; };
static std::vector<Pair> pairs_of(size_t T, bool causal) {
    std::vector<Pair> p;
    for (size_t i = 0; i < T; ++i)
        for (size_t j = 0; j < T; ++j)
            if (!causal || j <= i) p.push_back(Pair{i, j});
    return p;
}

static void run_scores(Rig& r, size_t T, const Packing& pk, bool causal, Gate& gate) {
    const Side q(pk, T, 9100 + T), k(pk, T, 9200 + T);
    const std::vector<Pair> pairs = pairs_of(T, causal);
    ApproxAttentionScores att(*r.hks[0], *r.hks[1], T, pk.block, pk.stride, causal, kScale, kScale, kPost);
    CHECK(att.tokens() == T && att.pairs() == pairs.size() && att.causal() == causal);
    CHECK(att.output_scale() == (kScale * kScale) / (double)r.params[0].moduli.back() / kPost);   // the scale rule, in its double operations
    Ciphertext cq(*r.ctx[0], 2, T), ck(*r.ctx[0], 2, T), scores(*r.ctx[1], 2, pairs.size());
    r.encrypt(q, T, cq);
    r.encrypt(k, T, ck);
    att.apply(cq, ck, scores);
    r.ctx[0]->synchronize();
    CHECK(!scores.is_ntt());
    const std::vector<uint64_t> got = words(scores);
    // every slot of every pair against float64 and the bound
    const double A = q.max_abs(), B = k.max_abs();
    const double bound = att.error_bound(A, B, fresh_noise_bound(r.log2n, kScale, A), fresh_noise_bound(r.log2n, kScale, B));
    CHECK(bound == ApproxAttentionScores::error_bound(r.log2n, r.params[0].moduli, r.special, pk.block, kScale, kScale, kPost, A, B, fresh_noise_bound(r.log2n, kScale, A),
                                                      fresh_noise_bound(r.log2n, kScale, B)));
    const std::vector<cplx> z = r.decrypt(scores, att.output_scale());
    double worst = 0, gap = INFINITY;
    for (size_t a = 0; a < pairs.size(); ++a) {
        for (size_t s = 0; s < r.row(); ++s) {
            const size_t head = s % pk.stride;
            const double want = head < pk.heads ? score(q, k, pairs[a].i, pairs[a].j, head) : 0.0;
            worst = std::max(worst, std::max(std::fabs(z[a * r.row() + s].real() - want), std::fabs(z[a * r.row() + s].imag())));
        }
        for (size_t b = 0; b < a; ++b)
            for (size_t h = 0; h < pk.heads; ++h) gap = std::min(gap, std::fabs(score(q, k, pairs[a].i, pairs[a].j, h) - score(q, k, pairs[b].i, pairs[b].j, h)));
    }
    std::printf("attention scores at N = %zu, T = %zu, block %zu stride %zu%s: %zu pairs x %zu slots, max error 2^%.2f, error_bound 2^%.2f, smallest gap between pairs 2^%.2f\n",
                r.params[0].n(), T, pk.block, pk.stride, causal ? " causal" : "", pairs.size(), r.row(), std::log2(worst), std::log2(bound), std::log2(gap));
    CHECK(worst <= bound);
    CHECK(pairs.size() < 2 || gap >= 4 * bound);
    // word for word: the product step on pair lists copied out item by item, then SlotSum on the next level
    {
        const size_t item = 2 * r.params[0].n_limbs() * r.params[0].n() * 8;
        Ciphertext lhs(*r.ctx[0], 2, pairs.size()), rhs(*r.ctx[0], 2, pairs.size()), prod(*r.ctx[1], 2, pairs.size()), want(*r.ctx[1], 2, pairs.size());
        for (size_t a = 0; a < pairs.size(); ++a) {
            HIP(hipMemcpy((char*)lhs.data() + a * item, (const char*)cq.data() + pairs[a].i * item, item, hipMemcpyDeviceToDevice));
            HIP(hipMemcpy((char*)rhs.data() + a * item, (const char*)ck.data() + pairs[a].j * item, item, hipMemcpyDeviceToDevice));
        }
        r.hks[0]->multiply_rescale_range(lhs, 0, rhs, 0, pairs.size(), prod, 0);
        SlotSum sum(*r.hks[1], pk.block, pk.stride);
        sum.apply(prod, want);
        r.ctx[0]->synchronize();
        CHECK(words(want) == got);
    }
    // behind the gate: the Stream* path
    {
        Ciphertext a(*r.ctx[0], 2, T), b(*r.ctx[0], 2, T), za(*r.ctx[0], 2, T), zb(*r.ctx[0], 2, T);
        HIP(hipMemset(za.data(), 0, za.words() * 8));
        HIP(hipMemset(zb.data(), 0, zb.words() * 8));
        const double t_enqueue = gate.gated("ApproxAttentionScores::apply", {late(a, za, cq), late(b, zb, ck)}, {out_of(scores)}, [&](Stream* s) { att.apply(a, b, scores, s); });
        CHECK(words(scores) == got);
        std::printf("ApproxAttentionScores::apply behind the gate: t_enqueue %.3f ms, G %.1f ms\n", t_enqueue * 1e3, gate.G * 1e3);
    }
}

static void rejections(Rig& r) {
    auto build = [&](HybridKeySwitcher& a, HybridKeySwitcher& b, size_t T, size_t block, size_t stride, double qs, double post) {
        ApproxAttentionScores att(a, b, T, block, stride, false, qs, kScale, post);
    };
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(*r.hks[0], *r.hks[1], 0, 8, 4, kScale, kPost); }, "no tokens");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(*r.hks[0], *r.hks[1], 2, 6, 4, kScale, kPost); }, "block no power of two");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(*r.hks[0], *r.hks[1], 2, r.row(), 2, kScale, kPost); }, "block * stride above N / 2");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(*r.hks[0], *r.hks[1], 2, 8, 4, 0.0, kPost); }, "q_scale 0");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(*r.hks[0], *r.hks[1], 2, 8, 4, kScale, INFINITY); }, "post_factor infinite");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { build(*r.hks[0], *r.hks[0], 2, 8, 4, kScale, kPost); }, "ks_next on the same level");
    ApproxAttentionScores att(*r.hks[0], *r.hks[1], 3, 8, 4, true, kScale, kScale, kPost);
    Ciphertext q(*r.ctx[0], 2, 3), two(*r.ctx[0], 2, 2), s6(*r.ctx[1], 2, 6), s9(*r.ctx[1], 2, 9), high(*r.ctx[0], 2, 6);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { att.apply(two, q, s6); }, "apply, 2 queries for 3 tokens");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { att.apply(q, q, s9); }, "apply, 9 scores for the causal 6");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { att.apply(q, q, high); }, "apply, scores one level too high");
}

static int run_ref() {
    uint64_t special = 0, special_psi = 0;
    for (unsigned log2n : {10u, 12u}) {
        const FheParams p = ring(log2n, 3, special, special_psi);
        const double Bn = fresh_noise_bound(log2n, kScale, 1.0);
        auto bound = [&](size_t block, double A, double B, double Bq) {
            return ApproxAttentionScores::error_bound(log2n, p.moduli, special, block, kScale, kScale, kPost, A, B, Bq, Bn);
        };
        const double b8 = bound(8, 1, 1, Bn);
        std::printf("static error_bound at log2 N = %u, block 8: 2^%.2f; block 64: 2^%.2f\n", log2n, std::log2(b8), std::log2(bound(64, 1, 1, Bn)));
        CHECK(b8 > 0 && bound(64, 1, 1, Bn) > b8 && bound(8, 2, 1, Bn) > b8 && bound(8, 1, 2, Bn) > b8 && bound(8, 1, 1, 2 * Bn) > b8);
        CHECK(ApproxAttentionScores::error_bound(log2n, p.moduli, special, 8, kScale, kScale, 2 * kPost, 1, 1, Bn, Bn) == 2 * b8);   // linear in post_factor (a power of two: exact)
    }
    const FheParams p = ring(10, 3, special, special_psi);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)ApproxAttentionScores::error_bound(10, {p.moduli[0]}, special, 8, kScale, kScale, kPost, 1, 1, 1, 1); }, "error_bound: one limb");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { (void)ApproxAttentionScores::error_bound(10, p.moduli, special, 8, kScale, kScale, 0.0, 1, 1, 1, 1); }, "error_bound: post_factor 0");
    return finish("attention scores reference OK");
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "ref") return run_ref();
    if (mode != "run" || argc < 6) { std::printf("usage: test_attention_api run <log2 N> <T> <one | heads> <causal 0 | 1> [gate seconds] | ref\n"); return 2; }
    const unsigned log2n = (unsigned)std::atoi(argv[2]);
    const size_t T = (size_t)std::atoi(argv[3]);
    const std::string packing = argv[4];
    if (log2n < 10 || log2n > 13 || T < 1 || T > 8 || (packing != "one" && packing != "heads")) { std::printf("usage: log2 N in [10, 13], T in [1, 8], packing one | heads\n"); return 2; }
    try {
        Gate gate(argc > 6 ? std::atof(argv[6]) : 0.040);
        if (!gate.ok()) { std::printf("no non-blocking stream\n"); return 2; }
        Rig r(log2n);
        run_scores(r, T, Packing::of(packing), std::atoi(argv[5]) != 0, gate);
        rejections(r);
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    return finish("attention scores C++ facade OK");
}
