// fhe_polynomial.cpp - the facade's slot-wise polynomial of the approximate (CKKS-style) family (ApproxPolynomial): the power schedule over the levels'
// key switchers, the scale rule and the error bound of include/deeppowers/fhe.hpp.  Part of libdpfhe_api.so (fhe_api.cpp names the other units).
#include <algorithm>
#include <cmath>

#include "fhe_internal.h"

namespace deeppowers {
namespace fhe {

using namespace detail;

namespace {

constexpr size_t kMinDegree = 2, kMaxDegree = 15;

size_t ceil_log2(size_t k) {
    size_t r = 0;
    while (((size_t)1 << r) < k) ++r;
    return r;
}

// s_1 .. s_d by the header's rule; drop[r] = the prime a product at level r + 1 drops
std::vector<double> power_scales(size_t d, double input_scale, const std::vector<uint64_t>& drop) {
    std::vector<double> s(d + 1, 0.0);
    s[1] = input_scale;
    for (size_t k = 2; k <= d; ++k) {
        const size_t r = ceil_log2(k), i = (size_t)1 << (r - 1), j = k - i;
        s[k] = (s[i] * s[j]) / (double)drop[r - 1];
    }
    return s;
}

bool same_params(const FheParams& a, const FheParams& b) { return a.log2_n == b.log2_n && a.moduli == b.moduli && a.psi == b.psi; }

void check_shape(const std::vector<double>& coeffs, size_t levels, double input_scale, double output_scale) {
    if (coeffs.size() < kMinDegree + 1 || coeffs.size() > kMaxDegree + 1) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxPolynomial: the degree must lie in [2, 15]");
    if (levels != ceil_log2(coeffs.size() - 1)) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxPolynomial: ceil(log2 degree) levels, input level first");
    for (double a : coeffs)
        if (!std::isfinite(a)) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxPolynomial: coefficients must be finite");
    if (!(std::isfinite(input_scale) && input_scale > 0) || !(std::isfinite(output_scale) && output_scale > 0))
        throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxPolynomial: scales must be finite and positive");
}

}  // namespace

class __attribute__((visibility("hidden"))) ApproxPolynomial::Impl {
public:
    std::vector<HybridKeySwitcher*> levels;
    std::vector<const Context*> ctx;     // depth 0 .. r*: the levels' data contexts, then sum_ctx
    const Context* out = nullptr;
    std::vector<double> a, s;            // a_0 .. a_d; s_1 .. s_d (s[0] unused)
    std::vector<int64_t> c;              // c_0 .. c_d
    std::vector<uint64_t> special;       // P of every level
    double x_scale = 0, y_scale = 0;
    size_t d = 0, rstar = 0;
    uint64_t* d_w = nullptr;             // [d + 1][L of sum_ctx]: rows c_1 .. c_d, then c_0
    // scratch, grown for a larger T: powers of depth r (1 <= r < r*) as [power][T]; both operands of level r as [power][T] at depth r - 1; all powers at depth r*
    std::vector<std::unique_ptr<Ciphertext>> lvl, op_a, op_b;
    std::unique_ptr<Ciphertext> terms;

    size_t first_power(size_t r) const { return r ? ((size_t)1 << (r - 1)) + 1 : 1; }            // the powers of depth r: first .. last
    size_t last_power(size_t r) const { return r ? std::min((size_t)1 << r, d) : 1; }
    size_t ct_words(size_t depth) const { return 2 * ctx[depth]->params().n_limbs() * ctx[depth]->params().n(); }
    ~Impl() { if (d_w) (void)hipFree(d_w); }
};

ApproxPolynomial::ApproxPolynomial(const std::vector<HybridKeySwitcher*>& levels, const Context& sum_ctx, const Context& out_ctx, const std::vector<double>& coeffs,
                                   double input_scale, double output_scale)
    : impl_(new Impl) {
    Impl& I = *impl_;
    check_shape(coeffs, levels.size(), input_scale, output_scale);
    I.d = coeffs.size() - 1; I.rstar = levels.size(); I.a = coeffs; I.x_scale = input_scale; I.y_scale = output_scale; I.levels = levels; I.out = &out_ctx;
    for (HybridKeySwitcher* ks : levels) {
        if (!ks) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxPolynomial: null key switcher");
        I.ctx.push_back(&ks->data_context());
        I.special.push_back(ks->extended_context().params().moduli.back());
    }
    I.ctx.push_back(&sum_ctx);
    for (size_t r = 0; r + 1 < I.ctx.size(); ++r)
        if (I.ctx[r]->params().n_limbs() < 2 || !same_params(I.ctx[r + 1]->params(), I.ctx[r]->params().drop_last_limb()) || I.ctx[r + 1]->device_id() != I.ctx[0]->device_id())
            throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxPolynomial: every level's context must be the one before it without its last limb, on the same device");
    if (sum_ctx.params().n_limbs() < 2 || !same_params(out_ctx.params(), sum_ctx.params().drop_last_limb()) || out_ctx.device_id() != sum_ctx.device_id())
        throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxPolynomial: out_ctx must be a context on sum_ctx.params().drop_last_limb(), on the same device");
    std::vector<uint64_t> drop;
    for (size_t r = 0; r < I.rstar; ++r) drop.push_back(I.ctx[r]->params().moduli.back());
    I.s = power_scales(I.d, input_scale, drop);
    const FheParams& ps = sum_ctx.params();
    const double top = output_scale * (double)ps.moduli.back();
    I.c.assign(I.d + 1, 0);
    for (size_t k = 0; k <= I.d; ++k) {
        const double v = k ? coeffs[k] * (top / I.s[k]) : coeffs[0] * output_scale;   // (c[0] is the constant at the OUTPUT scale: c_0 = c[0] q*)
        if (!(std::fabs(v) < std::ldexp(1.0, 62))) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxPolynomial: a weight |c_k| reaches 2^62 (lower output_scale or the coefficient)");
        I.c[k] = std::llround(v);
    }
    std::vector<int64_t> rows(I.c.begin() + 1, I.c.end());   // c_1 .. c_d, then the constant row: c_0 = llround(a_0 S) q*
    rows.push_back(I.c[0]);
    const std::vector<uint64_t> w = signed_weight_rows(ps, rows, I.d);
    I.d_w = device_alloc<uint64_t>(sum_ctx.device_id(), w.size());
    hip_check(hipMemcpy(I.d_w, w.data(), w.size() * sizeof(uint64_t), hipMemcpyHostToDevice), "hipMemcpy H2D");
    I.lvl.resize(I.rstar + 1); I.op_a.resize(I.rstar + 1); I.op_b.resize(I.rstar + 1);
}
ApproxPolynomial::~ApproxPolynomial() = default;

size_t ApproxPolynomial::degree() const { return impl_->d; }
size_t ApproxPolynomial::depth() const { return impl_->rstar + 1; }
double ApproxPolynomial::output_scale() const { return impl_->y_scale; }
double ApproxPolynomial::power_scale(size_t k) const {
    if (k < 1 || k > impl_->d) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxPolynomial::power_scale: 1 <= k <= degree");
    return impl_->s[k];
}
int64_t ApproxPolynomial::weight(size_t k) const {
    if (k > impl_->d) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxPolynomial::weight: k <= degree");
    return impl_->c[k];
}

double ApproxPolynomial::error_bound(uint32_t log2_n, const std::vector<uint64_t>& data_moduli, const std::vector<uint64_t>& special_primes,
                                     const std::vector<double>& coeffs, double input_scale, double output_scale, double X, double Bin) {
    check_shape(coeffs, special_primes.size(), input_scale, output_scale);
    const size_t d = coeffs.size() - 1, rstar = special_primes.size(), L0 = data_moduli.size();
    if (L0 < rstar + 2) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxPolynomial::error_bound: the input level needs ceil(log2 degree) + 2 limbs");
    const BoundUnits bu(log2_n);
    const double N = bu.N, H = bu.H, u = bu.u, u8 = bu.u8;
    const LevelLadder ladder = level_ladder(data_moduli, special_primes, N);
    const std::vector<uint64_t>& drop = ladder.drop;
    const std::vector<double>& K = ladder.K;   // K_r of level r + 1
    const std::vector<double> s = power_scales(d, input_scale, drop);
    std::vector<double> D(d + 1, 0.0), Xp(d + 1, 1.0);
    for (size_t k = 1; k <= d; ++k) Xp[k] = Xp[k - 1] * X;
    D[1] = N * Bin;
    for (size_t k = 2; k <= d; ++k) {
        const size_t r = ceil_log2(k), i = (size_t)1 << (r - 1), j = k - i;
        D[k] = (s[i] * Xp[i] * D[j] + s[j] * Xp[j] * D[i] + D[i] * D[j] + N * (K[r - 1] + H)) / (double)drop[r - 1] + N * H + 4 * u * s[k] * Xp[k];
    }
    const double top = output_scale * (double)data_moduli[L0 - rstar - 1];
    double sum = (double)data_moduli[L0 - rstar - 1] * (0.5 + 2 * u * std::fabs(coeffs[0]) * output_scale), A = std::fabs(coeffs[0]);
    for (size_t k = 1; k <= d; ++k) {
        const double ak = std::fabs(coeffs[k]), R = 0.5 + 4 * u * ak * top / s[k];
        sum += R * s[k] * Xp[k] + ak * (top / s[k]) * D[k] + R * D[k];
        A += ak * Xp[k];
    }
    const double pre = sum / top + N * H / output_scale;
    return pre + u8 * N * (A + pre);
}

double ApproxPolynomial::error_bound(double X, double Bin) const {
    const Impl& I = *impl_;
    return error_bound(I.ctx[0]->params().log2_n, I.ctx[0]->params().moduli, I.special, I.a, I.x_scale, I.y_scale, X, Bin);
}

void ApproxPolynomial::apply(const Ciphertext& x, Ciphertext& y, Stream* stream) const {
    Impl& I = *impl_;
    const size_t T = x.batch(), d = I.d, rstar = I.rstar;
    if (x.is_ntt() || x.size() != 2 || x.words() != T * I.ct_words(0) || y.size() != 2 || y.batch() != T ||
        y.words() != T * 2 * I.out->params().n_limbs() * I.out->params().n())
        throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxPolynomial::apply: T 2-component coefficient-domain ciphertexts on the input context in, T on out_ctx out");
    if (T == 0) return;
    grow_scratch(I.terms, d * T, [&](size_t m) { return new Ciphertext(*I.ctx[rstar], 2, m); });
    // where the T items of power k live (its own depth), and a copy of them to `dst` at depth `to` (<= its own limbs: the first limbs of every polynomial)
    auto depth_of = [&](size_t k) { return ceil_log2(k); };
    auto power = [&](size_t k) -> const uint64_t* {
        const size_t r = depth_of(k);
        if (r == 0) return x.data();
        if (r == rstar) return I.terms->data() + (k - 1) * T * I.ct_words(rstar);
        return I.lvl[r]->data() + (k - I.first_power(r)) * T * I.ct_words(r);
    };
    auto drop_to = [&](uint64_t* dst, size_t to, size_t k) { keep_first_limbs(dst, *I.ctx[to], power(k), *I.ctx[depth_of(k)], 2 * T, stream); };
    for (size_t r = 1; r <= rstar; ++r) {
        const size_t first = I.first_power(r), count = I.last_power(r) - first + 1, half = (size_t)1 << (r - 1);
        Ciphertext* out = r == rstar ? I.terms.get() : &grow_scratch(I.lvl[r], count * T, [&](size_t m) { return new Ciphertext(*I.ctx[r], 2, m); });
        const size_t out_first = r == rstar ? (first - 1) * T : 0;
        if (r == 1) {   // x^2 = x * x, straight from the input
            I.levels[0]->multiply_rescale_range(x, 0, x, 0, T, *out, out_first, stream);
            continue;
        }
        Ciphertext& A = grow_scratch(I.op_a[r], count * T, [&](size_t m) { return new Ciphertext(*I.ctx[r - 1], 2, m); });
        Ciphertext& B = grow_scratch(I.op_b[r], count * T, [&](size_t m) { return new Ciphertext(*I.ctx[r - 1], 2, m); });
        for (size_t idx = 0; idx < count; ++idx) {
            drop_to(A.data() + idx * T * I.ct_words(r - 1), r - 1, half);
            drop_to(B.data() + idx * T * I.ct_words(r - 1), r - 1, first + idx - half);
        }
        I.levels[r - 1]->multiply_rescale_range(A, 0, B, 0, count * T, *out, out_first, stream);
    }
    for (size_t k = 1; k < I.first_power(rstar); ++k) drop_to(I.terms->data() + (k - 1) * T * I.ct_words(rstar), rstar, k);
    check(dpfhe_lincomb_rescale(handle_of(*I.ctx[rstar]), y.data(), I.terms->data(), I.d_w, d, T, stream), "dpfhe_lincomb_rescale");
    y.set_ntt(false);
}

}  // namespace fhe
}  // namespace deeppowers
