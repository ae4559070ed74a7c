// fhe_invsqrt.cpp - the facade's slot-wise 1 / sqrt(v) of the approximate (CKKS-style) family (ApproxInvSqrt): Newton steps y <- 1.5 y - 0.5 (v y)(y y) on a
// caller's guess, two levels each - the two products on one key switcher, their product with the weighted y in ONE fused step on the next
// (HybridKeySwitcher::multiply_lincomb_rescale_range) -, the scale rule and the error bound of include/deeppowers/fhe.hpp.  Part of libdpfhe_api.so.
#include <algorithm>
#include <cmath>

#include "fhe_internal.h"

namespace deeppowers {
namespace fhe {

using namespace detail;

namespace {

struct StepScales {
    double s_a, s_b, top, s_next;
    int64_t w;
};

bool good_scale(double s) { return std::isfinite(s) && s >= std::ldexp(1.0, 20) && s < std::ldexp(1.0, 62); }

// the header's rule, in exactly its double operations; q[i] = the prime level i drops (2 K of them).  s gets s_0 .. s_K.
std::vector<StepScales> step_scales(const std::vector<uint64_t>& q, double v_scale, double guess_scale, std::vector<double>& s) {
    if (q.empty() || (q.size() & 1)) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxInvSqrt: two levels per iteration, at least one iteration");
    if (!(std::isfinite(v_scale) && v_scale > 0) || !(std::isfinite(guess_scale) && guess_scale > 0))
        throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxInvSqrt: scales must be finite and positive");
    std::vector<StepScales> st;
    s.assign(1, guess_scale);
    for (size_t n = 0; n < q.size() / 2; ++n) {
        if (!good_scale(s[n])) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxInvSqrt: a scale s_n leaves [2^20, 2^62) (see balanced_guess_scale)");
        const double q_a = (double)q[2 * n], q_b = (double)q[2 * n + 1];
        StepScales t;
        t.s_a = (v_scale * s[n]) / q_a;
        t.s_b = (s[n] * s[n]) / q_a;
        t.top = 2.0 * (t.s_a * t.s_b);
        const double w = 1.5 * (t.top / s[n]);
        if (!(std::fabs(w) < std::ldexp(1.0, 62))) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxInvSqrt: a weight |w_n| reaches 2^62");
        t.w = std::llround(w);
        t.s_next = t.top / q_b;
        st.push_back(t);
        s.push_back(t.s_next);
    }
    if (!good_scale(s.back())) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxInvSqrt: a scale s_n leaves [2^20, 2^62) (see balanced_guess_scale)");
    return st;
}

bool same_params(const FheParams& a, const FheParams& b) { return a.log2_n == b.log2_n && a.moduli == b.moduli && a.psi == b.psi; }

}  // namespace

class __attribute__((visibility("hidden"))) ApproxInvSqrt::Impl {
public:
    std::vector<HybridKeySwitcher*> levels;
    std::vector<const Context*> ctx;     // level 0 .. 2 K - 1: the key switchers' data contexts; ctx[2 K] = out_ctx
    std::vector<uint64_t> special;       // P of every level
    std::vector<double> s;               // s_0 .. s_K
    std::vector<StepScales> st;
    std::vector<std::unique_ptr<ScalarWeights>> weights;   // per iteration, on ctx[2 n + 1]: (-1, w_n, no constant)
    double v_scale = 0;
    size_t K = 0;
    // scratch, grown for a larger T: v at level 2 n (n >= 1), the products (a | b) of iteration n at level 2 n + 1, y_n at level 2 n (n >= 1)
    std::vector<std::unique_ptr<Ciphertext>> v_at, ab, y_at;
    size_t ct_words(size_t level) const { return 2 * ctx[level]->params().n_limbs() * ctx[level]->params().n(); }
};

ApproxInvSqrt::ApproxInvSqrt(const std::vector<HybridKeySwitcher*>& levels, const Context& out_ctx, double v_scale, double guess_scale) : impl_(new Impl) {
    Impl& I = *impl_;
    if (levels.empty() || (levels.size() & 1)) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxInvSqrt: two levels per iteration, at least one iteration");
    I.levels = levels; I.K = levels.size() / 2; I.v_scale = v_scale;
    for (HybridKeySwitcher* ks : levels) {
        if (!ks) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxInvSqrt: null key switcher");
        I.ctx.push_back(&ks->data_context());
        I.special.push_back(ks->extended_context().params().moduli.back());
    }
    I.ctx.push_back(&out_ctx);
    for (size_t r = 0; r + 1 < I.ctx.size(); ++r)
        if (I.ctx[r]->params().n_limbs() < 2 || !same_params(I.ctx[r + 1]->params(), I.ctx[r]->params().drop_last_limb()) || I.ctx[r + 1]->device_id() != I.ctx[0]->device_id())
            throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxInvSqrt: every level's context (and out_ctx after the last) must be the one before it without its last limb, on the same device");
    std::vector<uint64_t> drop;
    for (size_t r = 0; r < levels.size(); ++r) drop.push_back(I.ctx[r]->params().moduli.back());
    I.st = step_scales(drop, v_scale, guess_scale, I.s);
    for (size_t n = 0; n < I.K; ++n) I.weights.emplace_back(new ScalarWeights(*I.ctx[2 * n + 1], -1, {I.st[n].w}, 0));
    I.v_at.resize(I.K); I.ab.resize(I.K); I.y_at.resize(I.K);
}
ApproxInvSqrt::~ApproxInvSqrt() = default;

size_t ApproxInvSqrt::iterations() const { return impl_->K; }
size_t ApproxInvSqrt::depth() const { return 2 * impl_->K; }
double ApproxInvSqrt::scale(size_t n) const {
    if (n > impl_->K) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxInvSqrt::scale: n <= iterations");
    return impl_->s[n];
}
int64_t ApproxInvSqrt::weight(size_t n) const {
    if (n >= impl_->K) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxInvSqrt::weight: n < iterations");
    return impl_->st[n].w;
}

double ApproxInvSqrt::balanced_guess_scale(double v_scale, uint64_t q_a, uint64_t q_b) {
    if (!(std::isfinite(v_scale) && v_scale > 0) || !q_a || !q_b) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxInvSqrt::balanced_guess_scale: a positive scale and two primes");
    return std::sqrt(((double)q_a * (double)q_a) * ((double)q_b / (2.0 * v_scale)));
}

double ApproxInvSqrt::error_bound(uint32_t log2_n, const std::vector<uint64_t>& data_moduli, const std::vector<uint64_t>& special_primes, double v_scale,
                                  double guess_scale, double V, double Y, double Bv, double By) {
    const size_t depth = special_primes.size(), L0 = data_moduli.size();
    if (depth == 0 || (depth & 1)) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxInvSqrt::error_bound: two special primes per iteration");
    if (L0 < depth + 1) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxInvSqrt::error_bound: the input level needs 2 K + 1 limbs");
    if (!(V >= 0) || !(Y >= 0) || !(Bv >= 0) || !(By >= 0)) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxInvSqrt::error_bound: magnitudes and noise bounds must be non-negative");
    const BoundUnits bu(log2_n);
    const double N = bu.N, H = bu.H, u = bu.u, u8 = bu.u8;
    const LevelLadder ladder = level_ladder(data_moduli, special_primes, N);
    const std::vector<uint64_t>& drop = ladder.drop;
    const std::vector<double>& Kr = ladder.K;
    std::vector<double> s;
    const std::vector<StepScales> st = step_scales(drop, v_scale, guess_scale, s);
    const double Dv = N * Bv, Y2 = Y * Y, Y3 = Y2 * Y;
    double E = N * By, F = 0;   // y_n's slot error in the phase; the float64 iteration's own distance from the real one
    const double g = 1.5 * (1 + V * Y2), f = 8 * u * (1.5 * Y + 0.5 * V * Y3);
    for (size_t n = 0; n < depth / 2; ++n) {
        const StepScales& t = st[n];
        const double q_a = (double)drop[2 * n], q_b = (double)drop[2 * n + 1];
        const double Da = (v_scale * V * E + s[n] * Y * Dv + Dv * E + N * (Kr[2 * n] + H)) / q_a + N * H + 4 * u * t.s_a * V * Y;
        const double Db = (2 * s[n] * Y * E + E * E + N * (Kr[2 * n] + H)) / q_a + N * H + 4 * u * t.s_b * Y2;
        const double R = 0.5 + 4 * u * 1.5 * (t.top / s[n]), w = 1.5 * (t.top / s[n]) + R;
        E = (t.s_a * V * Y * Db + t.s_b * Y2 * Da + Da * Db + N * (Kr[2 * n + 1] + H) + w * E + R * s[n] * Y + u * t.top * V * Y3) / q_b + N * H + 2 * u * t.s_next * Y;
        F = g * F + f;
    }
    const double pre = E / s.back();
    return pre + u8 * N * (Y + pre) + F;
}

double ApproxInvSqrt::error_bound(double V, double Y, double Bv, double By) const {
    const Impl& I = *impl_;
    return error_bound(I.ctx[0]->params().log2_n, I.ctx[0]->params().moduli, I.special, I.v_scale, I.s[0], V, Y, Bv, By);
}

void ApproxInvSqrt::apply(const Ciphertext& v, const Ciphertext& y0, Ciphertext& y, Stream* stream) const {
    Impl& I = *impl_;
    const size_t T = v.batch(), K = I.K;
    auto on_level0 = [&](const Ciphertext& c) { return !c.is_ntt() && c.size() == 2 && c.batch() == T && c.words() == T * I.ct_words(0); };
    if (!on_level0(v) || !on_level0(y0) || y.size() != 2 || y.batch() != T || y.words() != T * I.ct_words(2 * K))
        throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxInvSqrt::apply: v and y0 are T 2-component coefficient-domain ciphertexts on the input context, y T on out_ctx");
    if (T == 0) return;
    const Ciphertext* yn = &y0;
    for (size_t n = 0; n < K; ++n) {
        const Ciphertext* vn = &v;
        if (n) {   // v at level 2 n: the first limbs of every polynomial (the ciphertext and its scale do not change)
            Ciphertext& vd = grow_scratch(I.v_at[n], T, [&](size_t m) { return new Ciphertext(*I.ctx[2 * n], 2, m); });
            keep_first_limbs(vd.data(), *I.ctx[2 * n], v.data(), *I.ctx[0], 2 * T, stream);
            vn = &vd;
        }
        Ciphertext& ab = grow_scratch(I.ab[n], 2 * T, [&](size_t m) { return new Ciphertext(*I.ctx[2 * n + 1], 2, m); });
        I.levels[2 * n]->multiply_rescale_range(*vn, 0, *yn, 0, T, ab, 0, stream);    // a = v y_n
        I.levels[2 * n]->multiply_rescale_range(*yn, 0, *yn, 0, T, ab, T, stream);    // b = y_n y_n
        Ciphertext* out = n + 1 == K ? &y : &grow_scratch(I.y_at[n], T, [&](size_t m) { return new Ciphertext(*I.ctx[2 * n + 2], 2, m); });
        // y_{n+1} = round((w_n y_n - a b) / q_b): y_n is read where it lives, one limb above this level
        I.levels[2 * n + 1]->multiply_lincomb_rescale_range(ab, 0, ab, T, T, *I.weights[n], {LincombTerm{yn, 0}}, *out, 0, stream);
        yn = out;
    }
    y.set_ntt(false);
}

}  // namespace fhe
}  // namespace deeppowers
