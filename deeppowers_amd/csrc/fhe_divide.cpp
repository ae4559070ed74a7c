// fhe_divide.cpp - the facade's slot-wise division of the approximate (CKKS-style) family (ApproxDivide): Goldschmidt steps F = 2 - D; n_j <- n_j F; D <- D F,
// one level each - all T + 1 products of a group in ONE HybridKeySwitcher::multiply_complement_rescale_range, whose factor is never written -, the scale rule
// and the error bound of include/deeppowers/fhe.hpp.  Part of libdpfhe_api.so.
#include <algorithm>
#include <cmath>

#include "fhe_internal.h"

namespace deeppowers {
namespace fhe {

using namespace detail;

namespace {

struct DivideScales {
    std::vector<double> sigma, nu;   // sigma_0 .. sigma_K, nu_0 .. nu_K
    std::vector<int64_t> kappa;      // kappa_0 .. kappa_{K-1}
};

bool good_scale(double s) { return std::isfinite(s) && s >= std::ldexp(1.0, 20) && s < std::ldexp(1.0, 62); }

// the header's rule, in exactly its double operations; q[n] = the prime level n drops (K of them)
DivideScales divide_scales(const std::vector<uint64_t>& q, double num_scale, double den_scale) {
    if (q.empty()) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxDivide: one level per step, at least one step");
    if (!(std::isfinite(num_scale) && num_scale > 0) || !(std::isfinite(den_scale) && den_scale > 0))
        throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxDivide: scales must be finite and positive");
    DivideScales t;
    t.sigma.assign(1, den_scale);
    t.nu.assign(1, num_scale);
    for (size_t n = 0; n < q.size(); ++n) {
        if (!good_scale(t.sigma[n]) || !good_scale(t.nu[n])) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxDivide: a scale sigma_n or nu_n leaves [2^20, 2^62)");
        const double k = 2.0 * t.sigma[n];
        if (!(k < std::ldexp(1.0, 62))) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxDivide: a constant kappa_n reaches 2^62");
        t.kappa.push_back(std::llround(k));
        t.sigma.push_back((t.sigma[n] * t.sigma[n]) / (double)q[n]);
        t.nu.push_back((t.nu[n] * t.sigma[n]) / (double)q[n]);
    }
    if (!good_scale(t.sigma.back()) || !good_scale(t.nu.back())) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxDivide: a scale sigma_n or nu_n leaves [2^20, 2^62)");
    return t;
}

bool same_params(const FheParams& a, const FheParams& b) { return a.log2_n == b.log2_n && a.moduli == b.moduli && a.psi == b.psi; }

}  // namespace

class __attribute__((visibility("hidden"))) ApproxDivide::Impl {
public:
    std::vector<HybridKeySwitcher*> levels;
    std::vector<const Context*> ctx;     // level 0 .. K - 1: the key switchers' data contexts; ctx[K] = out_ctx
    std::vector<uint64_t> special;       // P of every level
    DivideScales sc;
    std::vector<std::unique_ptr<ComplementConstant>> kappa;   // per step, on ctx[n]: one upload at construction
    size_t K = 0;
    std::vector<std::unique_ptr<Ciphertext>> at;              // scratch, grown for a larger batch: the iterates (numerators | denominators) at level n, 1 <= n < K
    size_t ct_words(size_t level) const { return 2 * ctx[level]->params().n_limbs() * ctx[level]->params().n(); }
};

ApproxDivide::ApproxDivide(const std::vector<HybridKeySwitcher*>& levels, const Context& out_ctx, double num_scale, double den_scale) : impl_(new Impl) {
    Impl& I = *impl_;
    if (levels.empty()) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxDivide: one level per step, at least one step");
    I.levels = levels; I.K = levels.size();
    for (HybridKeySwitcher* ks : levels) {
        if (!ks) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxDivide: null key switcher");
        I.ctx.push_back(&ks->data_context());
        I.special.push_back(ks->extended_context().params().moduli.back());
    }
    I.ctx.push_back(&out_ctx);
    for (size_t r = 0; r + 1 < I.ctx.size(); ++r)
        if (I.ctx[r]->params().n_limbs() < 2 || !same_params(I.ctx[r + 1]->params(), I.ctx[r]->params().drop_last_limb()) || I.ctx[r + 1]->device_id() != I.ctx[0]->device_id())
            throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxDivide: every level's context (and out_ctx after the last) must be the one before it without its last limb, on the same device");
    std::vector<uint64_t> drop;
    for (size_t r = 0; r < I.K; ++r) drop.push_back(I.ctx[r]->params().moduli.back());
    I.sc = divide_scales(drop, num_scale, den_scale);
    for (size_t n = 0; n < I.K; ++n) I.kappa.emplace_back(new ComplementConstant(*I.ctx[n], I.sc.kappa[n]));
    I.at.resize(I.K);
}
ApproxDivide::~ApproxDivide() = default;

size_t ApproxDivide::iterations() const { return impl_->K; }
size_t ApproxDivide::depth() const { return impl_->K; }
double ApproxDivide::den_scale(size_t n) const {
    if (n > impl_->K) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxDivide::den_scale: n <= iterations");
    return impl_->sc.sigma[n];
}
double ApproxDivide::num_scale(size_t n) const {
    if (n > impl_->K) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxDivide::num_scale: n <= iterations");
    return impl_->sc.nu[n];
}
int64_t ApproxDivide::kappa(size_t n) const {
    if (n >= impl_->K) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxDivide::kappa: n < iterations");
    return impl_->sc.kappa[n];
}

double ApproxDivide::guess(double lo, double hi) {
    if (!(std::isfinite(lo) && std::isfinite(hi) && lo > 0 && hi >= lo)) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxDivide::guess: 0 < lo <= hi");
    return 2.0 / (lo + hi);
}
double ApproxDivide::residual(double lo, double hi, size_t K) {
    if (!(std::isfinite(lo) && std::isfinite(hi) && lo > 0 && hi >= lo)) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxDivide::residual: 0 < lo <= hi");
    double r = (hi - lo) / (hi + lo);
    for (size_t n = 0; n < K; ++n) r = r * r;
    return r;
}

double ApproxDivide::error_bound(uint32_t log2_n, const std::vector<uint64_t>& data_moduli, const std::vector<uint64_t>& special_primes, double num_scale,
                                 double den_scale, double Dm, double X, double Bd, double Bn) {
    const size_t K = special_primes.size(), L0 = data_moduli.size();
    if (K == 0) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxDivide::error_bound: one special prime per step");
    if (L0 < K + 1) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxDivide::error_bound: the input level needs K + 1 limbs");
    if (!(Dm >= 0) || !(X >= 0) || !(Bd >= 0) || !(Bn >= 0)) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxDivide::error_bound: magnitudes and noise bounds must be non-negative");
    const BoundUnits bu(log2_n);
    const double N = bu.N, H = bu.H, u = bu.u, u8 = bu.u8;
    const LevelLadder ladder = level_ladder(data_moduli, special_primes, N);
    const DivideScales sc = divide_scales(ladder.drop, num_scale, den_scale);
    if (!(Dm <= 2)) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxDivide::error_bound: every D_n lies in [0, 2] (max_abs_den <= 2), or the iteration diverges");
    const double Fm = 2;
    double E = N * Bd, G = N * Bn, Psi = 0, Phi = 0;   // the slot errors of D_n's and the numerators' phases; the float64 iteration's own distances from the real one
    for (size_t n = 0; n < K; ++n) {
        const double q = (double)ladder.drop[n], sg = sc.sigma[n], nu = sc.nu[n], f = E + 0.5, relin = N * (ladder.K[n] + H);
        const double G1 = (nu * X * f + sg * Fm * G + G * f + relin) / q + N * H + 4 * u * sc.nu[n + 1] * X;
        const double E1 = (sg * (Dm * f + Fm * E) + E * f + relin) / q + N * H + 4 * u * sc.sigma[n + 1] * Dm;
        const double Phi1 = Fm * Phi + X * Psi + 4 * u * X * Fm, Psi1 = (Fm + Dm) * Psi + 4 * u * Dm * Fm;
        E = E1; G = G1; Phi = Phi1; Psi = Psi1;
    }
    const double pre = G / sc.nu.back();
    return pre + u8 * N * (X + pre) + Phi;
}

double ApproxDivide::error_bound(double Dm, double X, double Bd, double Bn) const {
    const Impl& I = *impl_;
    return error_bound(I.ctx[0]->params().log2_n, I.ctx[0]->params().moduli, I.special, I.sc.nu[0], I.sc.sigma[0], Dm, X, Bd, Bn);
}

void ApproxDivide::apply(const Ciphertext& num, const Ciphertext& den, Ciphertext& y, Stream* stream) const {
    Impl& I = *impl_;
    const size_t G = den.batch(), K = I.K, GT = num.batch();
    auto on_level0 = [&](const Ciphertext& c) { return !c.is_ntt() && c.size() == 2 && c.words() == c.batch() * I.ct_words(0); };
    if (!on_level0(num) || !on_level0(den) || G == 0 || GT == 0 || GT % G || y.size() != 2 || y.batch() != GT || y.words() != GT * I.ct_words(K))
        throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxDivide::apply: num G T and den G 2-component coefficient-domain ciphertexts on the input context (G, T >= 1), y G T on out_ctx");
    const size_t T = GT / G;
    const Ciphertext *a = &num, *b = &den;
    size_t b_first = 0;
    for (size_t n = 0; n < K; ++n) {
        const bool last = n + 1 == K;
        // the step's output is the next step's input as it stands: the G T numerators, then - unless this is the last step - the G denominators
        Ciphertext* out = last ? &y : &grow_scratch(I.at[n], GT + G, [&](size_t m) { return new Ciphertext(*I.ctx[n + 1], 2, m); });
        I.levels[n]->multiply_complement_rescale_range(*a, 0, *b, b_first, G, T, !last, *I.kappa[n], *out, 0, stream);
        a = b = out;
        b_first = GT;
    }
    y.set_ntt(false);
}

}  // namespace fhe
}  // namespace deeppowers
