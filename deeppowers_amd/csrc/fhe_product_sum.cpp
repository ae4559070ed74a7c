// fhe_product_sum.cpp - the facade's slot-wise sum of products of the approximate (CKKS-style) family (ApproxProductSum): y_g = sum_k a_{g,k} b_{g,k} under ONE
// key switch and one rescale per group (HybridKeySwitcher::multiply_sum_rescale_range), the scale rule and the error bound of include/deeppowers/fhe.hpp.
// Part of libdpfhe_api.so.
#include <algorithm>
#include <cmath>

#include "fhe_internal.h"

namespace deeppowers {
namespace fhe {

using namespace detail;

class __attribute__((visibility("hidden"))) ApproxProductSum::Impl {
public:
    HybridKeySwitcher* ks = nullptr;
    size_t terms = 0;
    bool b_shared = false;
    double a_scale = 0, b_scale = 0;
};

ApproxProductSum::ApproxProductSum(HybridKeySwitcher& ks, size_t terms, bool b_shared, double a_scale, double b_scale) : impl_(new Impl) {
    if (terms == 0) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxProductSum: at least one term");
    if (!(std::isfinite(a_scale) && a_scale > 0) || !(std::isfinite(b_scale) && b_scale > 0))
        throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxProductSum: scales must be finite and positive");
    if (ks.data_context().params().n_limbs() < 2) throw Exception(ErrorCode::INVALID_STATE, "ApproxProductSum: no data limb left to drop");
    impl_->ks = &ks;
    impl_->terms = terms;
    impl_->b_shared = b_shared;
    impl_->a_scale = a_scale;
    impl_->b_scale = b_scale;
}
ApproxProductSum::~ApproxProductSum() = default;

size_t ApproxProductSum::terms() const { return impl_->terms; }
bool ApproxProductSum::b_shared() const { return impl_->b_shared; }
double ApproxProductSum::output_scale() const { return (impl_->a_scale * impl_->b_scale) / (double)impl_->ks->data_context().params().moduli.back(); }

double ApproxProductSum::error_bound(uint32_t log2_n, const std::vector<uint64_t>& data_moduli, uint64_t special_prime, size_t terms, double a_scale, double b_scale,
                                     double A, double B, double Ba, double Bb) {
    if (data_moduli.size() < 2 || !special_prime || terms == 0) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxProductSum::error_bound: two data limbs, a special prime, one term at least");
    if (!(A >= 0) || !(B >= 0) || !(Ba >= 0) || !(Bb >= 0)) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxProductSum::error_bound: magnitudes and noise bounds must be non-negative");
    const BoundUnits bu(log2_n);
    const double N = bu.N, H = bu.H, u = bu.u, u8 = bu.u8, K = (double)terms;
    const double Kr = keyswitch_term((double)data_moduli.size(), N, max_modulus(data_moduli, data_moduli.size()), special_prime), q = (double)data_moduli.back();
    const double S = (a_scale * b_scale) / q, Da = N * Ba, Db = N * Bb, Y = K * A * B;
    const double E = (K * (a_scale * A * Db + b_scale * B * Da + Da * Db) + N * (Kr + H)) / q + N * H + 4 * u * S * Y;
    const double pre = E / S, F = 2 * K * u * Y;
    return pre + u8 * N * (Y + pre) + F;
}
double ApproxProductSum::error_bound(double A, double B, double Ba, double Bb) const {
    const FheParams& pe = impl_->ks->extended_context().params();
    return error_bound(pe.log2_n, std::vector<uint64_t>(pe.moduli.begin(), pe.moduli.end() - 1), pe.moduli.back(), impl_->terms, impl_->a_scale, impl_->b_scale, A, B, Ba, Bb);
}

void ApproxProductSum::apply(const Ciphertext& a, const Ciphertext& b, Ciphertext& y, Stream* stream) const {
    const size_t K = impl_->terms, groups = y.batch();
    if (a.batch() != groups * K || b.batch() != (impl_->b_shared ? K : groups * K))
        throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxProductSum::apply: y holds G items, a holds G * terms, b as many or (shared) terms");
    impl_->ks->multiply_sum_rescale_range(a, 0, b, 0, impl_->b_shared, groups, K, y, 0, stream);
}

}  // namespace fhe
}  // namespace deeppowers
