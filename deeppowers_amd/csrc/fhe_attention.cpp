// fhe_attention.cpp - the facade's attention scores of the approximate (CKKS-style) family (ApproxAttentionScores): s_ij = post_factor <q_i, k_j> for all pairs
// of encrypted queries and keys - one all-pairs product step (HybridKeySwitcher::multiply_outer_rescale_range), one rotate-and-add ladder over all pairs on the
// next level (SlotSum's elements) -, the scale rule and the error bound of include/deeppowers/fhe.hpp.  Part of libdpfhe_api.so.
#include <cmath>

#include "fhe_internal.h"

namespace deeppowers {
namespace fhe {

using namespace detail;

class __attribute__((visibility("hidden"))) ApproxAttentionScores::Impl {
public:
    HybridKeySwitcher *ks = nullptr, *ks_next = nullptr;
    std::unique_ptr<SlotSum> sum;
    size_t tokens = 0;
    bool causal = false;
    double q_scale = 0, k_scale = 0, post = 0;
    std::unique_ptr<Ciphertext> products;   // the product step's pairs, before the ladder
};

ApproxAttentionScores::ApproxAttentionScores(HybridKeySwitcher& ks, HybridKeySwitcher& ks_next, size_t tokens, size_t block, size_t stride, bool causal, double q_scale,
                                             double k_scale, double post_factor)
    : impl_(new Impl) {
    auto good = [](double v) { return std::isfinite(v) && v > 0; };
    if (tokens == 0) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxAttentionScores: at least one token");
    if (!good(q_scale) || !good(k_scale) || !good(post_factor)) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxAttentionScores: scales and post_factor must be finite and positive");
    const FheParams& pd = ks.data_context().params();
    if (pd.n_limbs() < 2) throw Exception(ErrorCode::INVALID_STATE, "ApproxAttentionScores: no data limb left to drop");
    const FheParams next = pd.drop_last_limb();
    const FheParams& pn = ks_next.data_context().params();
    if (pn.log2_n != next.log2_n || pn.moduli != next.moduli || ks_next.data_context().device_id() != ks.data_context().device_id())
        throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxAttentionScores: ks_next must be the key switcher of ks's next level");
    impl_->sum.reset(new SlotSum(ks_next, block, stride));   // (INVALID_ARGUMENT for a bad block or stride)
    impl_->ks = &ks;
    impl_->ks_next = &ks_next;
    impl_->tokens = tokens;
    impl_->causal = causal;
    impl_->q_scale = q_scale;
    impl_->k_scale = k_scale;
    impl_->post = post_factor;
    impl_->products.reset(new Ciphertext(ks_next.data_context(), 2, pairs()));
}
ApproxAttentionScores::~ApproxAttentionScores() = default;

size_t ApproxAttentionScores::tokens() const { return impl_->tokens; }
size_t ApproxAttentionScores::pairs() const { return impl_->causal ? impl_->tokens * (impl_->tokens + 1) / 2 : impl_->tokens * impl_->tokens; }
bool ApproxAttentionScores::causal() const { return impl_->causal; }
double ApproxAttentionScores::output_scale() const {
    return (impl_->q_scale * impl_->k_scale) / (double)impl_->ks->data_context().params().moduli.back() / impl_->post;
}

double ApproxAttentionScores::error_bound(uint32_t log2_n, const std::vector<uint64_t>& data_moduli, uint64_t special_prime, size_t block, double q_scale, double k_scale,
                                          double post_factor, double A, double B, double Bq, double Bk) {
    if (data_moduli.size() < 2 || !(post_factor > 0)) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxAttentionScores::error_bound: two data limbs and a positive post_factor at least");
    const double S = (q_scale * k_scale) / (double)data_moduli.back(), u = BoundUnits(log2_n).u;
    const double e1 = ApproxProductSum::error_bound(log2_n, data_moduli, special_prime, 1, q_scale, k_scale, A, B, Bq, Bk);
    const std::vector<uint64_t> next(data_moduli.begin(), data_moduli.end() - 1);
    return post_factor * (SlotSum::error_bound(log2_n, next, special_prime, block, S, A * B, S * e1) + 4 * u * (double)block * A * B);
}
double ApproxAttentionScores::error_bound(double A, double B, double Bq, double Bk) const {
    const FheParams& pe = impl_->ks->extended_context().params();
    return error_bound(pe.log2_n, std::vector<uint64_t>(pe.moduli.begin(), pe.moduli.end() - 1), pe.moduli.back(), impl_->sum->block(), impl_->q_scale, impl_->k_scale,
                       impl_->post, A, B, Bq, Bk);
}

void ApproxAttentionScores::apply(const Ciphertext& q, const Ciphertext& k, Ciphertext& scores, Stream* stream) const {
    const size_t T = impl_->tokens, P = pairs();
    if (q.batch() != T || k.batch() != T || scores.batch() != P)
        throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxAttentionScores::apply: `tokens` queries and keys, pairs() scores");
    impl_->ks->multiply_outer_rescale_range(q, 0, T, k, 0, T, impl_->causal, *impl_->products, 0, stream);
    impl_->ks_next->rotate_add_range(*impl_->products, 0, P, impl_->sum->galois_elements(), scores, 0, stream);
}

}  // namespace fhe
}  // namespace deeppowers
