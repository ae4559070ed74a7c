// fhe_keyswitch.cpp - the facade's hybrid key switcher (one special prime P): relinearisation and Galois keys on the extended context Q P and the
// rotations built on them.  Part of libdpfhe_api.so (fhe_api.cpp names the other units); its keys are made by fhe_keys.cpp's make_switch_key.
#include <algorithm>
#include <cmath>

#include "fhe_internal.h"
#include "fhe_sampler.h"

namespace deeppowers {
namespace fhe {

using namespace detail;

namespace {

// One product step, behind the four multiply_*_rescale_range methods: the tensor products of groups x terms pairs summed per group, ONE key switch per group
// and a last pass that rescales - with `weights`, after combining with their addends and constant.  The single product (`sum` false: terms = 1, b not
// shared) keeps dpfhe_ct_mul, whose fused kernel dpfhe_ct_mul_sum does not run.  `what` and the wording `sum` picks are the public method's own.
struct ProductStep {
    const char* what;
    bool sum;
    size_t groups, terms;
    bool b_shared;
    const ScalarWeights* weights;                 // null: relinearise and rescale, nothing combined
    const std::vector<LincombTerm>* addends;      // one per weight
};

}  // namespace

// ---- HybridKeySwitcher ---------------------------------------------------------------------------------------------------
class __attribute__((visibility("hidden"))) HybridKeySwitcher::Impl {   // (hidden like the Sampler it holds)
public:
    const Context* data_ctx = nullptr;
    std::unique_ptr<Context> ext;
    std::unique_ptr<SecretKey> sk_ext;
    std::unique_ptr<PolyBuffer> relin;                       // [Ld][2][L][N]
    std::vector<std::pair<uint32_t, std::unique_ptr<PolyBuffer>>> galois;
    std::vector<std::pair<std::vector<uint32_t>, std::unique_ptr<PolyBuffer>>> packed;   // element list -> its keys back to back
    std::unique_ptr<PolyBuffer> scratch_work;      // batched rotations: reused across calls (one caller at a time per switcher)
    std::unique_ptr<Ciphertext> scratch_rotated;
    std::unique_ptr<Ciphertext> scratch_acc;       // rotate-and-add ladders: the ping-pong partner of the output
    std::unique_ptr<PolyBuffer> scratch_digits;    // hoisted rotations: NTT of the lifted digits, [Ld][L][N]
    std::unique_ptr<Ciphertext> scratch_in_ntt;    // rotate_hoisted_qp: NTT of the inputs on the data limbs
    std::unique_ptr<Ciphertext> scratch_product;   // multiply_rescale: the 3-component product on the data limbs
    void init(const Context& data, const SecretKey& sk, uint64_t special_prime, uint64_t special_psi) {
        data_ctx = &data;
        FheParams pe = data.params();
        pe.moduli.push_back(special_prime);
        pe.psi.push_back(special_psi);
        ext.reset(new Context(pe, data.device_id()));
        sk_ext.reset(new SecretKey(*ext, sk.coefficients()));
        p_special = special_prime;
        relin.reset(new PolyBuffer(*ext, pe.n_limbs() - 1, 2, true));
        make_key(sk_ext->ntt_squared(), *relin);
    }
    const PolyBuffer* find_key(uint32_t g) const {   // null: the element was never added
        for (auto& kv : galois) if (kv.first == g) return kv.second.get();
        return nullptr;
    }
    // the keys of an element list, packed back to back once and cached
    const PolyBuffer* packed_keys(const std::vector<uint32_t>& elts, Stream* s = nullptr) {
        for (auto& kv : packed) if (kv.first == elts) return kv.second.get();
        const FheParams& pe = ext->params();
        const size_t L = pe.n_limbs(), Ld = L - 1, key_words = Ld * 2 * L * pe.n();
        std::unique_ptr<PolyBuffer> buf(new PolyBuffer(*ext, elts.size() * Ld, 2, true));
        for (size_t i = 0; i < elts.size(); ++i) {
            const PolyBuffer* key = find_key(elts[i]);
            if (!key) throw Exception(ErrorCode::INVALID_STATE, "HybridKeySwitcher: no key for an element (add_galois_element first)");
            // on the caller's stream: a blocking null-stream copy would not order against work on a non-blocking stream
            hip_check(hipMemcpyAsync(buf->data() + i * key_words, key->data(), key_words * sizeof(uint64_t), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(s)),
                      "hipMemcpyAsync D2D");
        }
        // The pack is cached and handed to LATER callers on ANY stream: it happens once per element list, so the copies are simply waited for
        // here - nothing orders another stream's kernels against an asynchronous copy they never saw being enqueued.
        hip_check(hipStreamSynchronize(static_cast<hipStream_t>(s)), "hipStreamSynchronize (key pack)");
        packed.emplace_back(elts, std::move(buf));
        return packed.back().second.get();
    }
    void ensure_scratch(size_t k) {
        grow_scratch(scratch_work, k, [&](size_t b) { return new PolyBuffer(*ext, b, 2, false); });
        grow_scratch(scratch_rotated, k, [&](size_t b) { return new Ciphertext(*data_ctx, 2, b); });
    }
    void ensure_digits(size_t polys) { grow_scratch(scratch_digits, polys, [&](size_t b) { return new PolyBuffer(*ext, b, 1, true); }); }
    Sampler rng;
    uint64_t p_special = 0;

    void product_step(const ProductStep& st, const Ciphertext& a, size_t a_first, const Ciphertext& b, size_t b_first, Ciphertext& out, size_t out_first, Stream* s) {
        const std::string what = st.what;
        const FheParams& pd = data_ctx->params();
        const size_t Ld = pd.n_limbs(), n = pd.n(), in_words = 2 * Ld * n, out_words = 2 * (Ld - 1) * n, groups = st.groups;
        if (Ld < 2) throw Exception(ErrorCode::INVALID_STATE, what + ": no data limb left to drop");
        if (st.terms == 0) throw Exception(ErrorCode::INVALID_ARGUMENT, what + ": at least one term");
        const size_t a_count = groups * st.terms, b_count = st.b_shared ? st.terms : a_count;
        if (a.is_ntt() || b.is_ntt() || a.size() != 2 || b.size() != 2 || a.words() != a.batch() * in_words || b.words() != b.batch() * in_words ||
            a_first + a_count > a.batch() || b_first + b_count > b.batch())
            throw Exception(ErrorCode::INVALID_ARGUMENT, what + ": 2-component coefficient-domain ciphertexts on the data context, " +
                                                             (st.sum ? "groups * terms items of a, as many or (shared) terms items of b" : "ranges inside them"));
        if (out.size() != 2 || out.words() != out.batch() * out_words || out_first + groups > out.batch())
            throw Exception(ErrorCode::INVALID_ARGUMENT, what + ": output must live on the next-level context (Ld - 1 limbs), 2 components, with room for " +
                                                             (st.sum ? "one item per group" : "the range"));
        const uint64_t* ptrs[15] = {};   // the addends where they live, and how many limbs their contexts have (ScalarWeights holds at most 15)
        uint32_t limbs[15] = {};
        if (st.weights) {
            const std::string noun = st.sum ? "addend" : "term", a_noun = st.sum ? "an addend" : "a term";
            const FheParams& pw = st.weights->context().params();
            if (st.weights->terms() != st.addends->size() || pw.log2_n != pd.log2_n || pw.moduli != pd.moduli || st.weights->context().device_id() != data_ctx->device_id())
                throw Exception(ErrorCode::INVALID_ARGUMENT, what + ": weights built on the data context, one per " + noun);
            for (size_t k = 0; k < st.addends->size(); ++k) {
                const LincombTerm& t = (*st.addends)[k];
                if (!t.ct) throw Exception(ErrorCode::INVALID_ARGUMENT, what + ": null " + noun);
                const FheParams& pz = t.ct->context().params();
                const size_t Lz = pz.n_limbs();
                if (t.ct->is_ntt() || t.ct->size() != 2 || pz.log2_n != pd.log2_n || Lz < Ld || !std::equal(pd.moduli.begin(), pd.moduli.end(), pz.moduli.begin()) ||
                    t.ct->words() != t.ct->batch() * 2 * Lz * n || t.first + groups > t.ct->batch() || t.ct->context().device_id() != data_ctx->device_id())
                    throw Exception(ErrorCode::INVALID_ARGUMENT, what + ": " + a_noun + " is 2 components, coefficient domain, on a context whose first limbs are the data context's, range inside it");
                ptrs[k] = t.ct->data() + t.first * 2 * Lz * n;
                limbs[k] = (uint32_t)Lz;
            }
        }
        if (groups == 0) return;
        grow_scratch(scratch_product, groups, [&](size_t m) { return new Ciphertext(*data_ctx, 3, m); });
        grow_scratch(scratch_work, groups, [&](size_t m) { return new PolyBuffer(*ext, m, 2, false); });
        const uint64_t *pa = a.data() + a_first * in_words, *pb = b.data() + b_first * in_words;
        if (st.sum) check(dpfhe_ct_mul_sum(handle_of(*data_ctx), scratch_product->data(), pa, pb, groups, st.terms, st.b_shared ? 1 : groups, 0, s), "dpfhe_ct_mul_sum");
        else check(dpfhe_ct_mul(handle_of(*data_ctx), scratch_product->data(), pa, pb, groups, 0, s), "dpfhe_ct_mul");
        uint64_t* po = out.data() + out_first * out_words;
        if (st.weights)
            check(dpfhe_relinearize_lincomb_rescale_hybrid(handle_of(*ext), po, scratch_product->data(), relin->data(), scratch_work->data(), ptrs, limbs, st.addends->size(),
                                                           st.weights->data(), groups, s),
                  "dpfhe_relinearize_lincomb_rescale_hybrid");
        else
            check(dpfhe_relinearize_rescale_hybrid(handle_of(*ext), po, scratch_product->data(), relin->data(), scratch_work->data(), groups, s), "dpfhe_relinearize_rescale_hybrid");
        out.set_ntt(false);
    }

    // target (NTT domain on ext, all limbs) scaled by P limb-wise: P mod q_i for data limbs, 0 for the P limb
    void make_key(const uint64_t* d_target_ntt_ext, PolyBuffer& out) {
        const FheParams& pe = ext->params();
        const size_t n = pe.n(), L = pe.n_limbs();
        std::vector<uint64_t> host(L * n);
        hip_check(hipMemcpy(host.data(), d_target_ntt_ext, L * n * sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy D2H");
        for (size_t l = 0; l < L; ++l) {
            const uint64_t q = pe.moduli[l], f = p_special % q;   // 0 on the special limb itself
            for (size_t k = 0; k < n; ++k) host[l * n + k] = (uint64_t)((u128)host[l * n + k] * f % q);
        }
        PolyBuffer scaled(*ext, 1, 1, true);
        scaled.copy_from_host(host.data());
        make_switch_key(*ext, *sk_ext, rng, scaled.data(), out, L - 1, nullptr);
    }
};

HybridKeySwitcher::HybridKeySwitcher(const Context& data_ctx, const SecretKey& sk, uint64_t special_prime, uint64_t special_psi) : impl_(new Impl) {
    impl_->init(data_ctx, sk, special_prime, special_psi);
}
HybridKeySwitcher::HybridKeySwitcher(const Context& data_ctx, const SecretKey& sk, uint64_t special_prime, uint64_t special_psi, TestSeed seed) : impl_(new Impl) {
    impl_->rng = Sampler(seed);
    impl_->init(data_ctx, sk, special_prime, special_psi);
}
HybridKeySwitcher::~HybridKeySwitcher() = default;

void HybridKeySwitcher::add_galois_element(uint32_t g) {
    const FheParams& pe = impl_->ext->params();
    const size_t n = pe.n(), L = pe.n_limbs();
    if (!(g & 1u) || g >= 2 * n) throw Exception(ErrorCode::INVALID_ARGUMENT, "add_galois_element: element must be odd and < 2N");
    if (impl_->find_key(g)) return;
    PolyBuffer target = galois_target_ntt(*impl_->ext, impl_->sk_ext->coefficients(), g);
    std::unique_ptr<PolyBuffer> key(new PolyBuffer(*impl_->ext, L - 1, 2, true));
    impl_->make_key(target.data(), *key);
    impl_->galois.emplace_back(g, std::move(key));
}

const PolyBuffer& HybridKeySwitcher::galois_key(uint32_t g) const {
    const PolyBuffer* key = impl_->find_key(g);
    if (!key) throw Exception(ErrorCode::INVALID_STATE, "HybridKeySwitcher::galois_key: no key for this element (add_galois_element first)");
    return *key;
}

void HybridKeySwitcher::relinearize(const Ciphertext& in3, Ciphertext& out2, Stream* s) const {
    if (in3.is_ntt() || in3.size() != 3 || out2.size() != 2 || out2.batch() != in3.batch())
        throw Exception(ErrorCode::INVALID_ARGUMENT, "HybridKeySwitcher::relinearize: 3-component coefficient-domain input, 2-component output");
    PolyBuffer work(*impl_->ext, in3.batch(), 2, false);
    check(dpfhe_relinearize_hybrid(handle_of(*impl_->ext), out2.data(), in3.data(), impl_->relin->data(), work.data(), in3.batch(), s),
          "dpfhe_relinearize_hybrid");
    hip_check(hipStreamSynchronize(static_cast<hipStream_t>(s)), "hipStreamSynchronize");   // `work` is freed on return
    out2.set_ntt(false);
}

void HybridKeySwitcher::apply_galois(const Ciphertext& in2, uint32_t g, Ciphertext& out2, Stream* s) const {
    if (in2.is_ntt() || in2.size() != 2 || out2.size() != 2 || out2.batch() != in2.batch())
        throw Exception(ErrorCode::INVALID_ARGUMENT, "HybridKeySwitcher::apply_galois: 2-component coefficient-domain input and output");
    const PolyBuffer* key = impl_->find_key(g);
    if (!key) throw Exception(ErrorCode::INVALID_STATE, "HybridKeySwitcher::apply_galois: no key for this element (add_galois_element first)");
    Ciphertext rotated(*impl_->data_ctx, 2, in2.batch());
    PolyBuffer work(*impl_->ext, in2.batch(), 2, false);
    check(dpfhe_apply_galois(handle_of(*impl_->data_ctx), rotated.data(), in2.data(), in2.batch() * 2, g, s), "dpfhe_apply_galois");
    check(dpfhe_switch_key_hybrid(handle_of(*impl_->ext), out2.data(), rotated.data(), key->data(), work.data(), in2.batch(), s),
          "dpfhe_switch_key_hybrid");
    hip_check(hipStreamSynchronize(static_cast<hipStream_t>(s)), "hipStreamSynchronize");
    out2.set_ntt(false);
}

void HybridKeySwitcher::apply_galois_many(const Ciphertext& in2, const std::vector<uint32_t>& elts, Ciphertext& out2, size_t out_first, Stream* s) const {
    if (in2.batch() != 1 && in2.batch() != elts.size())
        throw Exception(ErrorCode::INVALID_ARGUMENT, "HybridKeySwitcher::apply_galois_many: input of 1 or k items, output with room for k items");
    apply_galois_range(in2, 0, in2.batch() == 1 && elts.size() != 1, elts, out2, out_first, s);
}

void HybridKeySwitcher::apply_galois_range(const Ciphertext& in2, size_t in_first, bool broadcast, const std::vector<uint32_t>& elts, Ciphertext& out2,
                                           size_t out_first, Stream* s) const {
    const size_t k = elts.size();
    if (k == 0) return;
    if (in2.is_ntt() || in2.size() != 2 || out2.size() != 2 || in_first + (broadcast ? 1 : k) > in2.batch() || out_first + k > out2.batch())
        throw Exception(ErrorCode::INVALID_ARGUMENT, "HybridKeySwitcher::apply_galois_range: input range of 1 (broadcast) or k items, output with room for k items");
    const FheParams& pe = impl_->ext->params();
    const size_t L = pe.n_limbs(), Ld = L - 1, n = pe.n(), ct_words = 2 * Ld * n;
    const PolyBuffer* keys = impl_->packed_keys(elts, s);
    impl_->ensure_scratch(k);   // kept for the next call: no allocation and no host synchronisation on the steady path
    check(dpfhe_rotate_hybrid_batch(handle_of(*impl_->ext), out2.data() + out_first * ct_words, in2.data() + in_first * ct_words,
                                    broadcast ? 1 : k, elts.data(), keys->data(), impl_->scratch_work->data(), impl_->scratch_rotated->data(), k, s),
          "dpfhe_rotate_hybrid_batch");
    out2.set_ntt(false);
}

void HybridKeySwitcher::apply_galois_hoisted(const Ciphertext& in2, size_t in_first, size_t n_items, const std::vector<uint32_t>& elts, Ciphertext& out2,
                                             size_t out_first, Stream* s) const {
    const size_t k = elts.size();
    if (k == 0 || n_items == 0) return;
    if (in2.is_ntt() || in2.size() != 2 || out2.size() != 2 || in_first + n_items > in2.batch() || out_first + k * n_items > out2.batch())
        throw Exception(ErrorCode::INVALID_ARGUMENT, "HybridKeySwitcher::apply_galois_hoisted: n_items input items, output with room for k * n_items items");
    const FheParams& pe = impl_->ext->params();
    const size_t L = pe.n_limbs(), Ld = L - 1, n = pe.n(), ct_words = 2 * Ld * n;
    const PolyBuffer* keys = impl_->packed_keys(elts, s);
    impl_->ensure_scratch(k * n_items);
    impl_->ensure_digits(n_items * Ld);
    check(dpfhe_rotate_hybrid_hoisted(handle_of(*impl_->ext), out2.data() + out_first * ct_words, in2.data() + in_first * ct_words, n_items,
                                      elts.data(), keys->data(), impl_->scratch_work->data(), impl_->scratch_rotated->data(), impl_->scratch_digits->data(), k, s),
          "dpfhe_rotate_hybrid_hoisted");
    out2.set_ntt(false);
}

void HybridKeySwitcher::apply_galois_grouped(const Ciphertext& in2, size_t in_first, const std::vector<uint32_t>& elts, size_t group, Ciphertext& out2,
                                             size_t out_first, Stream* s) const {
    const size_t k = elts.size(), batch = k * group;
    if (batch == 0) return;
    if (in2.is_ntt() || in2.size() != 2 || out2.size() != 2 || in_first + batch > in2.batch() || out_first + batch > out2.batch())
        throw Exception(ErrorCode::INVALID_ARGUMENT, "HybridKeySwitcher::apply_galois_grouped: k * group items in and out");
    const FheParams& pe = impl_->ext->params();
    const size_t Ld = pe.n_limbs() - 1, n = pe.n(), ct_words = 2 * Ld * n;
    const PolyBuffer* keys = impl_->packed_keys(elts, s);
    impl_->ensure_scratch(batch);
    check(dpfhe_rotate_hybrid_grouped(handle_of(*impl_->ext), out2.data() + out_first * ct_words, in2.data() + in_first * ct_words, elts.data(), k,
                                      group, keys->data(), impl_->scratch_work->data(), impl_->scratch_rotated->data(), s),
          "dpfhe_rotate_hybrid_grouped");
    out2.set_ntt(false);
}

void HybridKeySwitcher::rotate_add_range(const Ciphertext& in2, size_t in_first, size_t count, const std::vector<uint32_t>& elts, Ciphertext& out2, size_t out_first,
                                         Stream* s) const {
    if (count == 0) return;
    const FheParams& pe = impl_->ext->params();
    const size_t Ld = pe.n_limbs() - 1, n = pe.n(), ct_words = 2 * Ld * n;
    if (elts.empty() || in2.is_ntt() || in2.size() != 2 || out2.size() != 2 || in2.words() != in2.batch() * ct_words || out2.words() != out2.batch() * ct_words ||
        in_first + count > in2.batch() || out_first + count > out2.batch())
        throw Exception(ErrorCode::INVALID_ARGUMENT, "HybridKeySwitcher::rotate_add_range: at least one element, count coefficient-domain items of the data context in and out");
    const PolyBuffer* keys = impl_->packed_keys(elts, s);
    grow_scratch(impl_->scratch_work, count, [&](size_t b) { return new PolyBuffer(*impl_->ext, b, 2, false); });
    if (elts.size() > 1) grow_scratch(impl_->scratch_acc, count, [&](size_t b) { return new Ciphertext(*impl_->data_ctx, 2, b); });
    check(dpfhe_rotate_add_hybrid(handle_of(*impl_->ext), out2.data() + out_first * ct_words, in2.data() + in_first * ct_words, elts.data(), keys->data(),
                                  impl_->scratch_work->data(), elts.size() > 1 ? impl_->scratch_acc->data() : nullptr, elts.size(), count, s),
          "dpfhe_rotate_add_hybrid");
    out2.set_ntt(false);
}

void HybridKeySwitcher::multiply_rescale(const Ciphertext& a, const Ciphertext& b, Ciphertext& out_next_level, Stream* s) const {
    if (b.batch() != a.batch() || out_next_level.batch() != a.batch())
        throw Exception(ErrorCode::INVALID_ARGUMENT, "HybridKeySwitcher::multiply_rescale: operands and output of one batch");
    multiply_rescale_range(a, 0, b, 0, a.batch(), out_next_level, 0, s);
}

void HybridKeySwitcher::multiply_rescale_range(const Ciphertext& a, size_t a_first, const Ciphertext& b, size_t b_first, size_t count, Ciphertext& out,
                                               size_t out_first, Stream* s) const {
    impl_->product_step({"HybridKeySwitcher::multiply_rescale", false, count, 1, false, nullptr, nullptr}, a, a_first, b, b_first, out, out_first, s);
}

// ---- ScalarWeights ---------------------------------------------------------------------------------------------------------
class __attribute__((visibility("hidden"))) ScalarWeights::Impl {
public:
    const Context* ctx = nullptr;
    size_t K = 0;
    uint64_t* d_w = nullptr;   // [K + 2][Ld]
    ~Impl() { if (d_w) (void)hipFree(d_w); }
};

ScalarWeights::ScalarWeights(const Context& data_ctx, int64_t product_weight, const std::vector<int64_t>& term_weights, int64_t constant_at_output) : impl_(new Impl) {
    const FheParams& p = data_ctx.params();
    const size_t Ld = p.n_limbs(), K = term_weights.size();
    if (Ld < 2) throw Exception(ErrorCode::INVALID_STATE, "ScalarWeights: no data limb left to drop");
    if (K > 15) throw Exception(ErrorCode::INVALID_ARGUMENT, "ScalarWeights: at most 15 terms");
    std::vector<int64_t> rows{product_weight};
    rows.insert(rows.end(), term_weights.begin(), term_weights.end());
    rows.push_back(constant_at_output);
    const int64_t lim = (int64_t)1 << 62;
    for (int64_t v : rows)
        if (v <= -lim || v >= lim) throw Exception(ErrorCode::INVALID_ARGUMENT, "ScalarWeights: a weight |w| reaches 2^62");
    const std::vector<uint64_t> w = signed_weight_rows(p, rows, K + 1);   // the constant row: constant_at_output * q_last
    impl_->ctx = &data_ctx;
    impl_->K = K;
    impl_->d_w = device_alloc<uint64_t>(data_ctx.device_id(), w.size());
    hip_check(hipMemcpy(impl_->d_w, w.data(), w.size() * sizeof(uint64_t), hipMemcpyHostToDevice), "hipMemcpy H2D");
}
ScalarWeights::~ScalarWeights() = default;
size_t ScalarWeights::terms() const { return impl_->K; }
const Context& ScalarWeights::context() const { return *impl_->ctx; }
const uint64_t* ScalarWeights::data() const { return impl_->d_w; }

void HybridKeySwitcher::multiply_lincomb_rescale_range(const Ciphertext& a, size_t a_first, const Ciphertext& b, size_t b_first, size_t count, const ScalarWeights& weights,
                                                       const std::vector<LincombTerm>& terms, Ciphertext& out, size_t out_first, Stream* s) const {
    impl_->product_step({"HybridKeySwitcher::multiply_lincomb_rescale", false, count, 1, false, &weights, &terms}, a, a_first, b, b_first, out, out_first, s);
}

// ---- sums of products: the tensor products summed by dpfhe_ct_mul_sum into the object's scratch, ONE key switch and one rounding per group ----------------
void HybridKeySwitcher::multiply_sum_rescale_range(const Ciphertext& a, size_t a_first, const Ciphertext& b, size_t b_first, bool b_shared, size_t groups, size_t terms,
                                                   Ciphertext& out, size_t out_first, Stream* s) const {
    impl_->product_step({"HybridKeySwitcher::multiply_sum_rescale", true, groups, terms, b_shared, nullptr, nullptr}, a, a_first, b, b_first, out, out_first, s);
}

void HybridKeySwitcher::multiply_sum_lincomb_rescale_range(const Ciphertext& a, size_t a_first, const Ciphertext& b, size_t b_first, bool b_shared, size_t groups,
                                                           size_t terms, const ScalarWeights& weights, const std::vector<LincombTerm>& addends, Ciphertext& out,
                                                           size_t out_first, Stream* s) const {
    impl_->product_step({"HybridKeySwitcher::multiply_sum_lincomb_rescale", true, groups, terms, b_shared, &weights, &addends}, a, a_first, b, b_first, out, out_first, s);
}

// ---- products with a shared complement factor: dpfhe_ct_mul_complement into the object's scratch, one key switch and one rounding per product ----------------
class __attribute__((visibility("hidden"))) ComplementConstant::Impl {
public:
    const Context* ctx = nullptr;
    int64_t kappa = 0;
    uint64_t* d_kappa = nullptr;   // [Ld]
    ~Impl() { if (d_kappa) (void)hipFree(d_kappa); }
};

ComplementConstant::ComplementConstant(const Context& data_ctx, int64_t kappa) : impl_(new Impl) {
    if (kappa < 0 || kappa >= ((int64_t)1 << 62)) throw Exception(ErrorCode::INVALID_ARGUMENT, "ComplementConstant: kappa in [0, 2^62)");
    const std::vector<uint64_t> w = signed_weight_rows(data_ctx.params(), {kappa}, 1);   // (no constant row: kappa lives at the INPUT's scale)
    impl_->ctx = &data_ctx;
    impl_->kappa = kappa;
    impl_->d_kappa = device_alloc<uint64_t>(data_ctx.device_id(), w.size());
    hip_check(hipMemcpy(impl_->d_kappa, w.data(), w.size() * sizeof(uint64_t), hipMemcpyHostToDevice), "hipMemcpy H2D");
}
ComplementConstant::~ComplementConstant() = default;
int64_t ComplementConstant::value() const { return impl_->kappa; }
const Context& ComplementConstant::context() const { return *impl_->ctx; }
const uint64_t* ComplementConstant::data() const { return impl_->d_kappa; }

void HybridKeySwitcher::multiply_complement_rescale_range(const Ciphertext& a, size_t a_first, const Ciphertext& b, size_t b_first, size_t groups, size_t terms,
                                                          bool with_self, const ComplementConstant& kappa, Ciphertext& out, size_t out_first, Stream* s) const {
    const std::string what = "HybridKeySwitcher::multiply_complement_rescale";
    const Context& data = *impl_->data_ctx;
    const FheParams& pd = data.params();
    const size_t Ld = pd.n_limbs(), n = pd.n(), in_words = 2 * Ld * n, out_words = 2 * (Ld - 1) * n, items = groups * (terms + (with_self ? 1 : 0));
    if (Ld < 2) throw Exception(ErrorCode::INVALID_STATE, what + ": no data limb left to drop");
    if (terms == 0 && !with_self) throw Exception(ErrorCode::INVALID_ARGUMENT, what + ": at least one term, or the self product");
    if (a.is_ntt() || b.is_ntt() || a.size() != 2 || b.size() != 2 || a.words() != a.batch() * in_words || b.words() != b.batch() * in_words ||
        a_first + groups * terms > a.batch() || b_first + groups > b.batch())
        throw Exception(ErrorCode::INVALID_ARGUMENT, what + ": 2-component coefficient-domain ciphertexts on the data context, groups * terms items of a and groups items of b");
    if (out.size() != 2 || out.words() != out.batch() * out_words || out_first + items > out.batch())
        throw Exception(ErrorCode::INVALID_ARGUMENT, what + ": output must live on the next-level context (Ld - 1 limbs), 2 components, with room for groups * terms (+ groups) items");
    const FheParams& pk = kappa.context().params();
    if (pk.log2_n != pd.log2_n || pk.moduli != pd.moduli || kappa.context().device_id() != data.device_id())
        throw Exception(ErrorCode::INVALID_ARGUMENT, what + ": kappa built on the data context");
    if (groups == 0) return;
    grow_scratch(impl_->scratch_product, items, [&](size_t m) { return new Ciphertext(data, 3, m); });
    grow_scratch(impl_->scratch_work, items, [&](size_t m) { return new PolyBuffer(*impl_->ext, m, 2, false); });
    check(dpfhe_ct_mul_complement(handle_of(data), impl_->scratch_product->data(), a.data() + a_first * in_words, b.data() + b_first * in_words, kappa.data(), groups,
                                  terms, with_self ? 1 : 0, 0, s),
          "dpfhe_ct_mul_complement");
    check(dpfhe_relinearize_rescale_hybrid(handle_of(*impl_->ext), out.data() + out_first * out_words, impl_->scratch_product->data(), impl_->relin->data(),
                                           impl_->scratch_work->data(), items, s),
          "dpfhe_relinearize_rescale_hybrid");
    out.set_ntt(false);
}

// ---- all pairs of two item ranges: dpfhe_ct_mul_outer into the object's scratch, one key switch and one rounding per pair ----------------------------------
void HybridKeySwitcher::multiply_outer_rescale_range(const Ciphertext& a, size_t a_first, size_t a_count, const Ciphertext& b, size_t b_first, size_t b_count, bool causal,
                                                     Ciphertext& out, size_t out_first, Stream* s) const {
    const std::string what = "HybridKeySwitcher::multiply_outer_rescale";
    const Context& data = *impl_->data_ctx;
    const FheParams& pd = data.params();
    const size_t Ld = pd.n_limbs(), n = pd.n(), in_words = 2 * Ld * n, out_words = 2 * (Ld - 1) * n;
    if (Ld < 2) throw Exception(ErrorCode::INVALID_STATE, what + ": no data limb left to drop");
    if (causal && a_count != b_count) throw Exception(ErrorCode::INVALID_ARGUMENT, what + ": the causal form pairs item i of a with items j <= i of b: as many of each");
    if (a.is_ntt() || b.is_ntt() || a.size() != 2 || b.size() != 2 || a.words() != a.batch() * in_words || b.words() != b.batch() * in_words ||
        a_first + a_count > a.batch() || b_first + b_count > b.batch())
        throw Exception(ErrorCode::INVALID_ARGUMENT, what + ": 2-component coefficient-domain ciphertexts on the data context, a_count items of a and b_count items of b");
    const size_t pairs = causal ? a_count * (a_count + 1) / 2 : a_count * b_count;
    if (out.size() != 2 || out.words() != out.batch() * out_words || out_first + pairs > out.batch())
        throw Exception(ErrorCode::INVALID_ARGUMENT, what + ": output must live on the next-level context (Ld - 1 limbs), 2 components, with room for one item per pair");
    if (pairs == 0) return;
    grow_scratch(impl_->scratch_product, pairs, [&](size_t m) { return new Ciphertext(data, 3, m); });
    grow_scratch(impl_->scratch_work, pairs, [&](size_t m) { return new PolyBuffer(*impl_->ext, m, 2, false); });
    check(dpfhe_ct_mul_outer(handle_of(data), impl_->scratch_product->data(), a.data() + a_first * in_words, b.data() + b_first * in_words, a_count, b_count,
                             causal ? DPFHE_OUTER_CAUSAL : 0, s),
          "dpfhe_ct_mul_outer");
    check(dpfhe_relinearize_rescale_hybrid(handle_of(*impl_->ext), out.data() + out_first * out_words, impl_->scratch_product->data(), impl_->relin->data(),
                                           impl_->scratch_work->data(), pairs, s),
          "dpfhe_relinearize_rescale_hybrid");
    out.set_ntt(false);
}

const Context& HybridKeySwitcher::extended_context() const { return *impl_->ext; }
const Context& HybridKeySwitcher::data_context() const { return *impl_->data_ctx; }

void HybridKeySwitcher::rotate_hoisted_qp(const Ciphertext& in2, size_t in_first, size_t n_items, const std::vector<uint32_t>& elts, PolyBuffer& out_qp,
                                          size_t out_first, Stream* s) const {
    const size_t k = elts.size();
    if (n_items == 0) return;
    const FheParams& pe = impl_->ext->params();
    const size_t L = pe.n_limbs(), Ld = L - 1, n = pe.n();
    if (in2.is_ntt() || in2.size() != 2 || out_qp.size() != 2 || in_first + n_items > in2.batch() || out_first + (k + 1) * n_items > out_qp.batch() ||
        out_qp.words() != out_qp.batch() * 2 * L * n)
        throw Exception(ErrorCode::INVALID_ARGUMENT, "HybridKeySwitcher::rotate_hoisted_qp: n_items coefficient-domain inputs, (k + 1) * n_items items on the extended context out");
    const PolyBuffer* keys = k ? impl_->packed_keys(elts, s) : nullptr;
    impl_->ensure_digits(n_items * Ld);
    grow_scratch(impl_->scratch_in_ntt, n_items, [&](size_t b) { return new Ciphertext(*impl_->data_ctx, 2, b, true); });
    check(dpfhe_rotate_hoisted_qp(handle_of(*impl_->ext), out_qp.data() + out_first * 2 * L * n, in2.data() + in_first * 2 * Ld * n, n_items,
                                  elts.data(), keys ? keys->data() : nullptr, impl_->scratch_in_ntt->data(), impl_->scratch_digits->data(), k, s),
          "dpfhe_rotate_hoisted_qp");
    out_qp.set_ntt(true);
}

void HybridKeySwitcher::switch_key_qp(const Ciphertext& in2, size_t in_first, const std::vector<uint32_t>& elts, size_t group, PolyBuffer& out_qp,
                                      size_t out_first, Stream* s) const {
    const size_t k = elts.size(), batch = k * group;
    if (batch == 0) return;
    const FheParams& pe = impl_->ext->params();
    const size_t L = pe.n_limbs(), Ld = L - 1, n = pe.n();
    if (in2.is_ntt() || in2.size() != 2 || out_qp.size() != 2 || in_first + batch > in2.batch() || out_first + batch > out_qp.batch() ||
        out_qp.words() != out_qp.batch() * 2 * L * n)
        throw Exception(ErrorCode::INVALID_ARGUMENT, "HybridKeySwitcher::switch_key_qp: k * group coefficient-domain items in, as many items on the extended context out");
    const PolyBuffer* keys = impl_->packed_keys(elts, s);
    check(dpfhe_switch_key_qp(handle_of(*impl_->ext), out_qp.data() + out_first * 2 * L * n, in2.data() + in_first * 2 * Ld * n, keys->data(), k,
                              group, s),
          "dpfhe_switch_key_qp");
    out_qp.set_ntt(true);
}

// ---- SlotSum -------------------------------------------------------------------------------------------------------------
class __attribute__((visibility("hidden"))) SlotSum::Impl {
public:
    HybridKeySwitcher* ks = nullptr;
    size_t block = 0, stride = 0;
    std::vector<uint32_t> elts;
};

SlotSum::SlotSum(HybridKeySwitcher& ks, size_t block, size_t stride) : impl_(new Impl) {
    const FheParams& p = ks.data_context().params();
    const size_t n = p.n();
    auto pow2 = [](size_t v) { return v && !(v & (v - 1)); };
    if (!pow2(block) || !pow2(stride) || block < 2 || stride > n / 2 || block > n / 2 / stride)
        throw Exception(ErrorCode::INVALID_ARGUMENT, "SlotSum: block and stride must be powers of two with block >= 2 and block * stride <= N / 2");
    impl_->ks = &ks;
    impl_->block = block;
    impl_->stride = stride;
    uint64_t g = 3;   // 3^stride mod 2N by `log2(stride)` squarings, then one squaring per step
    for (size_t v = stride; v > 1; v >>= 1) g = g * g % (2 * n);
    for (size_t b = block; b > 1; b >>= 1) {
        impl_->elts.push_back((uint32_t)g);
        ks.add_galois_element((uint32_t)g);
        g = g * g % (2 * n);
    }
}
SlotSum::~SlotSum() = default;
size_t SlotSum::block() const { return impl_->block; }
size_t SlotSum::stride() const { return impl_->stride; }
size_t SlotSum::steps() const { return impl_->elts.size(); }
const std::vector<uint32_t>& SlotSum::galois_elements() const { return impl_->elts; }

double SlotSum::error_bound(uint32_t log2_n, const std::vector<uint64_t>& data_moduli, uint64_t special_prime, size_t block, double scale, double max_abs_input,
                            double input_noise_bound) {
    const BoundUnits bu(log2_n);
    const double N = bu.N, H = bu.H, u8 = bu.u8, B = (double)block;
    const double K = keyswitch_term((double)data_moduli.size(), N, max_modulus(data_moduli, data_moduli.size()), special_prime);
    const double pre = N * (B * input_noise_bound + (B - 1) * (K + H)) / scale;
    return pre + u8 * N * (B * max_abs_input + pre);
}
double SlotSum::error_bound(double scale, double max_abs_input, double input_noise_bound) const {
    const FheParams& pe = impl_->ks->extended_context().params();
    return error_bound(pe.log2_n, std::vector<uint64_t>(pe.moduli.begin(), pe.moduli.end() - 1), pe.moduli.back(), impl_->block, scale, max_abs_input,
                       input_noise_bound);
}

void SlotSum::apply(const Ciphertext& x, Ciphertext& y, Stream* s) const {
    if (x.batch() == 0 || y.batch() != x.batch()) throw Exception(ErrorCode::INVALID_ARGUMENT, "SlotSum::apply: T items in, T items out");
    impl_->ks->rotate_add_range(x, 0, x.batch(), impl_->elts, y, 0, s);
}

}  // namespace fhe
}  // namespace deeppowers
