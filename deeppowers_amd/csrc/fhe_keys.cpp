// fhe_keys.cpp - everything in the facade that holds or draws secrets: SecretKey, KeyGenerator, Encryptor, Decryptor, Rerandomizer (host side: sampling
// and CRT decoding run on the CPU, polynomial arithmetic goes through the C ABI).  Part of libdpfhe_api.so (fhe_api.cpp names the other units).
//
// Every fresh RLWE sample has ONE builder: make_switch_key (relinearisation, Galois and hybrid keys), make_public_key, encrypt_scaled (symmetric) and
// encrypt_scaled_pk; a non-null Seed* means "the uniform half is expand(seed, item, ., 1), expanded on the device".  The ORDER in which a builder
// consumes its Sampler decides every word a TestSeed run produces (tests/test_gpu_facade_digests.py): each builder states its order.
#include <algorithm>
#include <cmath>

#include "fhe_bigint.h"
#include "fhe_internal.h"
#include "fhe_sampler.h"

namespace deeppowers {
namespace fhe {

using namespace detail;

namespace {
// ---- host samplers: one polynomial [L][N] each ------------------------------------------------------------------------------------------
template <class F>
void fill_poly(const FheParams& p, uint64_t* host, F f) {   // host[l][k] = f(k, q_l, l), limb-major
    const size_t n = p.n();
    for (size_t l = 0; l < p.n_limbs(); ++l)
        for (size_t k = 0; k < n; ++k) host[l * n + k] = f(k, p.moduli[l], l);
}
// a small signed polynomial (a secret), the same integer in every limb
template <class T>
void lift_to_limbs(const FheParams& p, const T* v, uint64_t* host) {
    fill_poly(p, host, [&](size_t k, uint64_t q, size_t) { return lift_signed(v[k], q); });
}
// uniform (it serves either domain); draws limb-major
void sample_uniform(Sampler& rng, const FheParams& p, uint64_t* host) {
    fill_poly(p, host, [&](size_t, uint64_t q, size_t) { return rng.below(q); });
}
// centred-binomial error, the same integer in every limb (`add`: host += e); draws one value per coefficient
void sample_error(Sampler& rng, const FheParams& p, uint64_t* host, bool add = false) {
    std::vector<int64_t> e(p.n());
    for (auto& v : e) v = rng.error();
    fill_poly(p, host, [&](size_t k, uint64_t q, size_t l) {
        const uint64_t v = (add ? host[l * e.size() + k] : 0) + lift_signed(e[k], q);
        return v >= q ? v - q : v;
    });
}
// scale * m per limb, for the N signed coefficients of one item
void scale_message(const FheParams& p, const int64_t* message, const std::vector<uint64_t>& scale, uint64_t* host) {
    fill_poly(p, host, [&](size_t k, uint64_t q, size_t l) { return (uint64_t)((u128)lift_signed(message[k], q) * scale[l] % q); });
}
void upload(uint64_t* d_dst, const std::vector<uint64_t>& host) {
    hip_check(hipMemcpy(d_dst, host.data(), host.size() * sizeof(uint64_t), hipMemcpyHostToDevice), "hipMemcpy H2D");
}
// the two scales of an encryption, one residue per limb: 2^k (approximate flavour) and floor(Q / t) (exact flavour); `who` leads the message of their check
std::vector<uint64_t> scale_power_of_two(const std::string& who, const FheParams& p, uint64_t log2_scale) {
    if (log2_scale > 200) throw Exception(ErrorCode::INVALID_ARGUMENT, who + ": log2_scale too large");
    std::vector<uint64_t> scale(p.n_limbs());
    for (size_t l = 0; l < p.n_limbs(); ++l) scale[l] = powmod(2, log2_scale, p.moduli[l]);
    return scale;
}
std::vector<uint64_t> scale_q_over_t(const std::string& who, const FheParams& p, uint64_t t) {
    if (t < 2) throw Exception(ErrorCode::INVALID_ARGUMENT, who + ": plaintext modulus must be >= 2");
    Big delta = modulus_product(p.moduli);
    big_divmod_small(delta, t);   // floor(Q / t)
    std::vector<uint64_t> scale(p.n_limbs());
    for (size_t l = 0; l < p.n_limbs(); ++l) scale[l] = big_mod_small(delta, p.moduli[l]);
    return scale;
}
std::vector<int8_t> sample_ternary(size_t n, Sampler rng) {
    std::vector<int8_t> s(n);
    for (auto& v : s) v = (int8_t)rng.ternary();
    return s;
}
void check_public_key(const char* who, const PublicKey& pk) {
    if (!pk.is_ntt() || pk.size() != 2 || pk.batch() != 1)
        throw Exception(ErrorCode::INVALID_ARGUMENT, std::string(who) + ": public key must be one 2-component NTT-domain item");
}
}  // namespace

// ---- SecretKey ----------------------------------------------------------------------------------------------------------
class SecretKey::Impl {
public:
    const Context* ctx = nullptr;
    std::vector<int8_t> s;
    std::unique_ptr<PolyBuffer> s_hat, s2_hat;
};

SecretKey::SecretKey(const Context& ctx) : SecretKey(ctx, sample_ternary(ctx.params().n(), Sampler())) {}
SecretKey::SecretKey(const Context& ctx, TestSeed seed) : SecretKey(ctx, sample_ternary(ctx.params().n(), Sampler(seed))) {}

SecretKey::SecretKey(const Context& ctx, const std::vector<int8_t>& coeffs) : impl_(new Impl) {
    impl_->ctx = &ctx;
    const FheParams& p = ctx.params();
    const size_t n = p.n(), L = p.n_limbs();
    if (coeffs.size() != n) throw Exception(ErrorCode::INVALID_ARGUMENT, "SecretKey: need N ternary coefficients");
    for (int8_t v : coeffs)
        if (v < -1 || v > 1) throw Exception(ErrorCode::INVALID_ARGUMENT, "SecretKey: coefficients must be in {-1, 0, 1}");
    impl_->s = coeffs;
    std::vector<uint64_t> host(L * n);
    lift_to_limbs(p, impl_->s.data(), host.data());
    impl_->s_hat.reset(new PolyBuffer(ctx, 1, 1, false));
    impl_->s2_hat.reset(new PolyBuffer(ctx, 1, 1, true));
    impl_->s_hat->copy_from_host(host.data());
    Evaluator ev(ctx);
    ev.transform_to_ntt_inplace(*impl_->s_hat);
    ev.dyadic_multiply(*impl_->s_hat, *impl_->s_hat, *impl_->s2_hat);
    ctx.synchronize();
}
SecretKey::~SecretKey() = default;
const std::vector<int8_t>& SecretKey::coefficients() const { return impl_->s; }
const uint64_t* SecretKey::ntt() const { return impl_->s_hat->data(); }
const uint64_t* SecretKey::ntt_squared() const { return impl_->s2_hat->data(); }

// ---- KeyGenerator ----------------------------------------------------------------------------------------------------------
class __attribute__((visibility("hidden"))) KeyGenerator::Impl {   // (hidden like the Sampler it holds)
public:
    const Context* ctx = nullptr;
    std::unique_ptr<SecretKey> sk;
    Sampler rng;
    void switch_key(const uint64_t* d_target_ntt, PolyBuffer& out, Seed* seed_out) { make_switch_key(*ctx, *sk, rng, d_target_ntt, out, 0, seed_out); }
    void galois_key(GaloisKeys& out, Seed* seed_out) {
        PolyBuffer target = galois_target_ntt(*ctx, sk->coefficients(), out.galois_elt());
        switch_key(target.data(), out, seed_out);
    }
};

KeyGenerator::KeyGenerator(const Context& ctx) : impl_(new Impl) {
    impl_->ctx = &ctx;
    impl_->sk.reset(new SecretKey(ctx));
}
KeyGenerator::KeyGenerator(const Context& ctx, TestSeed seed) : impl_(new Impl) {
    impl_->ctx = &ctx;
    impl_->sk.reset(new SecretKey(ctx, seed));
    impl_->rng = Sampler(TestSeed{seed.value ^ 0xD1B54A32D192ED03ull});
}
KeyGenerator::~KeyGenerator() = default;
const SecretKey& KeyGenerator::secret_key() const { return *impl_->sk; }

// NTT(sigma_g(s)): the target of the switching key for Galois element g
PolyBuffer detail::galois_target_ntt(const Context& ctx, const std::vector<int8_t>& s, uint32_t galois_elt) {
    const FheParams& p = ctx.params();
    const size_t n = p.n();
    std::vector<int8_t> sg(n, 0);
    for (size_t i = 0; i < n; ++i) {   // sigma_g(s): coefficient i -> index i g mod 2N, negated past N
        const size_t idx = (i * (size_t)galois_elt) & (2 * n - 1);
        if (idx < n) sg[idx] = s[i]; else sg[idx - n] = (int8_t)-s[i];
    }
    std::vector<uint64_t> host(p.n_limbs() * n);
    lift_to_limbs(p, sg.data(), host.data());
    PolyBuffer target(ctx, 1, 1, false);
    target.copy_from_host(host.data());
    Evaluator ev(ctx);
    ev.transform_to_ntt_inplace(target);
    ctx.synchronize();
    return target;
}

// Shared by relinearisation, Galois and hybrid keys: key_j = (-(a_j s) + e_j + g_j * target, a_j), everything in the NTT domain.
// Draw order: per digit j all of a_j (limb-major), then the N errors; seeded: the seed first, then per digit the N errors.
void detail::make_switch_key(const Context& ctx, const SecretKey& sk, Sampler& rng, const uint64_t* d_target_ntt, PolyBuffer& out, size_t n_digits, Seed* seed_out) {
    const FheParams& p = ctx.params();
    const size_t n = p.n(), L = p.n_limbs(), poly = L * n, digits = n_digits ? n_digits : L;
    dpfhe_ctx* h = handle_of(ctx);
    if (seed_out) {   // a_j = expand(seed, j, ., 1) written straight into the key's NTT-domain component
        if (out.batch() != L || out.size() != 2) throw Exception(ErrorCode::INVALID_ARGUMENT, "seeded switching key: [L][2][L][N] expected");
        draw_seed(rng, *seed_out);
        check(dpfhe_expand_uniform(h, out.data(), L, 2, 1, seed_out->bytes, 0, nullptr), "dpfhe_expand_uniform");
    }
    PolyBuffer e(ctx, 1, 1, false), t(ctx, 1, 1, true);
    std::vector<uint64_t> host(poly);
    for (size_t j = 0; j < digits; ++j) {
        uint64_t* b = out.data() + (j * 2 + 0) * poly;   // evk_j[0]
        uint64_t* a = out.data() + (j * 2 + 1) * poly;   // evk_j[1] = a_j
        if (!seed_out) {
            sample_uniform(rng, p, host.data());
            upload(a, host);
        }
        sample_error(rng, p, host.data());
        e.copy_from_host(host.data());
        check(dpfhe_ntt_fwd(h, e.data(), 1, nullptr), "dpfhe_ntt_fwd");                       // NTT(e_j)
        check(dpfhe_dyadic_mul(h, t.data(), a, sk.ntt(), 1, nullptr), "dpfhe_dyadic_mul");      // a_j s
        check(dpfhe_sub(h, b, e.data(), t.data(), 1, nullptr), "dpfhe_sub");                   // e_j - a_j s
        // + g_j * target : the target polynomial in limb j only (g_j = 1 mod q_j, 0 mod the other primes)
        check(dpfhe_add(h, t.data(), b, d_target_ntt, 1, nullptr), "dpfhe_add");
        hip_check(hipMemcpyAsync(b + j * n, t.data() + j * n, n * sizeof(uint64_t), hipMemcpyDeviceToDevice, nullptr), "hipMemcpyAsync");
        ctx.synchronize();
    }
    out.set_ntt(true);
}

namespace {
// pk = (e - a s, a), NTT domain.  Draw order: a, then the N errors; seeded: the seed, then the N errors.
void make_public_key(const Context& ctx, const SecretKey& sk, Sampler& rng, PublicKey& out, Seed* seed_out) {
    const FheParams& p = ctx.params();
    const size_t poly = p.n_limbs() * p.n();
    dpfhe_ctx* h = handle_of(ctx);
    std::vector<uint64_t> host(poly);
    uint64_t* a = out.data() + poly;   // uniform: any domain
    if (seed_out) {
        draw_seed(rng, *seed_out);
        check(dpfhe_expand_uniform(h, out.data(), 1, 2, 1, seed_out->bytes, 0, nullptr), "dpfhe_expand_uniform");
    } else {
        sample_uniform(rng, p, host.data());
        upload(a, host);
    }
    sample_error(rng, p, host.data());
    PolyBuffer e(ctx, 1, 1, false), t(ctx, 1, 1, true);
    e.copy_from_host(host.data());
    check(dpfhe_ntt_fwd(h, e.data(), 1, nullptr), "dpfhe_ntt_fwd");
    check(dpfhe_dyadic_mul(h, t.data(), a, sk.ntt(), 1, nullptr), "dpfhe_dyadic_mul");   // a s
    check(dpfhe_sub(h, out.data(), e.data(), t.data(), 1, nullptr), "dpfhe_sub");         // pk0 = e - a s
    ctx.synchronize();
    out.set_ntt(true);
}
}  // namespace

void KeyGenerator::create_relin_keys(RelinKeys& out) { impl_->switch_key(impl_->sk->ntt_squared(), out, nullptr); }
void KeyGenerator::create_relin_keys_seeded(RelinKeys& out, Seed& seed_out) { impl_->switch_key(impl_->sk->ntt_squared(), out, &seed_out); }
void KeyGenerator::create_galois_keys(GaloisKeys& out) { impl_->galois_key(out, nullptr); }
void KeyGenerator::create_galois_keys_seeded(GaloisKeys& out, Seed& seed_out) { impl_->galois_key(out, &seed_out); }
void KeyGenerator::create_public_key(PublicKey& out) { make_public_key(*impl_->ctx, *impl_->sk, impl_->rng, out, nullptr); }
void KeyGenerator::create_public_key_seeded(PublicKey& out, Seed& seed_out) { make_public_key(*impl_->ctx, *impl_->sk, impl_->rng, out, &seed_out); }

// ---- Encryptor --------------------------------------------------------------------------------------------------------------
namespace {
// c0 = -(a s) + e + scale * m, c1 = a with scale given per limb; seed_out != null: every c1 of the batch is expanded on the device from ONE fresh seed
// (item b: expand(seed, b, ., 1)).  Draw order, per item: a for every limb (limb-major), then the N errors; seeded: one seed for the call, then per
// item the N errors.
void encrypt_scaled(const Context& ctx, const SecretKey& sk, Sampler& rng, const int64_t* messages, const std::vector<uint64_t>& scale, Ciphertext& out,
                    Seed* seed_out) {
    const FheParams& p = ctx.params();
    const size_t n = p.n(), poly = p.n_limbs() * n;
    dpfhe_ctx* h = handle_of(ctx);
    if (seed_out) {
        draw_seed(rng, *seed_out);
        check(dpfhe_expand_uniform(h, out.data(), out.batch(), 2, 1, seed_out->bytes, 0, nullptr), "dpfhe_expand_uniform");   // c1 (coefficient domain)
    }
    PolyBuffer a(ctx, 1, 1, false), t(ctx, 1, 1, false);
    std::vector<uint64_t> ha(poly), hm(poly);
    for (size_t item = 0; item < out.batch(); ++item) {
        uint64_t* c0 = out.data() + (item * 2 + 0) * poly;
        uint64_t* c1 = out.data() + (item * 2 + 1) * poly;
        if (!seed_out) {
            sample_uniform(rng, p, ha.data());
            upload(c1, ha);                                 // c1 = a (coefficient domain)
        }
        scale_message(p, messages + item * n, scale, hm.data());
        sample_error(rng, p, hm.data(), /*add=*/true);
        t.copy_from_host(hm.data());                       // e + scale m
        hip_check(hipMemcpyAsync(a.data(), c1, poly * sizeof(uint64_t), hipMemcpyDeviceToDevice, nullptr), "hipMemcpyAsync");
        check(dpfhe_ntt_fwd(h, a.data(), 1, nullptr), "dpfhe_ntt_fwd");
        check(dpfhe_dyadic_mul(h, a.data(), a.data(), sk.ntt(), 1, nullptr), "dpfhe_dyadic_mul");
        check(dpfhe_ntt_inv(h, a.data(), 1, nullptr), "dpfhe_ntt_inv");          // c1 s
        check(dpfhe_sub(h, c0, t.data(), a.data(), 1, nullptr), "dpfhe_sub");     // c0 = e + scale m - c1 s
        ctx.synchronize();
    }
    out.set_ntt(false);
}
// (c0, c1) = (u pk0 + e1 + scale m, u pk1 + e2), u ternary, e1 / e2 centred binomial.  Draw order, per coefficient: ternary, error, error - so only the
// message scaling is shared with the builders above.
void encrypt_scaled_pk(const Context& ctx, const PublicKey& pk, Sampler& rng, const int64_t* messages, const std::vector<uint64_t>& scale, Ciphertext& out) {
    const FheParams& p = ctx.params();
    const size_t n = p.n(), L = p.n_limbs(), poly = L * n;
    dpfhe_ctx* h = handle_of(ctx);
    PolyBuffer u(ctx, 1, 1, false), t(ctx, 1, 2, false);
    std::vector<uint64_t> hu(poly), ht(2 * poly);
    for (size_t item = 0; item < out.batch(); ++item) {
        scale_message(p, messages + item * n, scale, ht.data());
        for (size_t k = 0; k < n; ++k) {
            const int64_t uv = rng.ternary(), e1 = rng.error(), e2 = rng.error();
            for (size_t l = 0; l < L; ++l) {
                const uint64_t q = p.moduli[l], v = ht[l * n + k] + lift_signed(e1, q);
                hu[l * n + k] = lift_signed(uv, q);
                ht[l * n + k] = v >= q ? v - q : v;                  // e1 + scale m
                ht[poly + l * n + k] = lift_signed(e2, q);           // e2
            }
        }
        uint64_t* c = out.data() + item * 2 * poly;
        u.copy_from_host(hu.data());
        t.copy_from_host(ht.data());
        check(dpfhe_ntt_fwd(h, u.data(), 1, nullptr), "dpfhe_ntt_fwd");
        check(dpfhe_dyadic_mul(h, c, u.data(), pk.data(), 1, nullptr), "dpfhe_dyadic_mul");                  // u pk0
        check(dpfhe_dyadic_mul(h, c + poly, u.data(), pk.data() + poly, 1, nullptr), "dpfhe_dyadic_mul");    // u pk1
        check(dpfhe_ntt_inv(h, c, 2, nullptr), "dpfhe_ntt_inv");
        check(dpfhe_add(h, c, c, t.data(), 2, nullptr), "dpfhe_add");
        ctx.synchronize();
    }
    out.set_ntt(false);
}
}  // namespace

class __attribute__((visibility("hidden"))) Encryptor::Impl {   // (hidden like the Sampler it holds)
public:
    const Context* ctx = nullptr;
    const SecretKey* sk = nullptr;     // symmetric mode
    const PublicKey* pk = nullptr;     // public-key mode
    Sampler rng;
    // the checks every entry shares, in the order the entries always made them; scale_of makes the entry's own check and builds its scale
    void encrypt(const char* name, const int64_t* messages, Ciphertext& out, Seed* seed_out,
                 std::vector<uint64_t> (*scale_of)(const std::string&, const FheParams&, uint64_t), uint64_t scale_arg) {
        const std::string who(name);
        if (seed_out && pk) throw Exception(ErrorCode::INVALID_STATE, who + ": a public-key encryption's c1 = u pk1 + e2 cannot be seeded");
        if (!messages) throw Exception(ErrorCode::INVALID_ARGUMENT, who + ": null messages");
        if (out.size() != 2) throw Exception(ErrorCode::INVALID_ARGUMENT, who + ": output must be a 2-component ciphertext");
        const std::vector<uint64_t> scale = scale_of(who, ctx->params(), scale_arg);
        if (pk) encrypt_scaled_pk(*ctx, *pk, rng, messages, scale, out);
        else encrypt_scaled(*ctx, *sk, rng, messages, scale, out, seed_out);
    }
};
Encryptor::Encryptor(const Context& ctx, const SecretKey& sk) : impl_(new Impl) { impl_->ctx = &ctx; impl_->sk = &sk; }
Encryptor::Encryptor(const Context& ctx, const SecretKey& sk, TestSeed seed) : impl_(new Impl) {
    impl_->ctx = &ctx; impl_->sk = &sk; impl_->rng = Sampler(seed);
}
Encryptor::Encryptor(const Context& ctx, const PublicKey& pk) : impl_(new Impl) {
    check_public_key("Encryptor", pk);
    impl_->ctx = &ctx; impl_->pk = &pk;
}
Encryptor::Encryptor(const Context& ctx, const PublicKey& pk, TestSeed seed) : impl_(new Impl) {
    check_public_key("Encryptor", pk);
    impl_->ctx = &ctx; impl_->pk = &pk; impl_->rng = Sampler(seed);
}
Encryptor::~Encryptor() = default;

void Encryptor::encrypt(const int64_t* messages, unsigned log2_scale, Ciphertext& out) {
    impl_->encrypt("encrypt", messages, out, nullptr, scale_power_of_two, log2_scale);
}
void Encryptor::encrypt_exact(const int64_t* messages, uint64_t t, Ciphertext& out) { impl_->encrypt("encrypt_exact", messages, out, nullptr, scale_q_over_t, t); }
void Encryptor::encrypt_seeded(const int64_t* messages, unsigned log2_scale, Ciphertext& out, Seed& seed_out) {
    impl_->encrypt("encrypt_seeded", messages, out, &seed_out, scale_power_of_two, log2_scale);
}
void Encryptor::encrypt_exact_seeded(const int64_t* messages, uint64_t t, Ciphertext& out, Seed& seed_out) {
    impl_->encrypt("encrypt_exact_seeded", messages, out, &seed_out, scale_q_over_t, t);
}

// ---- Decryptor --------------------------------------------------------------------------------------------------------------
class Decryptor::Impl {
public:
    const Context* ctx = nullptr;
    const SecretKey* sk = nullptr;
    std::vector<uint64_t> garner_inv;  // [i][j<i]: (q_j)^-1 mod q_i  (mixed-radix conversion)
    Big Q, halfQ;
};
Decryptor::Decryptor(const Context& ctx, const SecretKey& sk) : impl_(new Impl) {
    impl_->ctx = &ctx; impl_->sk = &sk;
    const FheParams& p = ctx.params();
    const size_t L = p.n_limbs();
    impl_->garner_inv.assign(L * L, 0);
    for (size_t i = 0; i < L; ++i)
        for (size_t j = 0; j < i; ++j) impl_->garner_inv[i * L + j] = powmod(p.moduli[j] % p.moduli[i], p.moduli[i] - 2, p.moduli[i]);
    impl_->Q = modulus_product(p.moduli);
    impl_->halfQ = impl_->Q;
    big_divmod_small(impl_->halfQ, 2);
}
Decryptor::~Decryptor() = default;

namespace {
// phase = c0 + c1 s (+ c2 s^2) per item on the device (NTT domain), then per coefficient the Garner mixed-radix digits
// x = v0 + v1 q0 + v2 q0 q1 + ... of its CRT composition in [0, Q); f(item, k, digits) consumes them
template <class F>
void for_each_phase(const Context& ctx, const SecretKey& sk, const std::vector<uint64_t>& garner_inv, const Ciphertext& ct, F f) {
    const FheParams& p = ctx.params();
    const size_t n = p.n(), L = p.n_limbs(), poly = L * n;
    dpfhe_ctx* h = handle_of(ctx);
    PolyBuffer acc(ctx, 1, 1, true), t(ctx, 1, 1, true);
    std::vector<uint64_t> ph(poly), digit(L);
    for (size_t item = 0; item < ct.batch(); ++item) {
        const uint64_t* c = ct.data() + item * ct.size() * poly;
        check(dpfhe_ntt_fwd_oop(h, t.data(), c + poly, 1, nullptr), "dpfhe_ntt_fwd_oop");
        check(dpfhe_dyadic_mul(h, acc.data(), t.data(), sk.ntt(), 1, nullptr), "dpfhe_dyadic_mul");
        if (ct.size() == 3) {
            check(dpfhe_ntt_fwd_oop(h, t.data(), c + 2 * poly, 1, nullptr), "dpfhe_ntt_fwd_oop");
            check(dpfhe_dyadic_mul_add(h, acc.data(), t.data(), sk.ntt_squared(), 1, nullptr), "dpfhe_dyadic_mul_add");
        }
        check(dpfhe_ntt_inv(h, acc.data(), 1, nullptr), "dpfhe_ntt_inv");
        check(dpfhe_add(h, acc.data(), acc.data(), c, 1, nullptr), "dpfhe_add");
        ctx.synchronize();
        hip_check(hipMemcpy(ph.data(), acc.data(), poly * sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy D2H");
        for (size_t k = 0; k < n; ++k) {
            for (size_t i = 0; i < L; ++i) {
                const uint64_t qi = p.moduli[i];
                uint64_t v = ph[i * n + k] % qi;
                for (size_t j = 0; j < i; ++j) {
                    const uint64_t dj = digit[j] % qi;
                    v = v >= dj ? v - dj : v + qi - dj;
                    v = (uint64_t)((u128)v * garner_inv[i * L + j] % qi);
                }
                digit[i] = v;
            }
            f(item, k, digit);
        }
    }
}
// round(t x / Q) in [0, t] from x's mixed-radix digits: x / Q = (v0 + q0 (v1 + q1 (...))) / (q0 q1 ...) evaluated from the lowest digit, f <- (v_i + f) / q_i.
// The phase is floor(Q/t) m + small noise, so t x / Q sits within ~2^-200 of an integer and 64-bit long double rounding is exact.
uint64_t round_t_x_over_q(const std::vector<uint64_t>& moduli, const std::vector<uint64_t>& digit, uint64_t t) {
    long double f = 0.0L;
    for (size_t i = 0; i < moduli.size(); ++i) f = ((long double)digit[i] + f) / (long double)moduli[i];
    return (uint64_t)(f * (long double)t + 0.5L);
}
}  // namespace

void Decryptor::decrypt(const Ciphertext& ct, unsigned log2_scale, int64_t* out) {
    if (!out) throw Exception(ErrorCode::INVALID_ARGUMENT, "decrypt: null output");
    if (ct.is_ntt()) throw Exception(ErrorCode::INVALID_STATE, "decrypt: ciphertext must be in the coefficient domain");
    const FheParams& p = impl_->ctx->params();
    const size_t n = p.n();
    for_each_phase(*impl_->ctx, *impl_->sk, impl_->garner_inv, ct, [&](size_t item, size_t k, const std::vector<uint64_t>& digit) {
        Big x = big_from_mixed_radix(p.moduli, digit);
        const bool neg = big_cmp(x, impl_->halfQ) > 0;
        if (neg) x = big_sub(impl_->Q, x);
        big_shr_round(x, log2_scale);
        for (size_t i = 1; i < x.size(); ++i)
            if (x[i]) throw Exception(ErrorCode::RUNTIME_ERROR, "decrypt: value does not fit 62 bits (scale or noise overflow)");
        if (x[0] >> 62) throw Exception(ErrorCode::RUNTIME_ERROR, "decrypt: value does not fit 62 bits (scale or noise overflow)");
        out[item * n + k] = neg ? -(int64_t)x[0] : (int64_t)x[0];
    });
}

void Decryptor::decrypt_exact(const Ciphertext& ct, uint64_t t, uint64_t* out) {
    if (!out) throw Exception(ErrorCode::INVALID_ARGUMENT, "decrypt_exact: null output");
    if (ct.is_ntt()) throw Exception(ErrorCode::INVALID_STATE, "decrypt_exact: ciphertext must be in the coefficient domain");
    if (t < 2 || t >> 32) throw Exception(ErrorCode::INVALID_ARGUMENT, "decrypt_exact: plaintext modulus must be in [2, 2^32)");
    const FheParams& p = impl_->ctx->params();
    const size_t n = p.n();
    for_each_phase(*impl_->ctx, *impl_->sk, impl_->garner_inv, ct, [&](size_t item, size_t k, const std::vector<uint64_t>& digit) {
        const uint64_t m = round_t_x_over_q(p.moduli, digit, t);
        out[item * n + k] = m >= t ? m - t : m;
    });
}

double Decryptor::noise_budget_bits(const Ciphertext& ct, uint64_t t) {
    if (ct.is_ntt()) throw Exception(ErrorCode::INVALID_STATE, "noise_budget_bits: ciphertext must be in the coefficient domain");
    if (t < 2 || t >> 32) throw Exception(ErrorCode::INVALID_ARGUMENT, "noise_budget_bits: plaintext modulus must be in [2, 2^32)");
    const FheParams& p = impl_->ctx->params();
    unsigned worst = 0;   // most noise bits seen
    for_each_phase(*impl_->ctx, *impl_->sk, impl_->garner_inv, ct, [&](size_t, size_t, const std::vector<uint64_t>& digit) {
        // m = round(t x / Q) (exact: the noise is far below the long double's resolution of 1/2), then the noise  e = t x - m Q  in exact integers
        Big x = big_from_mixed_radix(p.moduli, digit);
        big_mul_small(x, t);
        Big mq(impl_->Q);
        big_mul_small(mq, round_t_x_over_q(p.moduli, digit, t));
        worst = std::max(worst, big_bits(big_cmp(x, mq) >= 0 ? big_sub(x, mq) : big_sub(mq, x)));
    });
    return (double)big_bits(impl_->Q) - 1.0 - (double)worst;
}

namespace {
// per coefficient of every item of a compact ciphertext: (K, phase in [0, 2^K)), phase = c0 2^(K - k0) + (c1 * s) 2^(K - k1) mod 2^K
template <class F>
void for_each_compact_phase(const CompactCiphertext& ct, const std::vector<int8_t>& s, F f) {
    const size_t n = ct.ring_degree();
    const unsigned k0 = ct.bits(0), k1 = ct.bits(1), K = std::max(k0, k1);
    const size_t rec = n * (k0 + k1) / 8;
    std::vector<uint8_t> host(ct.bytes());
    ct.copy_to_host(host.data());
    auto value = [](const uint8_t* bytes, size_t j, unsigned k) {   // bits [j k, (j + 1) k) of a little-endian bit string
        uint64_t v = 0;
        for (unsigned b = 0; b < k; ++b) {
            const size_t bit = j * k + b;
            v |= (uint64_t)((bytes[bit / 8] >> (bit % 8)) & 1u) << b;
        }
        return v;
    };
    std::vector<uint64_t> c0(n), c1(n), acc(n);
    const uint64_t mask = K == 64 ? ~0ull : (1ull << K) - 1;
    for (size_t item = 0; item < ct.batch(); ++item) {
        const uint8_t* r = host.data() + item * rec;
        for (size_t j = 0; j < n; ++j) { c0[j] = value(r, j, k0); c1[j] = value(r + n * k0 / 8, j, k1); }
        std::fill(acc.begin(), acc.end(), 0);
        for (size_t j = 0; j < n; ++j) {   // c1 * s in Z_2^64[X]/(X^N + 1): s_j c1 X^j
            if (!s[j]) continue;
            const uint64_t sj = (uint64_t)(int64_t)s[j];   // +-1 in wrapping arithmetic
            for (size_t i = 0; i + j < n; ++i) acc[i + j] += sj * c1[i];
            for (size_t i = n - j; i < n; ++i) acc[i + j - n] -= sj * c1[i];   // X^N = -1
        }
        for (size_t k = 0; k < n; ++k) f(item, k, K, ((c0[k] << (K - k0)) + (acc[k] << (K - k1))) & mask);
    }
}
}  // namespace

void Decryptor::decrypt_exact(const CompactCiphertext& ct, uint64_t t, uint64_t* out) {
    if (!out) throw Exception(ErrorCode::INVALID_ARGUMENT, "decrypt_exact: null output");
    if (t < 2 || t >> 32) throw Exception(ErrorCode::INVALID_ARGUMENT, "decrypt_exact: plaintext modulus must be in [2, 2^32)");
    if (ct.ring_degree() != impl_->ctx->params().n()) throw Exception(ErrorCode::INVALID_ARGUMENT, "decrypt_exact: ring degree differs");
    const size_t n = ct.ring_degree();
    for_each_compact_phase(ct, impl_->sk->coefficients(), [&](size_t item, size_t k, unsigned K, uint64_t phase) {
        const u128 m = ((u128)t * phase + ((u128)1 << (K - 1))) >> K;   // round(t phase / 2^K), in [0, t]
        out[item * n + k] = (uint64_t)(m % t);
    });
}

double Decryptor::noise_budget_bits(const CompactCiphertext& ct, uint64_t t) {
    if (t < 2 || t >> 32) throw Exception(ErrorCode::INVALID_ARGUMENT, "noise_budget_bits: plaintext modulus must be in [2, 2^32)");
    if (ct.ring_degree() != impl_->ctx->params().n()) throw Exception(ErrorCode::INVALID_ARGUMENT, "noise_budget_bits: ring degree differs");
    double worst = 0.0;   // most noise bits seen
    unsigned K = 0;
    for_each_compact_phase(ct, impl_->sk->coefficients(), [&](size_t, size_t, unsigned k, uint64_t phase) {
        K = k;
        // e = t phase - m 2^K with m = round(t phase / 2^K): |e| <= 2^(K-1), exact in 128 bits (t phase < 2^92)
        const u128 tp = (u128)t * phase, m = (tp + ((u128)1 << (K - 1))) >> K, mq = m << K;
        const u128 e = tp >= mq ? tp - mq : mq - tp;
        const uint64_t hi = (uint64_t)(e >> 64), lo = (uint64_t)e;
        const double b = hi ? 128.0 - __builtin_clzll(hi) : (lo ? 64.0 - __builtin_clzll(lo) : 0.0);
        if (b > worst) worst = b;
    });
    return (double)(K + 1) - 1.0 - worst;   // bits(2^K) - 1 - worst, as for Q above
}

// ---- Rerandomizer -------------------------------------------------------------------------------------------------------
class __attribute__((visibility("hidden"))) Rerandomizer::Impl {   // (hidden like the Sampler it holds)
public:
    const Context* ctx = nullptr;
    const PublicKey* pk = nullptr;
    Sampler rng;
    std::unique_ptr<PolyBuffer> work;   // 3 L N words per item: u | the two products (dpfhe_rerandomize)
    unsigned log2_q = 0;                // floor(log2 Q), exact
    void init(const Context& c, const PublicKey& k) {
        check_public_key("Rerandomizer", k);
        if (&k.context() != &c) throw Exception(ErrorCode::INVALID_ARGUMENT, "Rerandomizer: the public key belongs to another context");
        ctx = &c; pk = &k;
        log2_q = big_bits(modulus_product(c.params().moduli)) - 1;
    }
};
Rerandomizer::Rerandomizer(const Context& ctx, const PublicKey& pk) : impl_(new Impl) { impl_->init(ctx, pk); }
Rerandomizer::Rerandomizer(const Context& ctx, const PublicKey& pk, TestSeed seed) : impl_(new Impl) {
    impl_->init(ctx, pk);
    impl_->rng = Sampler(seed);
}
Rerandomizer::~Rerandomizer() = default;
unsigned Rerandomizer::flood_bits_for(double noise_bits, unsigned log2_n, unsigned lambda) {
    const double b = std::ceil(noise_bits < 0 ? 0.0 : noise_bits);
    return (unsigned)b + lambda + log2_n;
}
unsigned Rerandomizer::max_flood_bits(uint64_t t) const {
    unsigned ceil_log2_t = 0;
    while (ceil_log2_t < 64 && ((uint64_t)1 << ceil_log2_t) < t) ++ceil_log2_t;
    const unsigned need = ceil_log2_t + 4;
    const unsigned cap = impl_->log2_q > need ? impl_->log2_q - need : 0;
    return cap < 250 ? cap : 250;
}
void Rerandomizer::rerandomize(Ciphertext& ct, uint64_t t, unsigned flood_bits, Stream* s) {
    Impl& I = *impl_;
    const FheParams& fp = I.ctx->params();
    if (ct.is_ntt() || ct.size() != 2 || ct.batch() == 0 || &ct.context() != I.ctx || ct.words() != ct.batch() * 2 * fp.n_limbs() * fp.n())
        throw Exception(ErrorCode::INVALID_ARGUMENT, "rerandomize: a 2-component coefficient-domain ciphertext of this context (relinearise a product first)");
    if (t < 2 || t >> 32) throw Exception(ErrorCode::INVALID_ARGUMENT, "rerandomize: plaintext modulus must be in [2, 2^32)");
    if (flood_bits < 1 || flood_bits > max_flood_bits(t))
        throw Exception(ErrorCode::INVALID_ARGUMENT, "rerandomize: flood_bits must lie in [1, floor(log2 Q) - ceil(log2 t) - 4] (and at most 250): less than about two bits of budget would remain");
    grow_scratch(I.work, ct.batch(), [&](size_t b) { return new PolyBuffer(*I.ctx, b, 3, false); });
    Seed seed;   // fresh for every call, never stored
    draw_seed(I.rng, seed);
    const int rc = dpfhe_rerandomize(handle_of(*I.ctx), ct.data(), I.pk->data(), ct.batch(), flood_bits, seed.bytes, 0, I.work->data(), s);
    secure_wipe(seed.bytes, sizeof(seed.bytes));
    check(rc, "dpfhe_rerandomize");
}

}  // namespace fhe
}  // namespace deeppowers
