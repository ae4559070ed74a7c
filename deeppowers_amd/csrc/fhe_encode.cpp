// fhe_encode.cpp - the facade's slot encoders: BatchEncoder (N slots of Z_t) and ComplexEncoder (N/2 complex slots).  Part of libdpfhe_api.so
// (fhe_api.cpp names the other units).
#include <mutex>

#include "fhe_internal.h"
#include "fhe_sampler.h"   // powmod

namespace deeppowers {
namespace fhe {

using namespace detail;

namespace {
// Device encoders (include/dpfhe.h dpfhe_encoder, dpfhe_cencoder), one per context an encoder has been asked to encode for: a device encoder is bound to
// one context's limbs.  An entry remembers the moduli it was made for: a context that died and another that took its handle's address never share one.
template <class Enc, int (*destroy)(Enc*)>
struct DeviceEncoders {
    struct Entry { void* handle; std::vector<uint64_t> moduli; Enc* enc; };
    std::mutex mutex;
    std::vector<Entry> entries;
    ~DeviceEncoders() {
        for (auto& e : entries) (void)destroy(e.enc);
    }
    // the encoder of context c (ring degree n), made by create(dpfhe_ctx*) - which throws rather than return null - on first use.  Thread-safe.
    template <class Create>
    Enc* get(const Context& c, size_t n, const char* who, Create create) {
        if (c.params().n() != n) throw Exception(ErrorCode::INVALID_ARGUMENT, std::string(who) + "::encode_device: the target's context has another ring degree");
        std::lock_guard<std::mutex> lock(mutex);
        for (size_t i = 0; i < entries.size(); ++i) {
            if (entries[i].handle != c.handle()) continue;
            if (entries[i].moduli == c.params().moduli) return entries[i].enc;
            (void)destroy(entries[i].enc);   // (frees its own tables only: the context it was bound to is gone)
            entries.erase(entries.begin() + i);
            break;
        }
        entries.push_back(Entry{c.handle(), c.params().moduli, create(handle_of(c))});
        return entries.back().enc;
    }
};

// 3^steps mod 2N: rotates the slots of a row of N/2 LEFT by steps (negative steps rotate right)
uint32_t galois_element_for(int steps, size_t n) {
    const long long row = (long long)n / 2;
    const uint64_t s = (uint64_t)(((steps % row) + row) % row);
    return (uint32_t)powmod(3, s, 2 * n);
}
}  // namespace

// ---- N3: slot packing --------------------------------------------------------------------------------------------------------
class BatchEncoder::Impl {
public:
    uint64_t t = 0;
    size_t n = 0;
    int logn = 0;
    uint64_t n_inv = 0, zeta = 0;
    mutable DeviceEncoders<dpfhe_encoder, dpfhe_encoder_destroy> encoders;
    dpfhe_encoder* encoder_for(const Context& c) const {
        return encoders.get(c, n, "BatchEncoder", [&](dpfhe_ctx* h) {
            dpfhe_encoder* e = nullptr;
            check(dpfhe_encoder_create(&e, h, t), "dpfhe_encoder_create");
            if (dpfhe_encoder_root(e) != zeta) {
                (void)dpfhe_encoder_destroy(e);
                throw Exception(ErrorCode::INVALID_STATE, "BatchEncoder::encode_device: host and device encoders disagree on the root of unity");
            }
            return e;
        });
    }
    std::vector<uint64_t> rp, irp;       // zeta^brv(i), zeta^-brv(i) mod t  (the library's NTT convention, over Z_t)
    std::vector<uint32_t> idx;           // slot -> NTT index: row 0 slots, then row 1 slots

    static uint32_t brv(uint32_t x, int bits) { uint32_t r = 0; for (int i = 0; i < bits; ++i) { r = (r << 1) | (x & 1); x >>= 1; } return r; }
    uint64_t mul(uint64_t a, uint64_t b) const { return (uint64_t)((u128)a * b % t); }
    void ntt_fwd(std::vector<uint64_t>& a) const {   // natural in -> bit-reversed out: a^[k] = a(zeta^(2 brv(k) + 1))
        for (size_t m = 1, len = n / 2; m < n; m <<= 1, len >>= 1)
            for (size_t i = 0; i < m; ++i) {
                const uint64_t w = rp[m + i];
                for (size_t j = 2 * i * len; j < 2 * i * len + len; ++j) {
                    const uint64_t u = a[j], v = mul(a[j + len], w);
                    a[j] = u + v >= t ? u + v - t : u + v;
                    a[j + len] = u >= v ? u - v : u + t - v;
                }
            }
    }
    void ntt_inv(std::vector<uint64_t>& a) const {
        for (size_t m = n / 2, len = 1; m >= 1; m >>= 1, len <<= 1)
            for (size_t i = 0; i < m; ++i) {
                const uint64_t w = irp[m + i];
                for (size_t j = 2 * i * len; j < 2 * i * len + len; ++j) {
                    const uint64_t u = a[j], v = a[j + len];
                    a[j] = u + v >= t ? u + v - t : u + v;
                    a[j + len] = mul(u >= v ? u - v : u + t - v, w);
                }
            }
        for (auto& v : a) v = mul(v, n_inv);
    }
};

BatchEncoder::BatchEncoder(const Context& ctx, uint64_t t) : impl_(new Impl) {
    const size_t n = ctx.params().n();
    if (t < 3 || (t >> 32) || (t - 1) % (2 * n) != 0) throw Exception(ErrorCode::INVALID_ARGUMENT, "BatchEncoder: plaintext modulus must be a prime = 1 mod 2N below 2^32");
    impl_->t = t; impl_->n = n; impl_->logn = (int)ctx.params().log2_n;
    uint64_t zeta = 0;
    for (uint64_t g = 2; g < t && !zeta; ++g) {   // zeta = g^((t-1)/2N) has order exactly 2N iff zeta^N = -1
        const uint64_t z = powmod(g, (t - 1) / (2 * n), t);
        if (powmod(z, n, t) == t - 1) zeta = z;
    }
    if (!zeta) throw Exception(ErrorCode::INVALID_ARGUMENT, "BatchEncoder: no primitive 2N-th root of unity mod t (t not prime?)");
    const uint64_t izeta = powmod(zeta, t - 2, t);
    impl_->zeta = zeta;
    impl_->rp.assign(n, 0); impl_->irp.assign(n, 0);
    uint64_t pw = 1, ipw = 1;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t r = Impl::brv((uint32_t)i, impl_->logn);
        impl_->rp[r] = pw; impl_->irp[r] = ipw;
        pw = impl_->mul(pw, zeta); ipw = impl_->mul(ipw, izeta);
    }
    impl_->n_inv = powmod(n % t, t - 2, t);
    impl_->idx.assign(n, 0);
    uint64_t e = 1;
    for (size_t i = 0; i < n / 2; ++i) {
        impl_->idx[i] = Impl::brv((uint32_t)((e - 1) / 2), impl_->logn);                  // zeta^(3^i)
        impl_->idx[n / 2 + i] = Impl::brv((uint32_t)((2 * n - e - 1) / 2), impl_->logn);  // zeta^(-3^i)
        e = e * 3 % (2 * n);
    }
}
BatchEncoder::~BatchEncoder() = default;
uint64_t BatchEncoder::plain_modulus() const { return impl_->t; }
size_t BatchEncoder::slot_count() const { return impl_->n; }
size_t BatchEncoder::row_size() const { return impl_->n / 2; }

void BatchEncoder::encode(const uint64_t* slots, int64_t* coeffs) const {
    if (!slots || !coeffs) throw Exception(ErrorCode::INVALID_ARGUMENT, "BatchEncoder::encode: null argument");
    const size_t n = impl_->n;
    std::vector<uint64_t> a(n);
    for (size_t i = 0; i < n; ++i) {
        if (slots[i] >= impl_->t) throw Exception(ErrorCode::INVALID_ARGUMENT, "BatchEncoder::encode: slot value >= plaintext modulus");
        a[impl_->idx[i]] = slots[i];
    }
    impl_->ntt_inv(a);
    for (size_t i = 0; i < n; ++i) coeffs[i] = a[i] > impl_->t / 2 ? (int64_t)a[i] - (int64_t)impl_->t : (int64_t)a[i];
}
void BatchEncoder::decode(const uint64_t* coeffs, uint64_t* slots) const {
    if (!slots || !coeffs) throw Exception(ErrorCode::INVALID_ARGUMENT, "BatchEncoder::decode: null argument");
    const size_t n = impl_->n;
    std::vector<uint64_t> a(coeffs, coeffs + n);
    for (auto& v : a) v %= impl_->t;
    impl_->ntt_fwd(a);
    for (size_t i = 0; i < n; ++i) slots[i] = a[impl_->idx[i]];
}
uint64_t BatchEncoder::root() const { return impl_->zeta; }
void BatchEncoder::encode_device_words(const Context& ctx, const uint32_t* slots, size_t items, uint64_t* d_out, uint32_t flags, Stream* s) const {
    if (!slots || !d_out || items == 0) throw Exception(ErrorCode::INVALID_ARGUMENT, "BatchEncoder::encode_device: null argument or no items");
    dpfhe_encoder* e = impl_->encoder_for(ctx);
    hipPointerAttribute_t attr{};
    const bool on_device = hipPointerGetAttributes(&attr, slots) == hipSuccess && attr.type == hipMemoryTypeDevice;
    if (on_device) {
        check(dpfhe_encode_slots(e, d_out, slots, items, flags, s), "dpfhe_encode_slots");
        return;
    }
    (void)hipGetLastError();   // (an unregistered host pointer is reported as an error by some runtimes)
    hip_check(hipSetDevice(ctx.device_id()), "hipSetDevice");
    void* stage = nullptr;
    const size_t bytes = items * impl_->n * sizeof(uint32_t);
    hip_check(hipMalloc(&stage, bytes), "hipMalloc");
    hipError_t err = hipMemcpyAsync(stage, slots, bytes, hipMemcpyHostToDevice, static_cast<hipStream_t>(s));
    int rc = DPFHE_SUCCESS;
    if (err == hipSuccess) rc = dpfhe_encode_slots(e, d_out, static_cast<const uint32_t*>(stage), items, flags, s);
    if (err == hipSuccess) err = hipStreamSynchronize(static_cast<hipStream_t>(s));
    (void)hipFree(stage);
    hip_check(err, "BatchEncoder::encode_device staging");
    check(rc, "dpfhe_encode_slots");
}
void BatchEncoder::encode_device(const uint32_t* slots, size_t items, Plaintext& out, bool to_ntt, Stream* s) const {
    if (out.batch() != items) throw Exception(ErrorCode::INVALID_ARGUMENT, "BatchEncoder::encode_device: the plaintext must hold `items` polynomials");
    encode_device_words(out.context(), slots, items, out.data(), to_ntt ? DPFHE_ENCODE_NTT : 0u, s);
    out.set_ntt(to_ntt);
}
uint32_t BatchEncoder::galois_element(int left_rotation) const { return galois_element_for(left_rotation, impl_->n); }

// ---- complex slot encoding (include/dpfhe.h dpfhe_encode_complex) ---------------------------------------------------------------------
class ComplexEncoder::Impl {
public:
    size_t n = 0;
    uint32_t logn = 0;
    mutable DeviceEncoders<dpfhe_cencoder, dpfhe_cencoder_destroy> encoders;
    dpfhe_cencoder* encoder_for(const Context& c) const {
        return encoders.get(c, n, "ComplexEncoder", [](dpfhe_ctx* h) {
            dpfhe_cencoder* e = nullptr;
            check(dpfhe_cencoder_create(&e, h), "dpfhe_cencoder_create");
            return e;
        });
    }
};

ComplexEncoder::ComplexEncoder(const Context& ctx) : impl_(new Impl) {
    impl_->n = ctx.params().n();
    impl_->logn = (uint32_t)ctx.params().log2_n;
}
ComplexEncoder::~ComplexEncoder() = default;
size_t ComplexEncoder::slot_count() const { return impl_->n / 2; }
uint32_t ComplexEncoder::galois_element(int steps) const { return galois_element_for(steps, impl_->n); }
uint32_t ComplexEncoder::conjugation_element() const { return (uint32_t)(2 * impl_->n - 1); }

void ComplexEncoder::encode(const std::complex<double>* slots, double scale, int64_t* coeffs) const {
    if (!slots || !coeffs) throw Exception(ErrorCode::INVALID_ARGUMENT, "ComplexEncoder::encode: null argument");
    const size_t n = impl_->n;
    std::vector<double> in(n);       // (staged: the entry takes 16-byte aligned buffers, the caller's need not be)
    std::vector<uint64_t> out(n);
    for (size_t i = 0; i < n / 2; ++i) { in[2 * i] = slots[i].real(); in[2 * i + 1] = slots[i].imag(); }
    const uint64_t any_modulus = 3;  // (the plain form has no limbs)
    check(dpfhe_encode_complex_host(&any_modulus, 1, impl_->logn, out.data(), in.data(), 1, scale, DPFHE_ENCODE_PLAIN), "dpfhe_encode_complex_host");
    for (size_t k = 0; k < n; ++k) coeffs[k] = (int64_t)out[k];
}
void ComplexEncoder::decode(const int64_t* coeffs, double scale, std::complex<double>* slots) const {
    if (!slots || !coeffs) throw Exception(ErrorCode::INVALID_ARGUMENT, "ComplexEncoder::decode: null argument");
    const size_t n = impl_->n;
    std::vector<double> out(n);
    check(dpfhe_decode_complex_host(impl_->logn, out.data(), coeffs, 1, scale, 0), "dpfhe_decode_complex_host");
    for (size_t i = 0; i < n / 2; ++i) slots[i] = std::complex<double>(out[2 * i], out[2 * i + 1]);
}
void ComplexEncoder::encode_device_words(const Context& ctx, const double* d_slots, size_t items, double scale, uint64_t* d_out, uint32_t flags, Stream* s) const {
    if (!d_slots || !d_out || items == 0) throw Exception(ErrorCode::INVALID_ARGUMENT, "ComplexEncoder::encode_device: null argument or no items");
    check(dpfhe_encode_complex(impl_->encoder_for(ctx), d_out, d_slots, items, scale, flags, s), "dpfhe_encode_complex");
}
void ComplexEncoder::encode_device(const double* d_slots, size_t items, double scale, Plaintext& out, bool to_ntt, bool real, Stream* s) const {
    if (out.batch() != items) throw Exception(ErrorCode::INVALID_ARGUMENT, "ComplexEncoder::encode_device: the plaintext must hold `items` polynomials");
    encode_device_words(out.context(), d_slots, items, scale, out.data(), (to_ntt ? DPFHE_ENCODE_NTT : 0u) | (real ? DPFHE_ENCODE_REAL : 0u), s);
    out.set_ntt(to_ntt);
}

}  // namespace fhe
}  // namespace deeppowers
