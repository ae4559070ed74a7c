// GPU test of slot encoding on the device in the C++ facade (BatchEncoder::encode_device, ExactPlaintext::set_slots_device): the device words equal
// encode + a lift to every limb + an upload word for word, also on the extended Q P context of a key switcher; an encrypted vector times a
// device-encoded plaintext and plus a device-encoded plaintext decrypts to the slot-wise product and sum mod t; the host and device encoders agree on
// the root of unity.  Built and run by tests/test_gpu_encode.py (-m gpu).  Exit code 0 = all checks passed.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <vector>

#include "facade_test.h"
#include "dpfhe.h"

using namespace deeppowers::fhe;
using namespace facade_test;

static Lcg rnd{2026};

static uint64_t lift(int64_t v, uint64_t q) {
    const int64_t r = (int64_t)((__int128)v % (__int128)q);
    return (uint64_t)(r < 0 ? r + (int64_t)q : r);
}

// encode() + lift + upload (+ the forward transform) of `items` slot vectors on `target`'s context
static std::vector<uint64_t> host_path(const BatchEncoder& be, const Context& target, const std::vector<uint64_t>& slots, size_t items, bool to_ntt) {
    const FheParams& p = target.params();
    const size_t n = p.n(), L = p.n_limbs();
    std::vector<int64_t> c(n);
    std::vector<uint64_t> h(items * L * n);
    for (size_t i = 0; i < items; ++i) {
        be.encode(&slots[i * n], c.data());
        for (size_t l = 0; l < L; ++l)
            for (size_t k = 0; k < n; ++k) h[(i * L + l) * n + k] = lift(c[k], p.moduli[l]);
    }
    Plaintext pt(target, items, false);
    pt.copy_from_host(h.data());
    if (to_ntt) Evaluator(target).transform_to_ntt_inplace(pt);
    target.synchronize();
    return words(pt);
}

static void word_for_word(uint64_t t) {
    FheParams p = FheParams::n8192(3);
    const uint64_t special = p.moduli.back(), special_psi = p.psi.back();
    p.moduli.pop_back(); p.psi.pop_back();
    const size_t n = p.n(), items = 5;
    Context ctx(p, 0);
    KeyGenerator kg(ctx, TestSeed{7});
    HybridKeySwitcher hks(ctx, kg.secret_key(), special, special_psi, TestSeed{8});
    const Context& ext = hks.extended_context();
    BatchEncoder be(ctx, t);
    std::vector<uint64_t> slots(items * n);
    std::vector<uint32_t> s32(items * n);
    for (size_t i = 0; i < slots.size(); ++i) { slots[i] = i < n ? t - 1 : rnd(t); s32[i] = (uint32_t)slots[i]; }
    // the C ABI's root is the facade's
    dpfhe_encoder* e = nullptr;
    CHECK(dpfhe_encoder_create(&e, static_cast<dpfhe_ctx*>(ctx.handle()), t) == 0);
    CHECK(e && dpfhe_encoder_root(e) == be.root() && be.root() != 0);
    CHECK(dpfhe_encoder_destroy(e) == 0);
    uint32_t* d_slots = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void**>(&d_slots), s32.size() * 4) == hipSuccess);
    CHECK(hipMemcpy(d_slots, s32.data(), s32.size() * 4, hipMemcpyHostToDevice) == hipSuccess);
    const Context* targets[] = {&ctx, &ext};
    for (const Context* target : targets)
        for (bool to_ntt : {false, true}) {
            const std::vector<uint64_t> want = host_path(be, *target, slots, items, to_ntt);
            Plaintext from_host(*target, items), from_dev(*target, items);
            be.encode_device(s32.data(), items, from_host, to_ntt);     // host pointer: staged
            be.encode_device(d_slots, items, from_dev, to_ntt);         // device pointer: enqueue only
            target->synchronize();
            CHECK(from_host.is_ntt() == to_ntt && from_dev.is_ntt() == to_ntt);
            CHECK(words(from_host) == want);
            CHECK(words(from_dev) == want);
        }
    // the plain form == encode() reduced to [0, t)
    {
        ExactPlaintext a(ctx, t, items), b(ctx, t, items);
        a.set_slots(be, slots.data());
        b.set_slots_device(be, d_slots);
        ctx.synchronize();
        std::vector<uint64_t> ha(items * n), hb(items * n);
        CHECK(hipMemcpy(ha.data(), a.data(), ha.size() * 8, hipMemcpyDeviceToHost) == hipSuccess);
        CHECK(hipMemcpy(hb.data(), b.data(), hb.size() * 8, hipMemcpyDeviceToHost) == hipSuccess);
        CHECK(ha == hb);
    }
    Plaintext wrong_batch(ctx, items + 1);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { be.encode_device(d_slots, items, wrong_batch); }, "plaintext of another batch");
    Context small(FheParams::n4096_l4(), 0);
    Plaintext other(small, items);
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { be.encode_device(d_slots, items, other); }, "plaintext of another ring degree");
    expect_error(ErrorCode::INVALID_ARGUMENT, [&] { be.encode_device(nullptr, items, wrong_batch); }, "null slots");
    (void)hipFree(d_slots);
}

// Enc(x) (.) device-encoded w + device-encoded b decrypts and decodes to x w + b slot by slot
static void request_time_operands() {
    const uint64_t t = 65537;
    FheParams p = FheParams::n8192(3);
    const size_t n = p.n();
    Context ctx(p, 0);
    Evaluator ev(ctx);
    KeyGenerator kg(ctx, TestSeed{17});
    Encryptor enc(ctx, kg.secret_key(), TestSeed{18});
    Decryptor dec(ctx, kg.secret_key());
    BatchEncoder be(ctx, t);
    std::vector<uint64_t> x(n), got(n), dm(n);
    std::vector<uint32_t> w(n), b(n);
    for (size_t i = 0; i < n; ++i) { x[i] = rnd(t); w[i] = (uint32_t)rnd(256); b[i] = (uint32_t)rnd(t); }
    std::vector<int64_t> cx(n);
    be.encode(x.data(), cx.data());
    Ciphertext ct(ctx, 2, 1), prod(ctx, 2, 1), sum(ctx, 2, 1);
    enc.encrypt_exact(cx.data(), t, ct);
    uint32_t* d = nullptr;                                   // the operands start life on the device
    CHECK(hipMalloc(reinterpret_cast<void**>(&d), 2 * n * 4) == hipSuccess);
    CHECK(hipMemcpy(d, w.data(), n * 4, hipMemcpyHostToDevice) == hipSuccess);
    CHECK(hipMemcpy(d + n, b.data(), n * 4, hipMemcpyHostToDevice) == hipSuccess);
    Plaintext pw(ctx, 1);
    be.encode_device(d, 1, pw, /*to_ntt=*/true);
    ExactPlaintext pb(ctx, t, 1);
    pb.set_slots_device(be, d + n);
    ev.transform_to_ntt_inplace(ct);
    ev.multiply_plain(ct, pw, prod);
    ev.transform_from_ntt_inplace(prod);
    ev.add_plain_exact(prod, pb, sum);
    ctx.synchronize();
    dec.decrypt_exact(prod, t, dm.data());
    be.decode(dm.data(), got.data());
    size_t bad = 0;
    for (size_t i = 0; i < n; ++i) bad += got[i] != x[i] * w[i] % t;
    CHECK(bad == 0);
    dec.decrypt_exact(sum, t, dm.data());
    be.decode(dm.data(), got.data());
    bad = 0;
    for (size_t i = 0; i < n; ++i) bad += got[i] != (x[i] * w[i] + b[i]) % t;
    CHECK(bad == 0);
    (void)hipFree(d);
}

int main() {
    try {
        word_for_word(65537);
        word_for_word(4293918721ull);   // a prime = 1 mod 2^17 just under 2^32
        request_time_operands();
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    return finish("encode C++ facade OK");
}
