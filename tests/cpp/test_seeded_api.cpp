// GPU test of the seeded ciphertexts and keys of the C++ facade (Seed, Encryptor::encrypt_seeded, KeyGenerator::create_*_seeded,
// PolyBuffer::save_seeded / load_seeded).  Built and run by tests/test_gpu_seeded.py (-m gpu).  Exit code 0 = all checks passed.
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "facade_test.h"

using namespace deeppowers::fhe;
using namespace facade_test;


static std::string save_v1(const PolyBuffer& b) { std::ostringstream os; b.save(os); return os.str(); }
static std::string save_s1(const PolyBuffer& b, const Seed& s) { std::ostringstream os; b.save_seeded(os, s); return os.str(); }

// negacyclic product in Z[X]/(X^N + 1), optionally mod t (t = 0: over the integers)
static std::vector<int64_t> negacyclic(const std::vector<int64_t>& a, const std::vector<int64_t>& b, size_t batch, size_t n, int64_t t) {
    std::vector<int64_t> r(batch * n, 0);
    for (size_t k = 0; k < batch; ++k)
        for (size_t i = 0; i < n; ++i) {
            if (!a[k * n + i]) continue;
            for (size_t j = 0; j < n; ++j) {
                int64_t pr = a[k * n + i] * b[k * n + j];
                if (t) pr %= t;
                int64_t& d = (i + j < n) ? r[k * n + i + j] : r[k * n + i + j - n];
                d = (i + j < n) ? d + pr : d - pr;
                if (t) d %= t;
            }
        }
    if (t)
        for (auto& v : r) v = (v % t + t) % t;
    return r;
}

static void approximate(const FheParams& p, size_t batch) {
    const size_t n = p.n();
    Context ctx(p, 0), ctx2(p, 0);
    Evaluator ev(ctx);
    KeyGenerator kg(ctx, TestSeed{41});
    Encryptor enc(ctx, kg.secret_key(), TestSeed{42});
    Decryptor dec(ctx, kg.secret_key());
    std::vector<int64_t> m1(batch * n), m2(batch * n), out(batch * n);
    Lcg lcg{5};
    auto rnd = [&]() { return (int64_t)lcg(201) - 100; };
    for (auto& v : m1) v = rnd();
    for (auto& v : m2) v = rnd();
    const unsigned scale = 45;

    // encrypt_seeded -> save_seeded -> load_seeded on a second context: the same words, and they decrypt to the messages
    Ciphertext c1(ctx, 2, batch), c2(ctx, 2, batch);
    Seed s1{}, s2{};
    enc.encrypt_seeded(m1.data(), scale, c1, s1);
    enc.encrypt_seeded(m2.data(), scale, c2, s2);
    CHECK(std::memcmp(s1.bytes, s2.bytes, 32) != 0);                 // one fresh seed per call
    dec.decrypt(c1, scale, out.data());
    CHECK(out == m1);
    const std::string v1 = save_v1(c1), seeded = save_s1(c1, s1);
    CHECK(seeded.size() == 80 + 8 * p.n_limbs() + 8 * batch * p.n_limbs() * n && seeded.compare(0, 8, std::string("DPFHEs1\0", 8)) == 0);
    CHECK(seeded.size() < 0.501 * v1.size());
    {
        Ciphertext back(ctx2, 2, batch);
        std::istringstream is(seeded);
        back.load_seeded(is);
        CHECK(words(back) == words(c1) && !back.is_ntt());
        SecretKey sk2(ctx2, kg.secret_key().coefficients());
        Decryptor dec_b(ctx2, sk2);
        dec_b.decrypt(back, scale, out.data());
        CHECK(out == m1);
        // the v1 reader rejects the seeded magic, the seeded reader rejects v1
        std::istringstream is2(seeded);
        expect_error(ErrorCode::INVALID_ARGUMENT, [&] { Ciphertext x(ctx2, 2, batch); x.load(is2); }, "load(DPFHEs1)");
        std::istringstream is3(v1);
        expect_error(ErrorCode::INVALID_ARGUMENT, [&] { Ciphertext x(ctx2, 2, batch); x.load_seeded(is3); }, "load_seeded(DPFHEv1)");
        std::istringstream is4(seeded.substr(0, seeded.size() - 8));
        expect_error(ErrorCode::INVALID_ARGUMENT, [&] { Ciphertext x(ctx2, 2, batch); x.load_seeded(is4); }, "load_seeded(truncated)");
    }
    // the same TestSeed gives the same seed and the same words (the testing path stays reproducible)
    {
        Encryptor again(ctx, kg.secret_key(), TestSeed{42});
        Ciphertext c(ctx, 2, batch);
        Seed sa{};
        again.encrypt_seeded(m1.data(), scale, c, sa);
        CHECK(std::memcmp(sa.bytes, s1.bytes, 32) == 0 && words(c) == words(c1));
    }
    // a stale seed never goes out: another seed, an overwritten word, a transformed buffer
    expect_error(ErrorCode::INVALID_STATE, [&] { save_s1(c1, s2); }, "save_seeded(wrong seed)");
    {
        std::vector<uint64_t> h = words(c2);
        h[p.n_limbs() * n + 3] ^= 1;    // item 0, c1, limb 0, coefficient 3
        Ciphertext c(ctx, 2, batch);
        c.copy_from_host(h.data());
        expect_error(ErrorCode::INVALID_STATE, [&] { save_s1(c, s2); }, "save_seeded(overwritten)");
        ev.transform_to_ntt_inplace(c2);
        expect_error(ErrorCode::INVALID_STATE, [&] { save_s1(c2, s2); }, "save_seeded(transformed)");
        ev.transform_from_ntt_inplace(c2);
        CHECK(save_s1(c2, s2).size() == seeded.size());
    }

    // seeded relinearisation keys: the stream's keys act word for word like the in-memory ones, and the product decrypts
    const std::vector<int64_t> want = negacyclic(m1, m2, batch, n, 0);
    Ciphertext c3(ctx, 3, batch), r_mem(ctx, 2, batch), r_load(ctx, 2, batch);
    ev.multiply(c1, c2, c3);
    RelinKeys rk(ctx);
    Seed ks{};
    kg.create_relin_keys_seeded(rk, ks);
    {
        RelinKeys rk2(ctx);
        std::string blob;
        { std::ostringstream os; rk.save_seeded(os, ks); blob = os.str(); }
        CHECK(blob.size() < 0.501 * save_v1(rk).size());
        std::istringstream is(blob);
        rk2.load_seeded(is);
        CHECK(words(rk2) == words(rk) && rk2.is_ntt());
        ev.relinearize(c3, rk, r_mem);
        ev.relinearize(c3, rk2, r_load);
        ctx.synchronize();
        CHECK(words(r_mem) == words(r_load));
        dec.decrypt(r_load, 2 * scale, out.data());
        CHECK(out == want);
    }
    // seeded Galois keys: the same for a rotation
    {
        const unsigned gscale = 100;
        Ciphertext cg(ctx, 2, batch);
        Seed sg{};
        enc.encrypt_seeded(m1.data(), gscale, cg, sg);
        const uint32_t g = 3;
        GaloisKeys gk(ctx, g), gk2(ctx, g);
        Seed gs{};
        kg.create_galois_keys_seeded(gk, gs);
        std::string blob;
        { std::ostringstream os; gk.save_seeded(os, gs); blob = os.str(); }
        std::istringstream is(blob);
        gk2.load_seeded(is);
        Ciphertext rot_mem(ctx, 2, batch), rot_load(ctx, 2, batch);
        ev.apply_galois(cg, gk, rot_mem);
        ev.apply_galois(cg, gk2, rot_load);
        ctx.synchronize();
        CHECK(words(rot_mem) == words(rot_load));
        dec.decrypt(rot_load, gscale, out.data());
        std::vector<int64_t> wantg(batch * n, 0);
        for (size_t b = 0; b < batch; ++b)
            for (size_t i = 0; i < n; ++i) {
                const size_t idx = (i * (size_t)g) & (2 * n - 1);
                if (idx < n) wantg[b * n + idx] = m1[b * n + i]; else wantg[b * n + idx - n] = -m1[b * n + i];
            }
        CHECK(out == wantg);
    }
    // seeded public key: it encrypts, the secret key decrypts; and a public-key Encryptor refuses to seed
    {
        PublicKey pk(ctx), pk2(ctx);
        Seed ps{};
        kg.create_public_key_seeded(pk, ps);
        std::string blob;
        { std::ostringstream os; pk.save_seeded(os, ps); blob = os.str(); }
        std::istringstream is(blob);
        pk2.load_seeded(is);
        CHECK(words(pk2) == words(pk));
        Encryptor penc(ctx, pk2, TestSeed{43});
        Ciphertext pc(ctx, 2, batch);
        penc.encrypt(m1.data(), scale, pc);
        dec.decrypt(pc, scale, out.data());
        CHECK(out == m1);
        Seed unused{};
        expect_error(ErrorCode::INVALID_STATE, [&] { penc.encrypt_seeded(m1.data(), scale, pc, unused); }, "public-key encrypt_seeded");
        expect_error(ErrorCode::INVALID_STATE, [&] { penc.encrypt_exact_seeded(m1.data(), 65537, pc, unused); }, "public-key encrypt_exact_seeded");
    }
}

// encrypt_exact_seeded -> ExactMultiplier -> relinearise -> decrypt_exact: the negacyclic product mod t
static void exact(size_t batch) {
    const FheParams level = FheParams::n8192(2), work = FheParams::n8192(5);
    const size_t n = level.n();
    const uint64_t t = 65537;
    Context lctx(level, 0), wctx(work, 0);
    Evaluator ev(lctx);
    KeyGenerator kg(lctx, TestSeed{51});
    Encryptor enc(lctx, kg.secret_key(), TestSeed{52});
    Decryptor dec(lctx, kg.secret_key());
    RelinKeys rk(lctx);
    Seed ks{};
    kg.create_relin_keys_seeded(rk, ks);
    std::vector<int64_t> a(batch * n), b(batch * n);
    Lcg lcg{17};
    auto rnd = [&]() { return (int64_t)lcg(t); };
    for (auto& v : a) v = rnd();
    for (auto& v : b) v = rnd();
    Ciphertext ca(lctx, 2, batch), cb(lctx, 2, batch), c3(lctx, 3, batch), cr(lctx, 2, batch);
    Seed sa{}, sb{};
    enc.encrypt_exact_seeded(a.data(), t, ca, sa);
    enc.encrypt_exact_seeded(b.data(), t, cb, sb);
    std::vector<uint64_t> dm(batch * n);
    dec.decrypt_exact(ca, t, dm.data());
    bool ok = true;
    for (size_t i = 0; i < dm.size(); ++i) ok = ok && dm[i] == (uint64_t)a[i];
    CHECK(ok);
    ExactMultiplier em(wctx, lctx, t);
    em.multiply(ca, cb, c3);
    ev.relinearize(c3, rk, cr);
    lctx.synchronize();
    dec.decrypt_exact(cr, t, dm.data());
    const std::vector<int64_t> want = negacyclic(a, b, batch, n, (int64_t)t);
    ok = true;
    for (size_t i = 0; i < dm.size(); ++i) ok = ok && dm[i] == (uint64_t)want[i];
    CHECK(ok);
}

int main() {
    approximate(FheParams::n4096_l4(), 3);
    approximate(FheParams::n8192_l6(), 2);
    exact(2);
    return finish("seeded C++ facade OK");
}
