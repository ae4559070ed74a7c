// Every word the C++ facade produces under a TestSeed, written to files so that tests/test_gpu_facade_digests.py can hash them: keys (plain and
// seeded), symmetric and public-key encryption (approximate and exact, plain and seeded), decryption and noise budgets, a compact result, a
// re-randomised result, the hybrid key switcher's outputs and both slot encoders.  It uses the public header only (and the HIP runtime for one device
// buffer), so the same source builds against any version of the library; the order of the calls on each generator is part of the test.
//   facade_digests <outdir> <log2_n> <q0> <psi0> <q1> <psi1> ... : the LAST (q, psi) pair is the key switcher's special prime.
// Exit code 0 = everything was written and the decryptions gave the messages back.
#include <hip/hip_runtime_api.h>

#include <complex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "facade_test.h"

using namespace deeppowers::fhe;
using namespace facade_test;

static std::string g_outdir;
static Lcg rnd{2024};

static void dump(const char* name, const void* data, size_t bytes) {
    const std::string path = g_outdir + "/" + name + ".bin";
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(data, 1, bytes, f) != bytes) { std::printf("FAIL cannot write %s\n", path.c_str()); ++failures; }
    if (f) std::fclose(f);
}
static void dump(const char* name, const PolyBuffer& b) {
    std::vector<uint64_t> w(b.words() + 1);
    b.copy_to_host(w.data());
    w[b.words()] = b.is_ntt() ? 1 : 0;   // the domain flag is part of what the facade produces
    dump(name, w.data(), w.size() * sizeof(uint64_t));
}
static void dump_text(const char* name, const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    const int len = std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    std::printf("%s = %s\n", name, buf);
    dump(name, buf, (size_t)len);
}

// decrypt and decrypt_exact of one ciphertext; `exact` says which of the two must give the messages back
static void decrypt_both(Decryptor& dec, const char* name, const Ciphertext& ct, const std::vector<int64_t>& m, bool exact) {
    const size_t count = m.size();
    // 2^30 is the scale of the approximate encryptions; an exact one carries floor(Q / t) m, about 2^164: 2^120 brings it below 62 bits
    std::vector<int64_t> approx(count);
    dec.decrypt(ct, exact ? 120 : 30, approx.data());
    dump((std::string(name) + ".decrypt").c_str(), approx.data(), count * sizeof(int64_t));
    std::vector<uint64_t> ex(count);
    dec.decrypt_exact(ct, T_MOD, ex.data());
    dump((std::string(name) + ".decrypt_exact").c_str(), ex.data(), count * sizeof(uint64_t));
    size_t bad = 0;
    for (size_t i = 0; i < count; ++i) bad += exact ? ex[i] != (uint64_t)m[i] : approx[i] != m[i];
    if (bad) { std::printf("FAIL %s: %zu of %zu values do not decrypt to the message\n", name, bad, count); ++failures; }
}

static void run(const FheParams& p, uint64_t special, uint64_t special_psi) {
    const size_t n = p.n(), B = 2;
    const uint32_t g_rot = 3, g_conj = (uint32_t)(2 * n - 1);
    Context ctx(p, 0);
    Evaluator ev(ctx);

    // ---- KeyGenerator(TestSeed{41}) ----
    KeyGenerator kg(ctx, TestSeed{41});
    const SecretKey& sk = kg.secret_key();
    dump("secret_key", sk.coefficients().data(), n);
    Seed seed;
    {
        RelinKeys rk(ctx);
        kg.create_relin_keys(rk);
        dump("relin_keys", rk);
        GaloisKeys g3(ctx, g_rot), gc(ctx, g_conj);
        kg.create_galois_keys(g3);
        dump("galois_keys_3", g3);
        kg.create_galois_keys(gc);
        dump("galois_keys_conj", gc);
    }
    PublicKey pk(ctx);
    kg.create_public_key(pk);
    dump("public_key", pk);
    {
        RelinKeys rk(ctx);
        kg.create_relin_keys_seeded(rk, seed);
        dump("relin_keys_seeded", rk);
        dump("relin_keys_seeded.seed", seed.bytes, 32);
        GaloisKeys g3(ctx, g_rot);
        kg.create_galois_keys_seeded(g3, seed);
        dump("galois_keys_3_seeded", g3);
        dump("galois_keys_3_seeded.seed", seed.bytes, 32);
        PublicKey pks(ctx);
        kg.create_public_key_seeded(pks, seed);
        dump("public_key_seeded", pks);
        dump("public_key_seeded.seed", seed.bytes, 32);
    }

    // ---- messages ----
    std::vector<int64_t> m_small(B * n), m_exact(B * n);
    for (auto& v : m_small) v = (int64_t)rnd(2001) - 1000;
    for (auto& v : m_exact) v = (int64_t)rnd(T_MOD);

    // ---- Encryptor(sk, TestSeed{42}) ----
    Encryptor enc_sk(ctx, sk, TestSeed{42});
    Ciphertext sk_approx(ctx, 2, B), sk_exact(ctx, 2, B), sk_approx_seeded(ctx, 2, B), sk_exact_seeded(ctx, 2, B);
    enc_sk.encrypt(m_small.data(), 30, sk_approx);
    dump("sk_encrypt", sk_approx);
    enc_sk.encrypt_exact(m_exact.data(), T_MOD, sk_exact);
    dump("sk_encrypt_exact", sk_exact);
    enc_sk.encrypt_seeded(m_small.data(), 30, sk_approx_seeded, seed);
    dump("sk_encrypt_seeded", sk_approx_seeded);
    dump("sk_encrypt_seeded.seed", seed.bytes, 32);
    enc_sk.encrypt_exact_seeded(m_exact.data(), T_MOD, sk_exact_seeded, seed);
    dump("sk_encrypt_exact_seeded", sk_exact_seeded);
    dump("sk_encrypt_exact_seeded.seed", seed.bytes, 32);

    // ---- Encryptor(pk, TestSeed{43}) ----
    Encryptor enc_pk(ctx, pk, TestSeed{43});
    Ciphertext pk_approx(ctx, 2, B), pk_exact(ctx, 2, B);
    enc_pk.encrypt(m_small.data(), 30, pk_approx);
    dump("pk_encrypt", pk_approx);
    enc_pk.encrypt_exact(m_exact.data(), T_MOD, pk_exact);
    dump("pk_encrypt_exact", pk_exact);

    // ---- Decryptor ----
    Decryptor dec(ctx, sk);
    decrypt_both(dec, "sk_encrypt", sk_approx, m_small, false);
    decrypt_both(dec, "sk_encrypt_exact", sk_exact, m_exact, true);
    decrypt_both(dec, "sk_encrypt_seeded", sk_approx_seeded, m_small, false);
    decrypt_both(dec, "sk_encrypt_exact_seeded", sk_exact_seeded, m_exact, true);
    decrypt_both(dec, "pk_encrypt", pk_approx, m_small, false);
    decrypt_both(dec, "pk_encrypt_exact", pk_exact, m_exact, true);
    dump_text("sk_encrypt_exact.noise_budget_bits", "%a", dec.noise_budget_bits(sk_exact, T_MOD));
    dump_text("pk_encrypt_exact.noise_budget_bits", "%a", dec.noise_budget_bits(pk_exact, T_MOD));
    {
        const auto w = CompactCiphertext::recommended_bits(p.log2_n, T_MOD);
        CompactCiphertext cc(ctx, B, w.first, w.second);
        ev.compact(pk_exact, cc);
        ctx.synchronize();
        std::vector<uint8_t> bytes(cc.bytes());
        cc.copy_to_host(bytes.data());
        dump("compact", bytes.data(), bytes.size());
        std::vector<uint64_t> got(B * n);
        dec.decrypt_exact(cc, T_MOD, got.data());
        dump("compact.decrypt_exact", got.data(), got.size() * sizeof(uint64_t));
        size_t bad = 0;
        for (size_t i = 0; i < B * n; ++i) bad += got[i] != (uint64_t)m_exact[i];
        CHECK(bad == 0);
        dump_text("compact.noise_budget_bits", "%a", dec.noise_budget_bits(cc, T_MOD));
    }

    // ---- Rerandomizer(pk, TestSeed{44}) ----
    {
        Rerandomizer rr(ctx, pk, TestSeed{44});
        dump_text("max_flood_bits", "%u", rr.max_flood_bits(T_MOD));
        CHECK(100 <= rr.max_flood_bits(T_MOD));
        std::vector<uint64_t> w(sk_exact.words());
        sk_exact.copy_to_host(w.data());
        Ciphertext ct(ctx, 2, B);
        ct.copy_from_host(w.data());
        rr.rerandomize(ct, T_MOD, 100);
        ctx.synchronize();
        dump("rerandomize", ct);
        decrypt_both(dec, "rerandomize", ct, m_exact, true);
    }

    // ---- HybridKeySwitcher(TestSeed{45}) ----
    {
        HybridKeySwitcher hks(ctx, sk, special, special_psi, TestSeed{45});
        hks.add_galois_element(g_rot);
        hks.add_galois_element(g_conj);
        const std::vector<uint32_t> elts{g_rot, g_conj};
        Ciphertext prod(ctx, 3, B), relin(ctx, 2, B);
        ev.multiply(sk_approx, pk_approx, prod);
        hks.relinearize(prod, relin);
        ctx.synchronize();
        dump("hybrid_relinearize", relin);
        Ciphertext rot(ctx, 2, B), many(ctx, 2, B), hoisted(ctx, 2, 2 * B);
        hks.apply_galois(sk_exact, g_rot, rot);
        ctx.synchronize();
        dump("hybrid_apply_galois", rot);
        hks.apply_galois_many(sk_exact, elts, many);
        ctx.synchronize();
        dump("hybrid_apply_galois_many", many);
        hks.apply_galois_hoisted(sk_exact, 0, B, elts, hoisted, 0);
        ctx.synchronize();
        dump("hybrid_apply_galois_hoisted", hoisted);
        PolyBuffer qp(hks.extended_context(), 3 * B, 2, true);
        hks.rotate_hoisted_qp(sk_exact, 0, B, elts, qp, 0);
        ctx.synchronize();
        dump("hybrid_rotate_hoisted_qp", qp);
    }

    // ---- BatchEncoder(65537) ----
    {
        BatchEncoder be(ctx, T_MOD);
        dump_text("batch_encoder.root", "%llu", (unsigned long long)be.root());
        dump_text("batch_encoder.galois_element", "%u %u", be.galois_element(1), be.galois_element(-1));
        std::vector<uint64_t> slots(n), back(n), coeffs_mod_t(n);
        std::vector<int64_t> coeffs(n);
        for (auto& v : slots) v = rnd(T_MOD);
        be.encode(slots.data(), coeffs.data());
        dump("batch_encoder.encode", coeffs.data(), n * sizeof(int64_t));
        for (size_t i = 0; i < n; ++i) coeffs_mod_t[i] = (uint64_t)(coeffs[i] < 0 ? coeffs[i] + (int64_t)T_MOD : coeffs[i]);
        be.decode(coeffs_mod_t.data(), back.data());
        dump("batch_encoder.decode", back.data(), n * sizeof(uint64_t));
        CHECK(back == slots);
        std::vector<uint32_t> slots32(B * n);
        for (auto& v : slots32) v = (uint32_t)rnd(T_MOD);
        Plaintext pt(ctx, B);
        be.encode_device(slots32.data(), B, pt, /*to_ntt=*/true);
        ctx.synchronize();
        dump("batch_encoder.encode_device", pt);
    }

    // ---- ComplexEncoder ----
    {
        ComplexEncoder ce(ctx);
        dump_text("complex_encoder.galois_element", "%u %u %u", ce.galois_element(1), ce.galois_element(-1), ce.conjugation_element());
        std::vector<double> z(B * n);   // B vectors of N/2 (re, im) pairs
        for (auto& v : z) v = ((double)rnd(2001) - 1000.0) / 64.0;
        double* d_z = nullptr;
        CHECK(hipMalloc(reinterpret_cast<void**>(&d_z), z.size() * sizeof(double)) == hipSuccess);
        CHECK(hipMemcpy(d_z, z.data(), z.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess);
        Plaintext pt(ctx, B);
        ce.encode_device(d_z, B, 1048576.0, pt);
        ctx.synchronize();
        dump("complex_encoder.encode_device", pt);
        (void)hipFree(d_z);
    }
}

int main(int argc, char** argv) {
    if (argc < 7 || (argc - 3) % 2) {
        std::printf("usage: facade_digests <outdir> <log2_n> <q> <psi> ... <special q> <special psi>\n");
        return 2;
    }
    g_outdir = argv[1];
    FheParams p;
    p.log2_n = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    for (int i = 3; i + 1 < argc; i += 2) {
        p.moduli.push_back(std::strtoull(argv[i], nullptr, 10));
        p.psi.push_back(std::strtoull(argv[i + 1], nullptr, 10));
    }
    const uint64_t special = p.moduli.back(), special_psi = p.psi.back();
    p.moduli.pop_back(); p.psi.pop_back();
    try {
        run(p, special, special_psi);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    return finish("facade digests written");
}
