// GPU test of the C++ facade's grouped key switching (GroupedKeySwitcher, KeyGenerator::make_grouped_key / make_grouped_galois_key) at N = 4096, four data limbs
// and two special primes (two groups of two), two items: a product of two encryptions relinearised with a grouped key for s^2 decrypts to the 3-component
// product's phase within GroupedKeySwitcher::noise_bound(), and to the plaintext product within that plus the encryptions' own noise; sigma_5 of a ciphertext
// switched with a grouped Galois key decrypts to sigma_5 of its phase within the same bound; the rejections.  Built and run by
// tests/test_gpu_switch_key_grouped_facade.py.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../facade_test.h"
#include "dpfhe.h"

using namespace deeppowers::fhe;
using namespace facade_test;

static const unsigned kLog2N = 12;
static const size_t kN = (size_t)1 << kLog2N, kLd = 4, kItems = 2;
static const uint32_t kAlpha = 2;

// the six largest chain primes, ascending: the two largest are the special ones (P >= every D_d)
static FheParams extended() {
    uint64_t special, special_psi;
    FheParams p = ring(kLog2N, kLd + kAlpha - 1, special, special_psi);
    p.moduli.push_back(special); p.psi.push_back(special_psi);
    std::vector<size_t> order(p.moduli.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return p.moduli[a] < p.moduli[b]; });
    FheParams out = p;
    for (size_t i = 0; i < order.size(); ++i) { out.moduli[i] = p.moduli[order[i]]; out.psi[i] = p.psi[order[i]]; }
    return out;
}

static int64_t worst_gap(const std::vector<int64_t>& a, const std::vector<int64_t>& b) {
    int64_t w = 0;
    for (size_t i = 0; i < a.size(); ++i) w = std::max<int64_t>(w, std::llabs(a[i] - b[i]));
    return w;
}

int main() {
    try {
        const FheParams pe = extended();
        FheParams pd = pe;
        pd.moduli.resize(kLd); pd.psi.resize(kLd);
        Context ext(pe, 0), data(pd, 0);
        KeyGenerator kg(ext, TestSeed{41});
        SecretKey sk(data, kg.secret_key().coefficients());
        Encryptor enc(data, sk, TestSeed{42});
        Decryptor dec(data, sk);
        Evaluator ev(data);
        GroupedKeySwitcher ks(ext, kAlpha);
        CHECK(ks.groups() == 2);
        PolyBuffer relin(ext, ks.groups(), 2, true), gal(ext, ks.groups(), 2, true);
        kg.make_grouped_key(kg.secret_key().ntt_squared(), kAlpha, relin);
        kg.make_grouped_galois_key(5, kAlpha, gal);

        SplitMix64 rng;
        rng.state = 4100;
        const int64_t M = 8, B = 21;
        std::vector<int64_t> m1(kItems * kN), m2(kItems * kN), want(kItems * kN), p3(kItems * kN), p2(kItems * kN);
        for (auto& v : m1) v = (int64_t)(rng.next() % (2 * M + 1)) - M;
        for (auto& v : m2) v = (int64_t)(rng.next() % (2 * M + 1)) - M;
        for (size_t t = 0; t < kItems; ++t)
            for (size_t i = 0; i < kN; ++i) {
                int64_t acc = 0;
                for (size_t j = 0; j < kN; ++j) acc += (j <= i ? 1 : -1) * m1[t * kN + j] * m2[t * kN + (i + kN - j) % kN];
                want[t * kN + i] = acc;
            }
        Ciphertext a(data, 2, kItems), b(data, 2, kItems), prod(data, 3, kItems), out(data, 2, kItems);
        enc.encrypt(m1.data(), 0, a);
        enc.encrypt(m2.data(), 0, b);
        ev.multiply(a, b, prod);
        expect_error(ErrorCode::INVALID_STATE, [&] { ks.relinearize(prod, out); }, "relinearize before set_relin_key");
        ks.set_relin_key(relin);
        ks.relinearize(prod, out);
        data.synchronize();
        dec.decrypt(prod, 0, p3.data());
        dec.decrypt(out, 0, p2.data());
        const double bound = ks.noise_bound(), fresh = (double)kN * (2.0 * M * B + B * B);
        std::printf("relinearised product: switching noise %lld against noise_bound %.1f; against the plaintext product %lld (+ fresh %.0f)\n",
                    (long long)worst_gap(p2, p3), bound, (long long)worst_gap(p2, want), fresh);
        CHECK((double)worst_gap(p2, p3) <= bound && (double)worst_gap(p2, want) <= bound + fresh && worst_gap(p2, p3) > 0);

        // sigma_5: the automorphism on the data context, then the grouped key switch
        Ciphertext rot(data, 2, kItems), sw(data, 2, kItems);
        CHECK(dpfhe_apply_galois(static_cast<dpfhe_ctx*>(data.handle()), rot.data(), a.data(), kItems * 2, 5, nullptr) == 0);
        ks.switch_key(rot, gal, sw);
        data.synchronize();
        std::vector<int64_t> pa(kItems * kN), ps(kItems * kN), moved(kItems * kN);
        dec.decrypt(a, 0, pa.data());
        dec.decrypt(sw, 0, ps.data());
        for (size_t t = 0; t < kItems; ++t)
            for (size_t i = 0; i < kN; ++i) {
                const size_t idx = (i * 5) & (2 * kN - 1);
                moved[t * kN + (idx < kN ? idx : idx - kN)] = idx < kN ? pa[t * kN + i] : -pa[t * kN + i];
            }
        std::printf("sigma_5 under a grouped Galois key: switching noise %lld against noise_bound %.1f\n", (long long)worst_gap(ps, moved), bound);
        CHECK((double)worst_gap(ps, moved) <= bound);

        expect_error(ErrorCode::INVALID_ARGUMENT, [&] { GroupedKeySwitcher k(ext, 0); }, "n_special 0");
        expect_error(ErrorCode::INVALID_ARGUMENT, [&] { GroupedKeySwitcher k(ext, 6); }, "n_special = L");
        uint64_t sp, sp_psi;
        FheParams down = ring(kLog2N, 1, sp, sp_psi);      // the chain descends: its second prime under its first
        down.moduli.push_back(sp); down.psi.push_back(sp_psi);
        Context narrow(down, 0);
        expect_error(ErrorCode::INVALID_STATE, [&] { GroupedKeySwitcher k(narrow, 1); }, "P below a data prime");
        expect_error(ErrorCode::INVALID_ARGUMENT, [&] { ks.switch_key(prod, gal, sw); }, "switch_key on 3 components");
        expect_error(ErrorCode::INVALID_ARGUMENT, [&] { kg.make_grouped_key(kg.secret_key().ntt_squared(), 3, relin); }, "key of another shape");
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    return finish("grouped key switch C++ facade OK");
}
