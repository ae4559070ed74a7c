// GPU test of slot sums on grouped-digit keys in the C++ facade (GroupedKeySwitcher::rotate_sum_range, SlotSum's GroupedKeySwitcher constructor) at N = 4096,
// four data limbs under two special primes, three tokens of the approximate family, block 8 at radix 2 (three stages of one element) and at radix 8 (one
// stage of seven): every decoded slot within SlotSum::error_bound of the float64 sum, and at radix 2 within that bound plus the HybridKeySwitcher form's own
// of the HybridKeySwitcher SlotSum on the same ciphertexts (both bound the distance to the same sum).  Built and run by tests/test_gpu_rotate_sum_grouped.py.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include "../facade_test.h"

using namespace deeppowers::fhe;
using namespace facade_test;
typedef std::complex<double> cplx;

static const unsigned kLog2N = 12;
static const size_t kLd = 4, kTokens = 3, kN = (size_t)1 << kLog2N, kRow = kN / 2, kBlock = 8;
static const uint32_t kAlpha = 2;
static const double kScale = std::ldexp(1.0, 50), kX = 1.0, kFresh = 21.0 + 0.5 + 8.0 * kLog2N * std::ldexp(1.0, -53) * kScale * kX;

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

int main() {
    try {
        const FheParams pe = extended();
        FheParams pd = pe;
        pd.moduli.resize(kLd); pd.psi.resize(kLd);
        Context ext(pe, 0), data(pd, 0);
        KeyGenerator kg(ext, TestSeed{51});
        SecretKey sk(data, kg.secret_key().coefficients());
        Encryptor enc(data, sk, TestSeed{52});
        Decryptor dec(data, sk);
        ComplexEncoder cenc(data);
        GroupedKeySwitcher gks(ext, kAlpha);
        HybridKeySwitcher hks(data, sk, pe.moduli.back(), pe.psi.back(), TestSeed{53});

        SplitMix64 rng;
        rng.state = 5100;
        std::vector<double> x(kTokens * kRow);
        std::vector<int64_t> msg(kTokens * kN), out(kTokens * kN);
        std::vector<cplx> z(kRow), zh(kRow);
        for (size_t t = 0; t < kTokens; ++t) {
            for (size_t i = 0; i < kRow; ++i) z[i] = cplx(x[t * kRow + i] = 0.5 + 0.5 * rng.unit(), 0.0);
            cenc.encode(z.data(), kScale, &msg[t * kN]);
        }
        Ciphertext cx(data, 2, kTokens), cy(data, 2, kTokens), ch(data, 2, kTokens);
        enc.encrypt(msg.data(), 0, cx);
        SlotSum hybrid(hks, kBlock);
        hybrid.apply(cx, ch);
        data.synchronize();
        std::vector<int64_t> hout(kTokens * kN);
        dec.decrypt(ch, 0, hout.data());
        const double hbound = hybrid.error_bound(kScale, kX, kFresh);

        for (size_t radix : {(size_t)2, (size_t)8}) {
            SlotSum sum(gks, kg, kBlock, 1, radix);
            CHECK(sum.radix() == radix && sum.steps() == (radix == 2 ? 3u : 1u) && sum.galois_elements().size() == (radix == 2 ? 3u : 7u));
            if (radix == 2) CHECK(sum.galois_elements() == hybrid.galois_elements());
            sum.apply(cx, cy);
            data.synchronize();
            dec.decrypt(cy, 0, out.data());
            // the header's derivation with noise_bound() in K + H's place, written out
            const double N = (double)kN, H = (N + 1) / 2, B = (double)kBlock, KH = gks.noise_bound(), u8 = 8.0 * kLog2N * std::ldexp(1.0, -53);
            const double pre = N * (B * kFresh + (radix == 2 ? (B - 1) * KH : (B - 1) * (KH - H) + H)) / kScale, bound = sum.error_bound(kScale, kX, kFresh);
            CHECK(bound == pre + u8 * N * (B * kX + pre));
            double worst = 0, apart = 0, smax = 0;
            for (size_t t = 0; t < kTokens; ++t) {
                cenc.decode(&out[t * kN], kScale, z.data());
                cenc.decode(&hout[t * kN], kScale, zh.data());
                for (size_t i = 0; i < kRow; ++i) {
                    double acc = 0;
                    for (size_t j = 0; j < kBlock; ++j) acc += x[t * kRow + (i + j) % kRow];
                    smax = std::max(smax, acc);
                    worst = std::max(worst, std::max(std::fabs(z[i].real() - acc), std::fabs(z[i].imag())));
                    apart = std::max(apart, std::abs(z[i] - zh[i]));
                }
            }
            std::printf("grouped keys, block %zu radix %zu: max|sum| %.3f, max error 2^%.2f, error_bound 2^%.2f; from the one-prime form 2^%.2f (its bound 2^%.2f)\n", kBlock,
                        radix, smax, std::log2(worst), std::log2(bound), std::log2(apart), std::log2(hbound));
            CHECK(smax >= 1.0 && worst <= bound && worst > 0);
            if (radix == 2) CHECK(apart <= bound + hbound);
        }
        PolyBuffer none(ext, gks.groups(), 2, true);
        expect_error(ErrorCode::INVALID_ARGUMENT, [&] { gks.rotate_sum_range(cx, 0, 2, std::vector<uint32_t>{3, 9}, none, cy, 0); }, "rotate_sum_range, two elements, one key");
    } catch (const std::exception& e) {
        std::printf("FAIL exception: %s\n", e.what());
        return 1;
    }
    return finish("slot sum grouped C++ facade OK");
}
