// The approximate family's static error bounds as exact doubles (%a), one line per point of a fixed grid: tests/test_approx_bounds_cpu.py compares the
// lines with tests/golden/approx_bounds.json.  The `ref` modes of the API programs print bounds to two decimals, which cannot see a changed rounding;
// this can.  Public header only, no device.  A point the library rejects prints its error code instead of a number.
#include <cstdint>
#include <cstdio>
#include <functional>
#include <vector>

#include "deeppowers/fhe.hpp"

using namespace deeppowers::fhe;

namespace {

// primes = 1 mod 2^16 just below 2^60, 2^55 and 2^50, so that every level has another qmax / P; the special prime sits just below 2^61
const std::vector<uint64_t> kData7 = {0xffffffffffc0001ull, 0xfffffffff840001ull, 0xfffffffff6a0001ull, 0x7fffffffe90001ull,
                                      0x3ffffffdf0001ull,   0x7fffffffbf0001ull,  0x3ffffffd20001ull};
const std::vector<uint64_t> kData3 = {0xffffffffffc0001ull, 0x3ffffffdf0001ull, 0x3ffffffd20001ull};
const uint64_t kSpecial = 0x1fffffffffe10001ull;
// none of these is a power of two: the products round
const double kScaleX = 0x1.23456789abcdp40, kScaleY = 0x1.0fedcba98765p35, kMaxX = 0x1.8p1, kNoise = 0x1.9p4, kNoise2 = 0x1.3p3;

void line(const char* name, const std::function<double()>& f) {
    try {
        std::printf("%s = %a\n", name, f());
    } catch (const Exception& e) {
        std::printf("%s = error %d\n", name, (int)e.code());
    }
}

}  // namespace

int main() {
    char name[160];
    for (uint32_t log2_n : {12u, 15u})
        for (const std::vector<uint64_t>* data : {&kData3, &kData7}) {
            const size_t L = data->size();
            for (size_t block : {(size_t)2, (size_t)64}) {
                std::snprintf(name, sizeof name, "SlotSum log2_n=%u limbs=%zu block=%zu", log2_n, L, block);
                line(name, [&] { return SlotSum::error_bound(log2_n, *data, kSpecial, block, kScaleX, kMaxX, kNoise); });
            }
            for (size_t degree : {(size_t)2, (size_t)7, (size_t)15}) {
                std::vector<double> coeffs(degree + 1);
                for (size_t k = 0; k <= degree; ++k) coeffs[k] = (k & 1 ? -1.0 : 1.0) / ((double)k + 1.5);
                size_t levels = 0;
                while (((size_t)1 << levels) < degree) ++levels;
                std::snprintf(name, sizeof name, "ApproxPolynomial log2_n=%u limbs=%zu degree=%zu", log2_n, L, degree);
                line(name, [&] {
                    return ApproxPolynomial::error_bound(log2_n, *data, std::vector<uint64_t>(levels, kSpecial), coeffs, kScaleX, kScaleY, kMaxX, kNoise);
                });
            }
            for (size_t steps : {(size_t)1, (size_t)3}) {
                double guess = 0;
                std::snprintf(name, sizeof name, "ApproxInvSqrt::balanced_guess_scale limbs=%zu steps=%zu", L, steps);
                line(name, [&] { return guess = ApproxInvSqrt::balanced_guess_scale(kScaleX, (*data)[L - 1], (*data)[L - 2]); });
                std::snprintf(name, sizeof name, "ApproxInvSqrt log2_n=%u limbs=%zu steps=%zu", log2_n, L, steps);
                line(name, [&] {
                    return ApproxInvSqrt::error_bound(log2_n, *data, std::vector<uint64_t>(2 * steps, kSpecial), kScaleX, guess, kMaxX, 0x1.2p-1, kNoise, kNoise2);
                });
            }
            for (size_t terms : {(size_t)1, (size_t)8}) {
                std::snprintf(name, sizeof name, "ApproxProductSum log2_n=%u limbs=%zu terms=%zu", log2_n, L, terms);
                line(name, [&] { return ApproxProductSum::error_bound(log2_n, *data, kSpecial, terms, kScaleX, kScaleY, kMaxX, 0x1.4p0, kNoise, kNoise2); });
            }
        }
    return 0;
}
