// The facade's generator of secret keys, errors and seeds (deeppowers_amd/csrc/fhe_sampler.h) driven on the CPU: no HIP, no library.  Prints what the
// secure path gives under a fixed 48-byte key buffer whose 64-bit block counter starts at 0xFFFFFFFE (the carry into the high word happens inside the
// window), and what the TestSeed path gives, one line per draw kind: "<generator> <kind> [<bound>] : v v v ...".  Every line starts from a fresh generator.
// tests/test_facade_sampler_cpu.py restates all of it from the definitions and compares.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fhe_sampler.h"

using deeppowers::fhe::TestSeed;
using deeppowers::fhe::detail::Sampler;

static Sampler fresh(bool secure) {
    if (!secure) return Sampler(TestSeed{7});
    unsigned char buf[Sampler::kKeyBytes];
    for (size_t i = 0; i < 40; ++i) buf[i] = (unsigned char)(7 * i + 3);   // key | nonce
    const uint64_t counter = 0xFFFFFFFEull;
    std::memcpy(buf + 40, &counter, 8);
    return Sampler(buf);
}

int main(int argc, char** argv) {
    const int count = 48;
    for (int secure = 1; secure >= 0; --secure) {
        const char* name = secure ? "chacha20" : "testseed";
        Sampler rng = fresh(secure);
        std::printf("%s next :", name);
        for (int i = 0; i < 40; ++i) std::printf(" %" PRIu64, rng.next());
        std::printf("\n");
        for (int a = 1; a < argc; ++a) {   // the bounds of below()
            const uint64_t bound = std::strtoull(argv[a], nullptr, 10);
            rng = fresh(secure);
            std::printf("%s below %" PRIu64 " :", name, bound);
            for (int i = 0; i < count; ++i) std::printf(" %" PRIu64, rng.below(bound));
            std::printf("\n");
        }
        rng = fresh(secure);
        std::printf("%s ternary :", name);
        for (int i = 0; i < count; ++i) std::printf(" %d", rng.ternary());
        std::printf("\n");
        rng = fresh(secure);
        std::printf("%s error :", name);
        for (int i = 0; i < count; ++i) std::printf(" %" PRId64, rng.error());
        std::printf("\n");
    }
    return 0;
}
