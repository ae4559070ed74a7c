// fhe_sampler.h - private to the facade: the generator behind every secret key, error and seed.  Host-only, no HIP (tests/cpp/sampler_stream.cpp drives it).
// Default: ChaCha20 (chacha20.h) keyed with 48 bytes from the operating system's CSPRNG (getrandom(2), /dev/urandom as fallback) - uniform values by
// rejection sampling, ternary secrets, centred-binomial errors (eta = 21: sigma = 3.24, |e| <= 21).  The TestSeed constructors of the public classes
// switch to SplitMix64 so that tests and examples are reproducible; that generator is invertible with 64 bits of state and must never protect real data.
#pragma once
#include <sys/random.h>

#include <cerrno>
#include <cstdio>
#include <cstring>

#include "chacha20.h"
#include "deeppowers/fhe.hpp"

namespace deeppowers {
namespace fhe {
namespace detail __attribute__((visibility("hidden"))) {

typedef unsigned __int128 u128;

inline void secure_wipe(void* p, size_t bytes) {   // (volatile: the stores to a dying buffer must not be optimised away)
    volatile unsigned char* wipe = static_cast<volatile unsigned char*>(p);
    for (size_t i = 0; i < bytes; ++i) wipe[i] = 0;
}

struct Sampler {
    static constexpr size_t kKeyBytes = 48;
    bool secure = true;
    uint64_t sm = 0;            // SplitMix64 state (testing)
    dpfhe::ExpandKey key = {};  // ChaCha20 key
    uint32_t st[4] = {};        // ChaCha20 words 12..15: a 64-bit block counter | a 64-bit nonce
    uint32_t blk[16] = {};
    int used = 16;              // 32-bit words of blk already handed out

    Sampler() { key_from_os(); }
    explicit Sampler(TestSeed seed) : secure(false), sm(seed.value) {}
    // the secure path under a caller's key material: bytes 0..31 the key, 32..39 the nonce, 40..47 the counter's start
    explicit Sampler(const unsigned char (&buf)[kKeyBytes]) { set_key(buf); }

    void set_key(const unsigned char (&buf)[kKeyBytes]) {
        std::memcpy(key.w, buf, 32);
        std::memcpy(st + 2, buf + 32, 8);
        // the last 8 bytes perturb the counter start so that equal (key, nonce) - impossible in practice - still differ
        std::memcpy(st, buf + 40, 8);
        used = 16;
    }
    void key_from_os() {
        unsigned char buf[kKeyBytes];
        size_t got = 0;
        while (got < sizeof(buf)) {
            const ssize_t r = getrandom(buf + got, sizeof(buf) - got, 0);
            if (r > 0) { got += (size_t)r; continue; }
            if (r < 0 && errno == EINTR) continue;
            break;
        }
        if (got < sizeof(buf)) {   // kernels without getrandom(2)
            FILE* f = std::fopen("/dev/urandom", "rb");
            if (f) { got += std::fread(buf + got, 1, sizeof(buf) - got, f); std::fclose(f); }
        }
        if (got < sizeof(buf)) throw Exception(ErrorCode::RUNTIME_ERROR, "no operating-system randomness available (getrandom, /dev/urandom)");
        set_key(buf);
        secure_wipe(buf, sizeof(buf));
    }
    void refill() {   // one ChaCha20 block; words 12, 13 are the block function's (counter, n0), here one 64-bit counter
        dpfhe::chacha20_block(key, st[0], st[1], st[2], st[3], blk);
        if (++st[0] == 0) ++st[1];
        used = 0;
    }
    uint64_t next() {
        if (!secure) {   // SplitMix64 (same generator as the synthetic-data spec)
            sm += 0x9E3779B97F4A7C15ull;
            uint64_t z = sm;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            return z ^ (z >> 31);
        }
        if (used > 14) refill();
        const uint64_t v = (uint64_t)blk[used] | ((uint64_t)blk[used + 1] << 32);
        used += 2;
        return v;
    }
    // uniform in [0, bound): rejection sampling on the smallest covering power of two (no modulo bias)
    uint64_t below(uint64_t bound) {
        if (bound <= 1) return 0;
        const uint64_t mask = ~0ull >> __builtin_clzll(bound - 1);
        for (;;) {
            const uint64_t v = next() & mask;
            if (v < bound) return v;
        }
    }
    int ternary() { return (int)below(3) - 1; }
    // centred binomial, eta = 21: popcount(21 bits) - popcount(21 bits); variance 10.5 (sigma 3.24)
    int64_t error() {
        const uint64_t v = next();
        return (int64_t)__builtin_popcountll(v & 0x1fffffull) - (int64_t)__builtin_popcountll((v >> 21) & 0x1fffffull);
    }
};

inline uint64_t lift_signed(int64_t v, uint64_t q) { return v >= 0 ? (uint64_t)v % q : q - ((uint64_t)(-v) % q == 0 ? q : (uint64_t)(-v) % q); }
inline uint64_t powmod(uint64_t b, uint64_t e, uint64_t q) {
    uint64_t r = 1;
    for (b %= q; e; e >>= 1) { if (e & 1) r = (uint64_t)((u128)r * b % q); b = (uint64_t)((u128)b * b % q); }
    return r;
}

// 32 bytes from the generator (the OS CSPRNG, or the deterministic TestSeed stream)
inline void draw_seed(Sampler& rng, Seed& out) {
    for (int i = 0; i < 4; ++i) {
        const uint64_t v = rng.next();
        std::memcpy(out.bytes + 8 * i, &v, 8);
    }
}

}  // namespace detail
}  // namespace fhe
}  // namespace deeppowers
