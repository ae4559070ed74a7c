// fhe_bigint.h - private to the facade: little-endian multiword unsigned integers, just enough for CRT composition of <= 1024 limbs.
// Host-only, no HIP.
#pragma once
#include <cstdint>
#include <vector>

namespace deeppowers {
namespace fhe {
namespace detail __attribute__((visibility("hidden"))) {

typedef unsigned __int128 u128;
typedef std::vector<uint64_t> Big;

inline void big_mul_small(Big& a, uint64_t m) {
    u128 carry = 0;
    for (auto& w : a) { u128 t = (u128)w * m + carry; w = (uint64_t)t; carry = t >> 64; }
    if (carry) a.push_back((uint64_t)carry);
}
inline void big_add(Big& a, const Big& b) {
    if (a.size() < b.size()) a.resize(b.size(), 0);
    u128 carry = 0;
    for (size_t i = 0; i < a.size(); ++i) { u128 t = (u128)a[i] + (i < b.size() ? b[i] : 0) + carry; a[i] = (uint64_t)t; carry = t >> 64; }
    if (carry) a.push_back((uint64_t)carry);
}
inline int big_cmp(const Big& a, const Big& b) {
    size_t n = a.size() > b.size() ? a.size() : b.size();
    for (size_t i = n; i-- > 0;) {
        uint64_t x = i < a.size() ? a[i] : 0, y = i < b.size() ? b[i] : 0;
        if (x != y) return x < y ? -1 : 1;
    }
    return 0;
}
inline Big big_sub(const Big& a, const Big& b) {  // a >= b
    Big r(a.size(), 0);
    uint64_t borrow = 0;
    for (size_t i = 0; i < a.size(); ++i) {
        u128 t = (u128)a[i] - (i < b.size() ? b[i] : 0) - borrow;
        r[i] = (uint64_t)t; borrow = (uint64_t)(t >> 64) & 1;
    }
    return r;
}
inline uint64_t big_divmod_small(Big& a, uint64_t m) {  // a = floor(a / m), returns a mod m
    u128 rem = 0;
    for (size_t i = a.size(); i-- > 0;) { u128 cur = (rem << 64) | a[i]; a[i] = (uint64_t)(cur / m); rem = cur % m; }
    while (a.size() > 1 && a.back() == 0) a.pop_back();
    return (uint64_t)rem;
}
inline uint64_t big_mod_small(const Big& a, uint64_t m) { Big t(a); return big_divmod_small(t, m); }
inline void big_shr_round(Big& a, unsigned sh) {  // a = floor((a + 2^(sh-1)) / 2^sh)
    if (sh) {
        Big half((sh - 1) / 64 + 1, 0);
        half[(sh - 1) / 64] = 1ull << ((sh - 1) % 64);
        big_add(a, half);
    }
    const size_t ws = sh / 64, bs = sh % 64;
    Big r(a.size() > ws ? a.size() - ws : 1, 0);
    for (size_t i = 0; i + ws < a.size(); ++i) {
        r[i] = a[i + ws] >> bs;
        if (bs && i + ws + 1 < a.size()) r[i] |= a[i + ws + 1] << (64 - bs);
    }
    a = r;
}
inline unsigned big_bits(const Big& a) {   // bit length: 0 for 0, floor(log2 a) + 1 otherwise
    for (size_t i = a.size(); i-- > 0;)
        if (a[i]) return (unsigned)(i * 64) + (unsigned)(64 - __builtin_clzll(a[i]));
    return 0;
}
inline Big modulus_product(const std::vector<uint64_t>& moduli) {   // Q
    Big Q{1};
    for (uint64_t q : moduli) big_mul_small(Q, q);
    return Q;
}
// x = v0 + v1 q0 + v2 q0 q1 + ... from its mixed-radix (Garner) digits
inline Big big_from_mixed_radix(const std::vector<uint64_t>& moduli, const std::vector<uint64_t>& digit) {
    Big x{0};
    for (size_t i = moduli.size(); i-- > 0;) { big_mul_small(x, moduli[i]); big_add(x, Big{digit[i]}); }
    return x;
}

}  // namespace detail
}  // namespace fhe
}  // namespace deeppowers
