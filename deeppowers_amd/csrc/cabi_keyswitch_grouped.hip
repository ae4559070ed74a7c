// cabi_keyswitch_grouped.hip - the C ABI's hybrid key switching with grouped digits and several special primes (keyswitch_grouped.h).  The transforms, the key
// inner product and the constants of a base extension are borrowed from their own units (cabi.h), which also lists the other units and states the ABI's conventions.
#include "cabi.h"
#include "keyswitch_grouped.h"

// the product of limbs [l0, l0 + count) as little-endian 64-bit words (host; at most 10 primes below 2^60)
static std::vector<uint64_t> limb_product(const dpfhe_ctx* c, uint32_t l0, uint32_t count) {
    std::vector<uint64_t> r{1};
    for (uint32_t i = 0; i < count; ++i) {
        unsigned __int128 carry = 0;
        for (uint64_t& w : r) {
            const unsigned __int128 t = (unsigned __int128)w * c->moduli[l0 + i] + carry;
            w = (uint64_t)t;
            carry = t >> 64;
        }
        if (carry) r.push_back((uint64_t)carry);
    }
    return r;
}
static bool less_than(const std::vector<uint64_t>& a, const std::vector<uint64_t>& b) {   // (no leading zero words on either side)
    if (a.size() != b.size()) return a.size() < b.size();
    for (size_t i = a.size(); i-- > 0;)
        if (a[i] != b[i]) return a[i] < b[i];
    return false;
}

// The device table of (context, alpha): BaseExtArgs[groups + 1] - block d: digit group d onto all L limbs; the last block: the special limbs onto the data limbs,
// with P^-1 (dpfhe_scale_round's constants at multiplier 1).  Made ONCE per (context, alpha), by the first call that gets this far - a call with batch == 0 is
// the warm-up that does nothing else: the verdict P >= max_d D_d, the constants (host only, before the device is touched), then one synchronous upload under
// a guard of its own.  Every later call reads the pointer and nothing else.  (cabi.h: dpfhe_rotate_sum_hoisted_grouped shares the table.)
int grouped_table(dpfhe_ctx* c, uint32_t alpha, unsigned groups, const char* what) {
    std::lock_guard<std::mutex> lock(c->grouped_mutex);
    if (c->grouped_tabs[alpha].load(std::memory_order_relaxed)) return DPFHE_SUCCESS;
    const uint32_t L = c->n_limbs, Ld = L - alpha;
    auto width = [&](unsigned d) { return Ld - d * alpha < alpha ? Ld - d * alpha : alpha; };
    const std::vector<uint64_t> P = limb_product(c, Ld, alpha);   // the division by P tames the switching noise only when no digit is larger than P
    for (unsigned d = 0; d < groups; ++d)
        if (less_than(P, limb_product(c, d * alpha, width(d)))) return fail(DPFHE_INVALID_STATE, what, "the special primes' product is smaller than a digit group's");
    std::vector<unsigned char> host((groups + 1) * sizeof(BaseExtArgs));
    BaseExtArgs* a = reinterpret_cast<BaseExtArgs*>(host.data());
    for (unsigned d = 0; d < groups; ++d)
        if (int rc = fill_base_ext_args(c, 0, d * alpha, width(d), 0, L, 1, a[d], what)) return rc;
    if (int rc = fill_base_ext_args(c, 1, Ld, alpha, 0, Ld, 1, a[groups], what)) return rc;
    DPFHE_ON_DEVICE(c, what);
    void* tab = nullptr;
    if (int rc = upload_blob(&tab, host, "dpfhe_switch_key_grouped: digit-group table upload")) return rc;
    c->grouped_tabs[alpha].store(tab, std::memory_order_release);
    return DPFHE_SUCCESS;
}

template <int NS>
static void launch_grouped_kernels(bool lift, const GroupedKsPlan& plan, hipStream_t s, u64* out, const u64* a, const u64* b, int in_comps, int add_mask,
                                   const BaseExtArgs* tabs, const dpfhe_ctx* c, int n_data, int chunks) {
    const int L = (int)c->n_limbs, n = 1 << c->log2n;
    if (lift)
        hipLaunchKernelGGL((digit_group_lift_kernel<NS>), dim3((unsigned)plan.lift_grid), dim3(256), 0, s, out, a, in_comps, tabs, c->lc, n_data, L, plan.groups, n, chunks);
    else
        hipLaunchKernelGGL((grouped_moddown_kernel<NS>), dim3((unsigned)plan.moddown_grid), dim3(256), 0, s, out, a, b, in_comps, add_mask, tabs + plan.groups, c->lc, n_data, L, n,
                           chunks);
}
// one kernel pair per number of special primes (the digit arrays are indexed at compile time)
void launch_grouped(uint32_t alpha, bool lift, const GroupedKsPlan& plan, hipStream_t s, u64* out, const u64* a, const u64* b, int in_comps, int add_mask,
                    const BaseExtArgs* tabs, const dpfhe_ctx* c, int n_data, int chunks) {
    static_assert(kGroupedMaxSpecial == 10, "one case per number of special primes below");
#define GROUPED_CASE(NS) case NS: launch_grouped_kernels<NS>(lift, plan, s, out, a, b, in_comps, add_mask, tabs, c, n_data, chunks); break;
    switch (alpha) { GROUPED_CASE(1) GROUPED_CASE(2) GROUPED_CASE(3) GROUPED_CASE(4) GROUPED_CASE(5) GROUPED_CASE(6) GROUPED_CASE(7) GROUPED_CASE(8) GROUPED_CASE(9)
                     GROUPED_CASE(10) default: break; }
#undef GROUPED_CASE
}

extern "C" int dpfhe_switch_key_grouped(dpfhe_ctx* c, uint64_t* d_out2, const uint64_t* d_in, uint32_t in_components, uint32_t n_special, const uint64_t* d_key,
                                        uint64_t* d_digits, uint64_t* d_work, size_t batch, void* stream) {
    const char* what = "dpfhe_switch_key_grouped";
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, what, "null context");
    const uint32_t L = c->n_limbs, alpha = n_special;
    if (alpha == 0 || alpha > (uint32_t)kGroupedMaxSpecial || alpha >= L) return fail(DPFHE_INVALID_ARGUMENT, what, "n_special must be in [1, 10] and leave a data limb");
    if (in_components != 2 && in_components != 3) return fail(DPFHE_INVALID_ARGUMENT, what, "in_components must be 2 or 3");
    if (L > (uint32_t)kBxMaxDst) return fail(DPFHE_INVALID_ARGUMENT, what, "at most 20 limbs (the limit of dpfhe_base_extend)");
    const uint32_t Ld = L - alpha, groups = (Ld + alpha - 1) / alpha;
    const bool made = c->grouped_tabs[alpha].load(std::memory_order_acquire) != nullptr;
    if (batch == 0) return made ? (int)DPFHE_SUCCESS : grouped_table(c, alpha, groups, what);   // (the warm-up)
    if (!d_out2 || !d_in || !d_key || !d_digits || !d_work || misaligned(d_out2) || misaligned(d_in) || misaligned(d_key) || misaligned(d_digits) || misaligned(d_work))
        return fail(DPFHE_INVALID_ARGUMENT, what, "null or misaligned buffer");
    const size_t n = (size_t)1 << c->log2n;
    const int chunks = chunks_of(n);
    const GroupedKsPlan plan = GroupedKsMap::plan(batch, L, alpha, n);
    if (!plan.ok || batch > kMaxGrid / ((size_t)L * chunks) || !ntt_grid_fits(c, batch * groups * L) || !ntt_grid_fits(c, batch * 2 * L))
        return fail(DPFHE_INVALID_ARGUMENT, what, "batch too large for one launch");
    {   // the three written buffers overlap nothing
        const uint64_t* bufs[] = {d_out2, d_digits, d_work, d_in, d_key};
        const size_t sizes[] = {batch * 2 * Ld * n, batch * groups * L * n, batch * 2 * L * n, batch * in_components * Ld * n, (size_t)groups * 2 * L * n};
        for (int a = 0; a < 3; ++a)
            for (int b = a + 1; b < 5; ++b)
                if (overlaps(bufs[a], sizes[a], bufs[b], sizes[b])) return fail(DPFHE_INVALID_ARGUMENT, what, "buffers must not overlap");
    }
    if (!made)
        if (int rc = grouped_table(c, alpha, groups, what)) return rc;
    const BaseExtArgs* tabs = static_cast<const BaseExtArgs*>(c->grouped_tabs[alpha].load(std::memory_order_acquire));
    DPFHE_ON_DEVICE(c, what);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // 1. the centred digit of every group on every limb of Q P;  2. their transforms
    launch_grouped(alpha, true, plan, s, d_digits, d_in, nullptr, (int)in_components, 0, tabs, c, (int)Ld, chunks);
    if (int rc = check_launch("digit group lift kernel launch")) return rc;
    if (int rc = ntt_launch_items(c, false, d_digits, d_digits, batch * groups, 0, s)) return rc;
    // 3. sum_d digit_d (.) key_d over Q P;  4. back to coefficients
    launch_key_inner_product(c, batch * L * (size_t)chunks, s, d_work, d_digits, d_key, (int)groups, chunks);
    if (int rc = check_launch("key inner product kernel launch")) return rc;
    if (int rc = ntt_launch_items(c, true, d_work, d_work, batch * 2, 0, s)) return rc;
    // 5. divide by P with rounding, add (c0, c1 or 0)
    launch_grouped(alpha, false, plan, s, d_out2, d_work, d_in, (int)in_components, in_components == 3 ? 3 : 1, tabs, c, (int)Ld, chunks);
    return check_launch("grouped division launch");
}
