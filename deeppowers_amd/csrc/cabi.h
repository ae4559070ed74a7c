// cabi.h - what the translation units of the C ABI share (host only): the context, the error report, the argument predicates, the dispatch over
// arithmetic policies and limb classes, and the few launch functions one family borrows from another.  The units of include/dpfhe.h:
//   cabi_ctx.hip        contexts, their tables, the fused multiply's tuner, the scratch arenas, dpfhe_strerror / dpfhe_last_error
//   cabi_poly.hip       transforms, coefficient-wise operations, copy                                  (kernels_poly.h)
//   cabi_mul.hip        ciphertext multiply, its traced form, sums of products, all-pairs products     (kernels_mul.h, mul_sum.h, mul_outer.h)
//   cabi_keyswitch.hip  key switching (RNS-digit and hybrid keys), rescales, host twins of the fused rescales  (kernels_keyswitch.h)
//   cabi_rotate.hip     Galois automorphisms, batched and hoisted rotations, the rotate-and-add ladder (kernels_rotate.h, rotate_add.h)
//   cabi_linalg.hip     matrix-vector products, shard-local sums                                       (kernels_linalg.h)
//   cabi_bx.hip         base extension, scale-and-round                                                (base_ext.h; kernels in k_bx_*.hip)
//   cabi_comm.hip       the RCCL communicator
//   k_expand / k_plain_add / k_compact / k_noise / k_encode / k_cencode.hip   each newer family whole: kernel, launcher, host twin, entries
// A __global__ function of these units is defined in a header that exactly ONE of them includes, or in the unit itself; the per-policy templates of
// kernels.h are instantiated by one k_*.hip per policy.  So every kernel is built in one object (tests/test_cabi_cpu.py
// test_every_kernel_is_built_in_exactly_one_object).  Launch glue is static in its unit unless declared here.
// exports.map keeps everything below out of the dynamic symbol table.
//
// Reference seam this stands in for: none exists.  Conventions follow the
// reference's HAL: device chosen by id (/root/reference/src/api/cpp/src/deeppowers.cpp:15), raw device
// pointers (/root/reference/src/core/hal/hal.hpp:44-48), optional stream last (hal.hpp:95), errors as
// deeppowers::common::ErrorCode numbers (/root/reference/src/common/error.hpp:10-40).
// Unlike /root/reference/src/core/distributed/distributed_context.cpp:88,109 nothing here allocates,
// creates streams or synchronises per call.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/dpfhe.h"
#include "devtables.h"
#include "launch.h"
#include "scratch_pool.h"
#include "tables.h"
#include "workmap.h"

using namespace dpfhe;   // (an internal header: every unit that includes it is the library's own)

int fail(int code, const char* what, const char* detail);   // sets dpfhe_last_error() to "what: detail" and returns code (cabi_ctx.hip)
#define HIP_TRY(expr)                                                                  \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess)                                                          \
            return fail(_e == hipErrorOutOfMemory ? DPFHE_OUT_OF_MEMORY : DPFHE_DEVICE_ERROR, #expr, hipGetErrorString(_e)); \
    } while (0)

// Every compute entry point runs on the CONTEXT's device (tables and, by contract, the caller's buffers live there), whatever
// the calling thread's current device is: the guard switches to it for the duration of the call and restores the caller's
// device afterwards.  Same device: two cheap runtime queries, no switch.
struct DeviceGuard {
    int prev = -1, want = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) : want(device) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != want) err = hipSetDevice(want);
    }
    ~DeviceGuard() {
        if (prev >= 0 && prev != want) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define DPFHE_ON_DEVICE(ctx, what)                                                                            \
    DeviceGuard _guard((ctx)->device);                                                                         \
    if (_guard.err != hipSuccess) return fail(DPFHE_DEVICE_ERROR, what, hipGetErrorString(_guard.err))

// the device calls of the scratch arenas (scratch_pool.h lists them): whatever allocates, frees or waits runs under a DeviceGuard on the context's
// device; record runs inside an entry that holds one already (cabi_ctx.hip)
struct HipScratchBackend {
    using Stream = hipStream_t;
    using Event = hipEvent_t;
    int device;
    int alloc(size_t words, uint64_t*& p, const char*& detail);
    void free(uint64_t* p);
    int new_event(Event& e, const char*& detail);
    void destroy_event(Event e);
    void record(Event e, Stream s) { (void)hipEventRecord(e, s); }
    void wait(Event e);
};

// half-open byte ranges [a, a + na) and [b, b + nb) intersect
static inline bool overlaps_bytes(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + nb && b0 < a0 + na;
}
// the same for word ranges
static inline bool overlaps(const uint64_t* a, size_t na, const uint64_t* b, size_t nb) { return overlaps_bytes(a, na * 8, b, nb * 8); }

static inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
static const size_t kMaxGrid = 0x7fffffff;

struct dpfhe_ctx {
    uint32_t log2n = 0, n_limbs = 0;
    int device = 0;
    bool fold = false;
    int n_cu = 256;          // compute units of the device (launch-size caps of the streaming kernels)
    std::vector<uint64_t> moduli;   // host copy (constants of dpfhe_base_extend / dpfhe_scale_round)
    uint64_t p_special = 0;  // the LAST modulus (the special prime of hybrid key switching when this is an extended context)
    void* d_blob = nullptr;  // one allocation: LimbConst[L] | fwd | inv | last | RescaleConst[L]  (FoldArith's and ShoupArith's tables share the arrangement: ctx_layout)
    const LimbConst* lc = nullptr;   // the limb constants at the head of d_blob: what the one-pass kernels read, whichever table set below is filled
    const RescaleConst* d_rescale = nullptr;
    void* rescale2_blob = nullptr;                   // a table of its own (the blob above is pinned by digest): RescaleConst[L-2] of the first L-2 limbs relative to
    const RescaleConst* d_rescale2 = nullptr;        // limb L-2 - on an extended context the division by the last DATA prime (relin_rescale_kernel); null when L < 3
    DevTables<ShoupArith> shoup{};   // the table set of the context-wide arithmetic (with_ctx_arith): the one that matches `fold` is filled
    DevTables<FoldArith> foldt{};
    // Round 6 - per-limb arithmetic classes.  A context whose limbs are not ALL of the pinned 2^60 - d shape used to run every limb on the
    // generic (Harvey / Shoup) kernels.  Now each limb gets the fastest policy its prime admits (tables.h limb_class) for the batched transforms and
    // the fused multiply: one launch per class present, each over that class's limbs only (devtables.h DevTables::n_active / active_map).  The
    // generic tables above stay complete (every limb): the one-pass kernels read their limb constants whatever the classes are (with_ctx_arith).
    // `classes` is set when L <= 16, 8 <= log2 N <= 14 and at least one limb has a faster class than the context-wide policy.
    bool classes = false;
    int uniform_cls = kClassShoup;                    // the class ALL limbs share (kClassShoup when they differ, or when `classes` is off): which policy's KEY-SWITCHING
                                                      // kernels the context runs (with_policy below); a mixture launches them once per class (class_mixture below)
    unsigned char limb_cls[16] = {};                  // LimbClass of limb i
    unsigned long long cls_map = 0;                   // the same, 4 bits per limb
    void* lazy29_blob = nullptr;                      // the fused multiply's bit-29 twiddles (ctx_tables.h build_lazy29_blob): log2 N = 12 with a FoldArith limb, null elsewhere
    void* class_blob = nullptr;                       // ONE blob of tables whose per-limb slots are in their limb's class format (mixed_layout)
    DevTables<FoldArith> cls_fold{};                  // typed views of it; the active-limb maps are set per launch (for_each_class)
    DevTables<F64Arith> cls_f64{};
    DevTables<FoldScaledArith> cls_fscaled{};
    DevTables<F64WideArith> cls_f64w{};
    DevTables<ShoupArith> cls_shoup{};
    MixedTables mixed{};                              // the batched transforms' one-launch view (kernels.h ntt_classes_kernel)
    // scratch of the composed large-ring operations: one arena per stream that ran one, leased through StreamScratch below (policy: scratch_pool.h)
    ScratchPool<HipScratchBackend> scratch{HipScratchBackend{0}};   // (dpfhe_ctx_create sets the backend's device)
    // which form of the fused multiply dpfhe_ct_mul(flags = 0) launches (launch.h CtMulVariant): the default of the ring degree until
    // dpfhe_ctx_autotune or dpfhe_ctx_set_ct_mul_variant says otherwise.  Both forms give the same words.
    std::atomic<int> ct_mul_variant{0};
    dpfhe_tune_info tune{};           // guarded by tune_mutex (the launch path reads ct_mul_variant only)
    mutable std::mutex tune_mutex;
    std::atomic<size_t> scratch_limit_words{(size_t)1024 << 17};   // slice size of the composed large-ring operations (dpfhe_ctx_set_scratch_limit; read on the compute path)
};

// allocates *dst on the current device and copies a host blob into it; a failure frees it again, reports `what` and returns the code (cabi_ctx.hip)
int upload_blob(void** dst, const std::vector<unsigned char>& host, const char* what);

inline bool ct_mul_variant_compiled(const dpfhe_ctx* c, int v) {
    return c->fold && (c->log2n == 12 || c->log2n == 13) && v >= 0 && v < kCtMulVariants;
}

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(DPFHE_DEVICE_ERROR, what, hipGetErrorString(e));
    return DPFHE_SUCCESS;
}

// hybrid key switching: the last limb is the special prime P, the others are the data limbs
inline int check_extended(const dpfhe_ctx* c, const char* what) {
    if (c->n_limbs < 2) return fail(DPFHE_INVALID_STATE, what, "the extended context needs at least one data limb and the special prime");
    return DPFHE_SUCCESS;
}
inline int check_galois_elts(const dpfhe_ctx* c, const uint32_t* elts, size_t n, const char* what) {
    const unsigned two_n = 2u << c->log2n;
    for (size_t i = 0; i < n; ++i)
        if (!(elts[i] & 1u) || elts[i] >= two_n) return fail(DPFHE_INVALID_ARGUMENT, what, "galois elements must be odd and < 2N");
    return DPFHE_SUCCESS;
}

template <class Arith>
static const DevTables<Arith>& tables_of(const dpfhe_ctx* c);
template <>
inline const DevTables<ShoupArith>& tables_of<ShoupArith>(const dpfhe_ctx* c) { return c->shoup; }
template <>
inline const DevTables<FoldArith>& tables_of<FoldArith>(const dpfhe_ctx* c) { return c->foldt; }

// The arithmetic of the one-pass (streaming) kernels and of the other context-wide launches: FoldArith when every limb is a pinned 2^60 - d prime, ShoupArith
// otherwise; fn(FoldArith{} or ShoupArith{}) launches.  It deliberately ignores the per-limb classes (running these kernels per class is DESIGN.md
// section 8, item 2), and it is not with_policy below, which picks the key-switching kernels' tables per class.
template <class Fn>
static auto with_ctx_arith(const dpfhe_ctx* c, Fn fn) { return c->fold ? fn(FoldArith{}) : fn(ShoupArith{}); }

// the widest grid a batched transform of `npolys` residue polynomials launches fits one launch
inline bool ntt_grid_fits(const dpfhe_ctx* c, size_t npolys) {
    // split transforms (N > 16384) launch npolys * N1 sub-transforms and npolys * N2 / 256 column workgroups
    const int log_n1 = split_log_n1((int)c->log2n);
    const size_t widest = log_n1 ? ((npolys << log_n1) > (npolys << (kSplitLog2N2 - 8)) ? (npolys << log_n1) : (npolys << (kSplitLog2N2 - 8))) : npolys;
    return npolys <= kMaxGrid && widest <= kMaxGrid;
}
// One launch per arithmetic class present among the first `limbs_used` limbs of a non-uniform context (dpfhe_ctx::classes): `fn(tables)` launches
// over the class's limbs.
template <class Fn>
static int for_each_class(const dpfhe_ctx* c, size_t limbs_used, Fn fn) {
    auto restrict_to = [&](auto tb, LimbClass k) {
        int na = 0;
        unsigned long long map = 0;
        for (size_t l = 0; l < limbs_used; ++l) if (c->limb_cls[l] == (unsigned char)k) map |= (unsigned long long)l << (4 * na++);
        tb.n_limbs = (int)limbs_used;
        tb.n_active = na;
        tb.active_map = map;
        return tb;
    };
    int rc = 0;
    { auto tb = restrict_to(c->cls_fold, kClassFold); if (tb.n_active && !rc) rc = fn(tb); }
    { auto tb = restrict_to(c->cls_f64, kClassF64); if (tb.n_active && !rc) rc = fn(tb); }
    { auto tb = restrict_to(c->cls_fscaled, kClassFoldScaled); if (tb.n_active && !rc) rc = fn(tb); }
    { auto tb = restrict_to(c->cls_f64w, kClassF64Wide); if (tb.n_active && !rc) rc = fn(tb); }
    { auto tb = restrict_to(c->cls_shoup, kClassShoup); if (tb.n_active && !rc) rc = fn(tb); }
    return rc;
}

// A MIXTURE of classes: per-limb classes are on and the limbs do not all share one.  Its transform-bearing kernels launch once per class present
// (for_each_class), each on that class's view of the class blob; uniform contexts launch once (with_policy).
inline bool class_mixture(const dpfhe_ctx* c) { return c->classes && c->uniform_cls == kClassShoup; }

// The policy of the KEY-SWITCHING kernels (relin_kernel, hoisted_ks_kernel, ntt_inv_galois_kernel) of a context that is NOT a mixture: fold for the pinned
// primes; the class's own for a context whose limbs all share one class (round 6: the generic forms of those kernels with that class's transforms and
// products - an all-f64 context no longer key-switches at the generic kernels' rate); the generic policy on the generic tables otherwise.  A mixture does
// not come here: relin_launch (cabi_keyswitch.hip) / with_policy_or_classes below launch it once per class, on the class blob.  fn(tables) launches.
template <class Fn>
static int with_policy(const dpfhe_ctx* c, Fn fn) {
    if (c->fold) return fn(c->foldt);
    if (c->classes) {
        if (c->uniform_cls == kClassF64) return fn(c->cls_f64);
        if (c->uniform_cls == kClassF64Wide) return fn(c->cls_f64w);
        if (c->uniform_cls == kClassFoldScaled) return fn(c->cls_fscaled);
    }
    return fn(c->shoup);
}

// the same choice for kernels whose workgroups map through DevTables::active_map (hoisted_ks_kernel, ntt_inv_galois_kernel): a mixture of classes launches once per class
template <class Fn>
static int with_policy_or_classes(const dpfhe_ctx* c, Fn fn) {
    if (class_mixture(c)) return for_each_class(c, c->n_limbs, fn);
    return with_policy(c, fn);
}

// Large batches go through in slices whose scratch stays below the context's scratch limit (the slices run back to back on the caller's stream and reuse
// the pool's block): the scratch of a composed operation is 4 (multiply) or L^2 / 2 (key switch) times its input.
// fn(first, count) over [0, total) in slices of at most `per` (scratch-limited slices; kMaxGaloisBatch elements per launch); stops at the first non-zero result
template <class Fn>
static int for_slices(size_t total, size_t per, Fn fn) {
    for (size_t first = 0; first < total; first += per)
        if (int rc = fn(first, total - first < per ? total - first : per)) return rc;
    return DPFHE_SUCCESS;
}
// The limbs of a kernel whose per-limb constants are a kernel ARGUMENT (plain add, noise), in launches of at most `max_per_launch`: fill(l0, count) sets
// limbs [l0, l0 + count) in the arguments, f() launches them (or runs the host twin); stops at the first non-zero result
template <class Fill, class Fn>
static int for_limb_groups(uint32_t n_limbs, uint32_t max_per_launch, Fill fill, Fn f) {
    return for_slices(n_limbs, max_per_launch, [&](size_t l0, size_t count) {
        fill((uint32_t)l0, (uint32_t)count);
        return f();
    });
}
inline size_t slice_items(const dpfhe_ctx* c, size_t batch, size_t scratch_words_per_item) {   // 1 GiB of scratch unless dpfhe_ctx_set_scratch_limit said otherwise
    const size_t fit = c->scratch_limit_words.load(std::memory_order_relaxed) / scratch_words_per_item;
    return fit == 0 ? 1 : (fit < batch ? fit : batch);
}

// A LEASE of the stream's scratch arena (scratch_pool.h: when arenas are made, grown, evicted and released): alloc() pins the arena's block into `p`, the
// destructor records the arena's event on the stream and unpins.  So the object lives until the last launch that reads `p` has been enqueued, and ends
// while the DeviceGuard of its entry is still in scope (declared after it): the event is recorded on the context's device.  Steady state: no allocation,
// no synchronisation, one hipEventRecord per lease.
// (Plain hipMalloc blocks, not the stream-ordered memory pool of rounds 2-4: round 5 found blocks of tens of MiB from that pool giving wrong results and
// millisecond allocation times in a process without PyTorch, while the same calls under PyTorch were exact.)
struct StreamScratch {
    u64* p = nullptr;
    dpfhe_ctx* c;
    hipStream_t s;
    StreamScratch(dpfhe_ctx* ctx, hipStream_t st) : c(ctx), s(st) {}
    ~StreamScratch() { if (held) c->scratch.end(lease); }
    StreamScratch(const StreamScratch&) = delete;
    StreamScratch& operator=(const StreamScratch&) = delete;
    int alloc(size_t words, const char* what);   // cabi_ctx.hip; once per object
private:
    ScratchPool<HipScratchBackend>::Lease lease;
    bool held = false;
};

// the ring of a host twin (no context to take it from): at least one limb, 8 <= log2 N <= 16, odd moduli in [3, 2^60)
inline int check_host_ring(const char* what, const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n) {
    if (n_limbs == 0 || log2_n < 8 || log2_n > (uint32_t)kMaxLog2N) return fail(DPFHE_INVALID_ARGUMENT, what, "n_limbs >= 1 and log2_n in [8, 16]");
    for (uint32_t l = 0; l < n_limbs; ++l)
        if (moduli[l] < 3 || (moduli[l] >> 60) || !(moduli[l] & 1)) return fail(DPFHE_INVALID_ARGUMENT, what, "moduli must be odd, >= 3 and < 2^60");
    return DPFHE_SUCCESS;
}

// t^-1 mod q by the extended Euclidean algorithm; false when gcd(t, q) != 1
inline bool inverse_mod(uint64_t t, uint64_t q, uint64_t& inv) {
    int64_t r0 = (int64_t)q, r1 = (int64_t)(t % q), s0 = 0, s1 = 1;   // q < 2^60: every remainder and coefficient fits int64
    while (r1) {
        const int64_t k = r0 / r1, r2 = r0 - k * r1, s2 = s0 - k * s1;
        r0 = r1; r1 = r2; s0 = s1; s1 = s2;
    }
    if (r0 != 1) return false;
    inv = s0 < 0 ? (uint64_t)(s0 + (int64_t)q) : (uint64_t)s0;
    return true;
}

// (g^-1 mod 2N for the coefficient-domain rotations: workmap.h galois_inverse)

// ---- launches one family borrows from another: arguments validated, device selected by the caller ------------------------------------------------------------
// batched transform of `items` RNS polynomials over the first `limbs_used` limbs (limbs_used = 0: all)
int ntt_launch_items(dpfhe_ctx* c, bool inverse, uint64_t* out, const uint64_t* in, size_t items, size_t limbs_used, hipStream_t s);   // cabi_poly.hip
inline int ntt_launch(dpfhe_ctx* c, bool inverse, uint64_t* out, const uint64_t* in, size_t npolys, hipStream_t s) {
    return ntt_launch_items(c, inverse, out, in, npolys / c->n_limbs, 0, s);
}
// dyadic_kernel<op> over `npolys` residue polynomials (DyOp; b_period as in kernels_poly.h); -1: no such op                                  // cabi_poly.hip
int launch_dyadic(const dpfhe_ctx* c, int op, u64* out, const u64* a, const u64* b, size_t npolys, hipStream_t s, int b_period);
// what the rotations borrow from key switching (cabi_keyswitch.hip, which describes each at its definition): the division by P, the digit lift, and the
// hybrid key switch itself with every check of its entries (`what` names the caller in its reports)
void launch_rescale(const dpfhe_ctx* c, size_t blocks, hipStream_t s, u64* out, const u64* in, const u64* add, int add_comps, int add_mask);
void launch_lift_digits(const dpfhe_ctx* c, size_t grid, hipStream_t s, u64* digits, const u64* comp, size_t item_stride, int chunks);
int key_switch_hybrid(dpfhe_ctx* c, const char* what, int in_comps, uint64_t* d_out2, const uint64_t* d_in, const uint64_t* d_key, uint64_t* d_work, size_t batch,
                      void* stream, size_t key_stride = 0, unsigned key_group = 1, bool drop_last = false);
// ... and its first pass alone, for a caller with a last pass of its own (the rotate-and-add ladder): the grid check, then the key products into d_work
bool key_products_fit(const dpfhe_ctx* c, size_t batch, size_t key_stride, unsigned key_group);
int key_products_hybrid(dpfhe_ctx* c, const char* what, int in_comps, uint64_t* d_work, const uint64_t* d_in, const uint64_t* d_key, size_t batch, hipStream_t s,
                        size_t key_stride, unsigned key_group);
