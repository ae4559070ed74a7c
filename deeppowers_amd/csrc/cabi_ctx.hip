// cabi_ctx.hip - libdpfhe_hip.so, the C ABI declared in include/dpfhe.h over the gfx950 kernels (cabi.h lists its units): contexts and their tables,
// the variant choice of the fused multiply, the scratch arenas of the composed large-ring operations, the error report.
// (The ABI's conventions and their source in the reference: head of cabi.h.)
#include <new>

#include "cabi.h"
#include "ctx_tables.h"
#include "fused_rescale.h"

static thread_local std::string g_last_error;

int fail(int code, const char* what, const char* detail) {
    g_last_error = std::string(what) + ": " + (detail ? detail : "");
    return code;
}

int upload_blob(void** dst, const std::vector<unsigned char>& host, const char* what) {
    hipError_t e = hipMalloc(dst, host.size());
    if (e == hipSuccess) e = hipMemcpy(*dst, host.data(), host.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) return DPFHE_SUCCESS;
    if (*dst) (void)hipFree(*dst);
    *dst = nullptr;
    return fail(e == hipErrorOutOfMemory ? DPFHE_OUT_OF_MEMORY : DPFHE_DEVICE_ERROR, what, hipGetErrorString(e));
}

// ------------------------------------------------------------------------------------------------
// Variant choice of the fused multiply (the reference sketches this class of mechanism as an auto-tuner:
// /root/reference/src/core/inference/auto_tuner.hpp:26-64).  The two forms move the same bytes and give the same words.
// dpfhe_ctx_create NEVER measures: it takes the ring degree's default form (or what an earlier EXPLICIT dpfhe_ctx_autotune on the same
// (device, log2 N, L) found - a process-wide cache), allocates nothing besides the tables and launches nothing (round 5: the constructor-time
// probe of round 4 cost 256 MiB and 30 launches per context to confirm a default that won on every box measured).
// dpfhe_ctx_autotune, on CALLER scratch: `reps` back-to-back launches per form over `pairs` synthetic ciphertext pairs, two passes in opposite
// orders, best pass per form; a non-default form is taken only when it is at least 3 % faster than the default.
// ------------------------------------------------------------------------------------------------
static const char* const kCtMulVariantNames[kCtMulVariants] = {"quad", "dual"};
static const float kTuneMargin = 0.97f;

__global__ __launch_bounds__(256) void tune_fill_kernel(u64* __restrict__ p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        p[i] = ((i + 1) * 0x9E3779B97F4A7C15ull) >> 5;   // < 2^59: a canonical residue of every FoldArith prime
}

// process-wide results of explicit probes, keyed (device, log2 N, L): a later context of the same shape starts from them
struct TuneKey {
    int device; uint32_t log2n, n_limbs;
    bool operator==(const TuneKey& o) const { return device == o.device && log2n == o.log2n && n_limbs == o.n_limbs; }
};
static std::mutex g_tune_cache_mutex;
static std::vector<std::pair<TuneKey, dpfhe_tune_info>> g_tune_cache;

// probes on `s`; synchronises it.  us[v] < 0: not available.  Returns a hipError_t.
static hipError_t probe_ct_mul(dpfhe_ctx* c, u64* work, size_t pairs, unsigned reps, hipStream_t s, float us[kCtMulVariants]) {
    const size_t poly = (size_t)c->n_limbs << c->log2n, blocks = pairs * c->n_limbs;
    u64 *a = work, *b = work + 2 * pairs * poly, *o = work + 4 * pairs * poly;
    hipLaunchKernelGGL(tune_fill_kernel, dim3(c->n_cu * 8), dim3(256), 0, s, work, 4 * pairs * poly);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t err = hipEventCreate(&e0);
    if (err == hipSuccess) err = hipEventCreate(&e1);
    for (int v = 0; v < kCtMulVariants; ++v) us[v] = -1.0f;
    for (int pass = 0; pass < 2 && err == hipSuccess; ++pass) {
        for (int i = 0; i < kCtMulVariants && err == hipSuccess; ++i) {
            const int v = pass ? kCtMulVariants - 1 - i : i;
            if (!ct_mul_variant_compiled(c, v)) continue;
            if (launch_ct_mul_variant<FoldArith>((int)c->log2n, v, o, a, b, blocks, c->foldt, s)) continue;    // warm-up (code object, clocks)
            (void)hipEventRecord(e0, s);
            for (unsigned r = 0; r < reps; ++r) (void)launch_ct_mul_variant<FoldArith>((int)c->log2n, v, o, a, b, blocks, c->foldt, s);
            (void)hipEventRecord(e1, s);
            err = hipEventSynchronize(e1);
            float ms = 0;
            if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
            if (err == hipSuccess) { const float t = ms * 1e3f / reps; if (us[v] < 0 || t < us[v]) us[v] = t; }
        }
    }
    if (err == hipSuccess) err = hipGetLastError();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return err;
}

static void adopt_probe(dpfhe_ctx* c, const float us[kCtMulVariants], size_t pairs, unsigned reps) {
    const int def = ct_mul_default_variant((int)c->log2n);
    int best = def;
    for (int v = 0; v < kCtMulVariants; ++v)
        if (us[v] > 0 && us[def] > 0 && us[v] < kTuneMargin * us[def] && (best == def || us[v] < us[best])) best = v;
    dpfhe_tune_info t{};
    t.n_variants = kCtMulVariants;
    t.source = DPFHE_TUNE_EXPLICIT;
    t.probe_pairs = (uint32_t)pairs;
    t.probe_reps = reps;
    for (int v = 0; v < 8; ++v) t.probe_us[v] = v < kCtMulVariants ? us[v] : -1.0f;
    t.chosen = best;
    {
        std::lock_guard<std::mutex> lk(c->tune_mutex);
        c->tune = t;
        c->ct_mul_variant.store(best);
    }
    const TuneKey key{c->device, c->log2n, c->n_limbs};
    std::lock_guard<std::mutex> lk(g_tune_cache_mutex);
    for (auto& e : g_tune_cache)
        if (e.first == key) { e.second = t; return; }
    g_tune_cache.emplace_back(key, t);
}

// at context creation: the default form, or the cached result of an explicit probe of this shape on this device.  No device work.
static void tune_at_create(dpfhe_ctx* c) {
    const int def = ct_mul_default_variant((int)c->log2n);
    dpfhe_tune_info t{};
    t.chosen = def;
    t.source = DPFHE_TUNE_DEFAULT;
    t.n_variants = ct_mul_variant_compiled(c, def) ? kCtMulVariants : 0;
    for (int v = 0; v < 8; ++v) t.probe_us[v] = -1.0f;
    if (t.n_variants) {
        const TuneKey key{c->device, c->log2n, c->n_limbs};
        std::lock_guard<std::mutex> lk(g_tune_cache_mutex);
        for (const auto& e : g_tune_cache)
            if (e.first == key) { t = e.second; t.source = DPFHE_TUNE_CACHED; break; }
    }
    c->tune = t;
    c->ct_mul_variant.store(t.chosen);
}

extern "C" void dpfhe_tune_cache_clear(void) {
    std::lock_guard<std::mutex> lk(g_tune_cache_mutex);
    g_tune_cache.clear();
}

extern "C" int dpfhe_ctx_autotune(dpfhe_ctx* c, uint64_t* d_work, size_t work_words, uint32_t reps, void* stream) {
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_ctx_autotune", "null context");
    if (!ct_mul_variant_compiled(c, ct_mul_default_variant((int)c->log2n))) return DPFHE_SUCCESS;   // one form only: nothing to choose
    const size_t poly = (size_t)c->n_limbs << c->log2n, pairs = work_words / (7 * poly);
    if (!d_work || misaligned(d_work) || pairs == 0) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_ctx_autotune", "d_work must hold at least 7 L N words (one ciphertext pair + its product)");
    if (pairs * c->n_limbs > kMaxGrid) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_ctx_autotune", "work buffer too large for one launch");
    if (reps == 0) reps = 3;
    DPFHE_ON_DEVICE(c, "dpfhe_ctx_autotune");
    float us[kCtMulVariants];
    HIP_TRY(probe_ct_mul(c, d_work, pairs, reps, static_cast<hipStream_t>(stream), us));
    adopt_probe(c, us, pairs, reps);
    return DPFHE_SUCCESS;
}
extern "C" int dpfhe_ctx_tune_info(const dpfhe_ctx* c, dpfhe_tune_info* out) {
    if (!c || !out) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_ctx_tune_info", "null argument");
    std::lock_guard<std::mutex> lk(c->tune_mutex);
    *out = c->tune;
    out->chosen = c->ct_mul_variant.load();
    return DPFHE_SUCCESS;
}
extern "C" int dpfhe_ctx_set_ct_mul_variant(dpfhe_ctx* c, int variant) {
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_ctx_set_ct_mul_variant", "null context");
    if (!ct_mul_variant_compiled(c, variant)) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_ctx_set_ct_mul_variant", "this context has no such form of the fused multiply");
    std::lock_guard<std::mutex> lk(c->tune_mutex);
    c->ct_mul_variant.store(variant);
    c->tune.chosen = variant;
    c->tune.source = DPFHE_TUNE_FORCED;
    return DPFHE_SUCCESS;
}
extern "C" const char* dpfhe_ct_mul_variant_name(int variant) {
    return variant >= 0 && variant < kCtMulVariants ? kCtMulVariantNames[variant] : "";
}

// the tables of a context: built on the host by ctx_tables.h (layouts, blobs, typed views), uploaded and viewed on the device here
extern "C" int dpfhe_ctx_create(dpfhe_ctx** out, uint32_t log2_n, uint32_t n_limbs, const uint64_t* moduli,
                                const uint64_t* psi, int device_id) {
    if (!out || !moduli || !psi) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_ctx_create", "null argument");
    if (log2_n < 8 || log2_n > (uint32_t)kMaxLog2N) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_ctx_create", "log2_n must be in [8, 16]");
    if (n_limbs == 0 || n_limbs > 1024) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_ctx_create", "n_limbs must be in [1, 1024]");
    const size_t L = n_limbs;
    std::vector<HostLimbTables> ht(L);
    bool fold = true;
    for (size_t l = 0; l < L; ++l) {
        // inverses (N^-1, psi^-1, rescale constants) are Fermat powers: a composite modulus that happens to satisfy
        // psi^N = -1 would make them silently wrong, so primality is checked (deterministic Miller-Rabin, one-off)
        if (!h_is_prime(moduli[l])) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_ctx_create", "modulus is not prime");
        int rc = build_limb_tables((int)log2_n, moduli[l], psi[l], ht[l]);
        if (rc) return fail(rc, "dpfhe_ctx_create", "modulus must be < 2^60 and 1 mod 2N, psi a primitive 2N-th root");
        fold = fold && fold_eligible(moduli[l]);
    }
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_ctx_create", "no such device");
    int prev = 0;
    HIP_TRY(hipGetDevice(&prev));
    HIP_TRY(hipSetDevice(device_id));

    dpfhe_ctx* c = new (std::nothrow) dpfhe_ctx;
    if (!c) return fail(DPFHE_OUT_OF_MEMORY, "dpfhe_ctx_create", "host allocation");
    c->log2n = log2_n; c->n_limbs = n_limbs; c->device = c->scratch.backend().device = device_id; c->fold = fold; c->p_special = moduli[L - 1];
    c->moduli.assign(moduli, moduli + L);
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) c->n_cu = cus; }

    const CtxLayout lay = ctx_layout((int)log2_n, L, fold);
    const std::vector<unsigned char> blob = build_ctx_blob((int)log2_n, ht, fold);
    // the table uploads; a failed one frees what exists, restores the caller's device and reports `stage`
    auto upload = [&](void*& dst, const std::vector<unsigned char>& host, const char* stage) -> int {
        const int rc = upload_blob(&dst, host, stage);
        if (rc) {
            (void)dpfhe_ctx_destroy(c);
            (void)hipSetDevice(prev);
        }
        return rc;
    };
    if (int rc = upload(c->d_blob, blob, "dpfhe_ctx_create: table upload")) return rc;
    const unsigned char* d = static_cast<const unsigned char*>(c->d_blob);
    c->lc = reinterpret_cast<const LimbConst*>(d + lay.o_lc);
    c->d_rescale = reinterpret_cast<const RescaleConst*>(d + lay.o_resc);
    if (fold) c->foldt = ctx_view<FoldArith>(d, lay, L);
    else c->shoup = ctx_view<ShoupArith>(d, lay, L);
    // per-limb arithmetic classes of a non-uniform context (see dpfhe_ctx::classes)
    if (ctx_limb_classes((int)log2_n, ht, fold, c->limb_cls)) {
        const MixedLayout m = mixed_layout((int)log2_n, L);
        const std::vector<unsigned char> mb = build_class_blob((int)log2_n, ht, c->limb_cls);
        for (size_t l = 0; l < L; ++l) c->cls_map |= (unsigned long long)c->limb_cls[l] << (4 * l);
        if (int rc = upload(c->class_blob, mb, "dpfhe_ctx_create: class table upload")) return rc;
        const unsigned char* b = static_cast<const unsigned char*>(c->class_blob);
        c->cls_fold = mixed_view<FoldArith>(b, m, L);
        c->cls_f64 = mixed_view<F64Arith>(b, m, L);
        c->cls_fscaled = mixed_view<FoldScaledArith>(b, m, L);
        c->cls_f64w = mixed_view<F64WideArith>(b, m, L);
        c->cls_shoup = mixed_view<ShoupArith>(b, m, L);
        c->mixed.fwd = b + m.o_fwd; c->mixed.inv = b + m.o_inv; c->mixed.last = b + m.o_last;
        c->mixed.lc = reinterpret_cast<const LimbConst*>(b + m.o_lc);
        c->mixed.n_limbs = (int)L;
        c->mixed.cls_map = c->cls_map;
        c->classes = true;
        bool same = true;
        for (size_t l = 1; l < L; ++l) same = same && c->limb_cls[l] == c->limb_cls[0];
        if (same) c->uniform_cls = c->limb_cls[0];
    }
    {   // the fused multiply's lazy tables: seen through whichever FoldArith view launches ct_mul_quad_kernel at N = 4096
        std::vector<bool> fold_limb(L);
        for (size_t l = 0; l < L; ++l) fold_limb[l] = fold || (c->classes && c->limb_cls[l] == kClassFold);
        const std::vector<unsigned char> lb = build_lazy29_blob((int)log2_n, ht, fold_limb);
        if (!lb.empty()) {
            if (int rc = upload(c->lazy29_blob, lb, "dpfhe_ctx_create: lazy table upload")) return rc;
            lazy29_view(fold ? c->foldt : c->cls_fold, static_cast<const unsigned char*>(c->lazy29_blob), lazy29_layout(L));
        }
    }
    if (L >= 3) {   // the second division of dpfhe_relinearize_rescale_hybrid
        std::vector<unsigned char> rb((L - 2) * sizeof(RescaleConst));
        fill_rescale_consts(reinterpret_cast<RescaleConst*>(rb.data()), moduli, L - 2, [](u64 a, u64 q) { return h_powmod(a, q - 2, q); });
        if (int rc = upload(c->rescale2_blob, rb, "dpfhe_ctx_create: second rescale table upload")) return rc;
        c->d_rescale2 = static_cast<const RescaleConst*>(c->rescale2_blob);
    }
    tune_at_create(c);   // default form of the fused multiply, or a cached explicit probe of this shape: no device work
    (void)hipSetDevice(prev);
    *out = c;
    return DPFHE_SUCCESS;
}

extern "C" int dpfhe_ctx_destroy(dpfhe_ctx* c) {
    if (!c) return DPFHE_SUCCESS;
    if (c->d_blob) (void)hipFree(c->d_blob);
    if (c->class_blob) (void)hipFree(c->class_blob);
    if (c->lazy29_blob) (void)hipFree(c->lazy29_blob);
    if (c->rescale2_blob) (void)hipFree(c->rescale2_blob);
    delete c;   // (the scratch pool waits for, frees and strips of its event every arena it still has)
    return DPFHE_SUCCESS;
}
extern "C" int dpfhe_ctx_set_scratch_limit(dpfhe_ctx* c, size_t mib) {
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_ctx_set_scratch_limit", "null context");
    if (mib == 0 || mib > ((size_t)1 << 20)) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_ctx_set_scratch_limit", "limit must be in [1 MiB, 1 TiB]");
    c->scratch_limit_words.store(mib << 17, std::memory_order_relaxed);
    return DPFHE_SUCCESS;
}
extern "C" uint32_t dpfhe_ctx_log2n(const dpfhe_ctx* c) { return c ? c->log2n : 0; }
extern "C" uint32_t dpfhe_ctx_limbs(const dpfhe_ctx* c) { return c ? c->n_limbs : 0; }
extern "C" int dpfhe_ctx_uses_fold(const dpfhe_ctx* c) { return c && c->fold ? 1 : 0; }
extern "C" int dpfhe_ctx_limb_class(const dpfhe_ctx* c, uint32_t limb) {
    if (!c || limb >= c->n_limbs) return -1;
    if (c->classes) return (int)c->limb_cls[limb];
    return c->fold ? DPFHE_ARITH_FOLD : DPFHE_ARITH_SHOUP;
}
static_assert(DPFHE_ARITH_SHOUP == kClassShoup && DPFHE_ARITH_FOLD == kClassFold && DPFHE_ARITH_F64 == kClassF64 && DPFHE_ARITH_FOLD_SCALED == kClassFoldScaled &&
              DPFHE_ARITH_F64_WIDE == kClassF64Wide, "dpfhe.h <-> tables.h");

// ------------------------------------------------------------------------------------------------
// the scratch arenas: the device calls of their policy (scratch_pool.h), the lease (cabi.h StreamScratch) and the three entries

// a device call of the backend under a guard on the context's device; a failed guard fails the call
template <class Fn>
static hipError_t on_device(int device, Fn fn) {
    DeviceGuard guard(device);
    const hipError_t e = guard.err != hipSuccess ? guard.err : fn();
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
}
int HipScratchBackend::alloc(size_t words, uint64_t*& p, const char*& detail) {
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) { detail = hipGetErrorString(guard.err); return DPFHE_DEVICE_ERROR; }
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), words * sizeof(u64));
    if (e == hipSuccess) return DPFHE_SUCCESS;
    (void)hipGetLastError();
    detail = hipGetErrorString(e);
    return DPFHE_OUT_OF_MEMORY;
}
// The event only says when the work that used the block is over, so that the block can be freed: nobody reads through it what that work wrote.  So no
// system-scope fence at the record - with one (the default) the cache write-back and invalidation between two back-to-back calls cost 3 to 5 us of device
// time per call at N = 16384 (profiles/r22_scratch_leases.txt).
int HipScratchBackend::new_event(Event& ev, const char*& detail) {
    const hipError_t e = on_device(device, [&] { return hipEventCreateWithFlags(&ev, hipEventDisableTiming | hipEventDisableSystemFence); });
    if (e != hipSuccess) detail = hipGetErrorString(e);
    return e == hipSuccess ? DPFHE_SUCCESS : DPFHE_DEVICE_ERROR;
}
void HipScratchBackend::free(uint64_t* p) { (void)on_device(device, [&] { return hipFree(p); }); }
void HipScratchBackend::destroy_event(Event ev) { (void)on_device(device, [&] { return hipEventDestroy(ev); }); }
void HipScratchBackend::wait(Event ev) { (void)on_device(device, [&] { return hipEventSynchronize(ev); }); }

int StreamScratch::alloc(size_t words, const char* what) {
    const char* detail = "";
    const int rc = c->scratch.acquire(s, words, lease, detail);
    if (rc) return fail(rc, what, detail);
    held = true;
    p = lease.p;
    return DPFHE_SUCCESS;
}

extern "C" int dpfhe_ctx_release_scratch(dpfhe_ctx* c, void* stream, uint32_t flags) {
    if (!c) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_ctx_release_scratch", "null context");
    if (flags & ~(uint32_t)DPFHE_SCRATCH_ALL) return fail(DPFHE_INVALID_ARGUMENT, "dpfhe_ctx_release_scratch", "unknown flag");
    if (c->scratch.release(static_cast<hipStream_t>(stream), (flags & DPFHE_SCRATCH_ALL) != 0))
        return fail(DPFHE_INVALID_STATE, "dpfhe_ctx_release_scratch", "an arena is in use by a call in progress (it stays)");
    return DPFHE_SUCCESS;
}
extern "C" size_t dpfhe_ctx_scratch_bytes(const dpfhe_ctx* c) { return c ? c->scratch.bytes() : 0; }

// ------------------------------------------------------------------------------------------------
extern "C" const char* dpfhe_strerror(int code) {
    switch (code) {
        case DPFHE_SUCCESS: return "success";
        case DPFHE_OUT_OF_MEMORY: return "out of memory";
        case DPFHE_DEVICE_ERROR: return "device error";
        case DPFHE_INVALID_ARGUMENT: return "invalid argument";
        case DPFHE_INVALID_STATE: return "invalid state";
        case DPFHE_RUNTIME_ERROR: return "runtime error";
        default: return "unknown error";
    }
}
extern "C" const char* dpfhe_last_error(void) { return g_last_error.c_str(); }
