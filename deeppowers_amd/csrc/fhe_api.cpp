// fhe_api.cpp - deeppowers::fhe facade over the C ABI (include/dpfhe.h): parameters, contexts, buffers and their wire formats, the evaluator and the
// communicator.  Plain C++17 (g++); the only HIP it touches is the runtime API for buffer ownership.  The other roles of the facade, all built into the
// same libdpfhe_api.so: fhe_keys.cpp (everything that holds or draws secrets), fhe_keyswitch.cpp, fhe_encode.cpp, fhe_packed.cpp (kBabyShiftDefault
// lives there), fhe_polynomial.cpp, fhe_invsqrt.cpp, fhe_product_sum.cpp, fhe_divide.cpp; fhe_internal.h is what they share.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <istream>
#include <ostream>

#include "fhe_internal.h"

namespace deeppowers {
namespace fhe {

using namespace detail;

namespace {
// the 20 largest primes below 2^60 that are 1 mod 2^14, largest first (deeppowers_amd/params.py ntt_primes(13, 20) generates the same list): {q, smallest
// primitive 8192-th root (N = 4096; 0 = not tabulated), smallest primitive 16384-th root (N = 8192)}
constexpr size_t kChainPrimes = 20;
const uint64_t kPrimes60[kChainPrimes][3] = {
    {1152921504606830593ull, 116777451583545ull, 25959043411404ull}, {1152921504606748673ull, 271802498405390ull, 100406242475323ull},
    {1152921504606683137ull, 134367042585739ull, 45474351589225ull}, {1152921504606601217ull, 276147373136904ull, 92707844590835ull},
    {1152921504606584833ull, 317490233586139ull, 23981819781494ull}, {1152921504606109697ull, 279138086580908ull, 253932030982881ull},
    {1152921504605962241ull, 0ull, 64984728504994ull}, {1152921504605913089ull, 0ull, 27694533958986ull},
    {1152921504605847553ull, 0ull, 105031879276246ull}, {1152921504605618177ull, 0ull, 157253107066567ull},
    {1152921504604979201ull, 0ull, 76334773615457ull}, {1152921504604766209ull, 0ull, 14852029848402ull},
    {1152921504604635137ull, 0ull, 93806574463579ull}, {1152921504602505217ull, 0ull, 217691047434989ull},
    {1152921504601980929ull, 0ull, 112510666220977ull}, {1152921504601915393ull, 0ull, 12114078003698ull},
    {1152921504601784321ull, 0ull, 4580624056246ull}, {1152921504600309761ull, 0ull, 135029094688496ull},
    {1152921504600260609ull, 0ull, 120773065591640ull}, {1152921504600145921ull, 0ull, 1663825873988ull}};
// the 8 largest primes below 2^60 that are 1 mod 2^15 (deeppowers_amd/params.py ntt_primes(14, 8)): {q, smallest primitive 32768-th root}
constexpr size_t kChainPrimes14 = 8;
const uint64_t kPrimes60N14[kChainPrimes14][2] = {
    {1152921504606748673ull, 62213374832584ull}, {1152921504606683137ull, 212089012217363ull}, {1152921504606584833ull, 92166579128688ull},
    {1152921504605962241ull, 74756755228070ull}, {1152921504604979201ull, 52069629205452ull}, {1152921504600260609ull, 27543819356734ull},
    {1152921504599080961ull, 92056553354496ull}, {1152921504598720513ull, 89492317149395ull}};
// the 14 largest primes below 2^60 that are 1 mod 2^16 (deeppowers_amd/params.py ntt_primes(15, 14)): {q, smallest primitive 65536-th root}; the first 8 are
// 2^60 - d with d < 2^24 (fold primes)
constexpr size_t kChainPrimes15 = 14;
const uint64_t kPrimes60N15[kChainPrimes15][2] = {
    {1152921504606584833ull, 4443670208963ull}, {1152921504598720513ull, 100545759574150ull}, {1152921504597016577ull, 31693996050849ull},
    {1152921504595968001ull, 88651361085495ull}, {1152921504595640321ull, 9679305630873ull}, {1152921504593412097ull, 24428769072221ull},
    {1152921504592822273ull, 18776242964106ull}, {1152921504592429057ull, 5821397352863ull}, {1152921504589938689ull, 33888991361320ull},
    {1152921504586530817ull, 74969624337902ull}, {1152921504585547777ull, 64462945958447ull}, {1152921504583647233ull, 6656235313685ull},
    {1152921504581877761ull, 18584577086900ull}, {1152921504581419009ull, 34653674914762ull}};
}  // namespace

FheParams FheParams::drop_last_limb() const {
    if (moduli.size() < 2) throw Exception(ErrorCode::INVALID_STATE, "drop_last_limb: no limb left to drop");
    FheParams p{log2_n, moduli, psi};
    p.moduli.pop_back(); p.psi.pop_back();
    return p;
}
FheParams FheParams::config1() { return FheParams{10, {1073707009ull}, {169871ull}}; }
FheParams FheParams::n4096_l4() {
    FheParams p{12, {}, {}};
    for (int i = 0; i < 4; ++i) { p.moduli.push_back(kPrimes60[i][0]); p.psi.push_back(kPrimes60[i][1]); }
    return p;
}
FheParams FheParams::n8192_l6() { return n8192(6); }
FheParams FheParams::n8192(size_t n_limbs) {
    if (n_limbs == 0 || n_limbs > kChainPrimes) throw Exception(ErrorCode::INVALID_ARGUMENT, "FheParams::n8192: 1..20 limbs");
    FheParams p{13, {}, {}};
    for (size_t i = 0; i < n_limbs; ++i) { p.moduli.push_back(kPrimes60[i][0]); p.psi.push_back(kPrimes60[i][2]); }
    return p;
}

FheParams FheParams::n16384(size_t n_limbs) {
    if (n_limbs == 0 || n_limbs > kChainPrimes14) throw Exception(ErrorCode::INVALID_ARGUMENT, "FheParams::n16384: 1..8 limbs");
    FheParams p{14, {}, {}};
    for (size_t i = 0; i < n_limbs; ++i) { p.moduli.push_back(kPrimes60N14[i][0]); p.psi.push_back(kPrimes60N14[i][1]); }
    return p;
}

FheParams FheParams::n32768(size_t n_limbs) {
    if (n_limbs == 0 || n_limbs > kChainPrimes15) throw Exception(ErrorCode::INVALID_ARGUMENT, "FheParams::n32768: 1..14 limbs");
    FheParams p{15, {}, {}};
    for (size_t i = 0; i < n_limbs; ++i) { p.moduli.push_back(kPrimes60N15[i][0]); p.psi.push_back(kPrimes60N15[i][1]); }
    return p;
}

// ---- Context ---------------------------------------------------------------------------------------
class Context::Impl {
public:
    FheParams params;
    int device_id = 0;
    dpfhe_ctx* h = nullptr;
};

Context::Context(const FheParams& params, int device_id) : impl_(new Impl) {
    impl_->params = params;
    impl_->device_id = device_id;
    if (params.moduli.empty() || params.moduli.size() != params.psi.size())
        throw Exception(ErrorCode::INVALID_ARGUMENT, "FheParams: moduli and psi must be non-empty and of equal length");
    check(dpfhe_ctx_create(&impl_->h, params.log2_n, (uint32_t)params.moduli.size(), params.moduli.data(), params.psi.data(), device_id), "dpfhe_ctx_create");
}
Context::~Context() {
    if (impl_ && impl_->h) dpfhe_ctx_destroy(impl_->h);
}
const FheParams& Context::params() const { return impl_->params; }
int Context::device_id() const { return impl_->device_id; }
bool Context::uses_fold() const { return dpfhe_ctx_uses_fold(impl_->h) != 0; }
int Context::limb_class(uint32_t limb) const { return dpfhe_ctx_limb_class(impl_->h, limb); }
void Context::release_scratch(void* stream, bool all_streams) { check(dpfhe_ctx_release_scratch(impl_->h, stream, all_streams ? DPFHE_SCRATCH_ALL : 0), "dpfhe_ctx_release_scratch"); }
size_t Context::scratch_bytes() const { return dpfhe_ctx_scratch_bytes(impl_->h); }
void* Context::handle() const { return impl_->h; }
Context::TuneInfo Context::tune_info() const {
    dpfhe_tune_info t{};
    check(dpfhe_ctx_tune_info(impl_->h, &t), "dpfhe_ctx_tune_info");
    static const char* const src[] = {"default", "?", "dpfhe_ctx_autotune", "forced", "cached dpfhe_ctx_autotune of this shape"};   // include/dpfhe.h DPFHE_TUNE_*
    TuneInfo r;
    r.chosen = dpfhe_ct_mul_variant_name(t.chosen);
    r.source = (t.source >= 0 && t.source < 5) ? src[t.source] : "?";
    r.probe_pairs = t.probe_pairs;
    r.probe_reps = t.probe_reps;
    for (int v = 0; v < t.n_variants && v < 8; ++v)
        if (t.probe_us[v] >= 0) r.probe_us.emplace_back(dpfhe_ct_mul_variant_name(v), t.probe_us[v]);
    return r;
}
Context::TuneInfo Context::autotune(PolyBuffer& scratch, unsigned reps) {
    check(dpfhe_ctx_autotune(impl_->h, scratch.data(), scratch.words(), reps, nullptr), "dpfhe_ctx_autotune");
    return tune_info();
}
void Context::synchronize() const {
    hip_check(hipSetDevice(impl_->device_id), "hipSetDevice");
    hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
}

void Context::set_scratch_limit(size_t mib) { check(dpfhe_ctx_set_scratch_limit(impl_->h, mib), "dpfhe_ctx_set_scratch_limit"); }

// ---- PolyBuffer -----------------------------------------------------------------------------------------
class PolyBuffer::Impl {
public:
    const Context* ctx = nullptr;
    uint64_t* d = nullptr;
    size_t batch = 0, comps = 0, words = 0;
    bool ntt = false;
    int device_id = 0;
    ~Impl() { if (d) (void)hipFree(d); }
};

PolyBuffer::PolyBuffer(const Context& ctx, size_t batch, size_t components, bool is_ntt) : impl_(new Impl) {
    if (batch == 0 || components == 0) throw Exception(ErrorCode::INVALID_ARGUMENT, "PolyBuffer: batch and components must be > 0");
    impl_->ctx = &ctx;
    impl_->batch = batch; impl_->comps = components; impl_->ntt = is_ntt; impl_->device_id = ctx.device_id();
    impl_->words = batch * components * ctx.params().n_limbs() * ctx.params().n();
    impl_->d = device_alloc<uint64_t>(impl_->device_id, impl_->words);
}
PolyBuffer::~PolyBuffer() = default;
PolyBuffer::PolyBuffer(PolyBuffer&&) noexcept = default;
PolyBuffer& PolyBuffer::operator=(PolyBuffer&&) noexcept = default;
uint64_t* PolyBuffer::data() { return impl_->d; }
const uint64_t* PolyBuffer::data() const { return impl_->d; }
size_t PolyBuffer::batch() const { return impl_->batch; }
size_t PolyBuffer::size() const { return impl_->comps; }
size_t PolyBuffer::words() const { return impl_->words; }
bool PolyBuffer::is_ntt() const { return impl_->ntt; }
void PolyBuffer::set_ntt(bool v) { impl_->ntt = v; }
const Context& PolyBuffer::context() const { return *impl_->ctx; }
void PolyBuffer::copy_from_host(const uint64_t* src) {
    if (!src) throw Exception(ErrorCode::INVALID_ARGUMENT, "copy_from_host: null source");
    hip_check(hipMemcpy(impl_->d, src, impl_->words * sizeof(uint64_t), hipMemcpyHostToDevice), "hipMemcpy H2D");
}
void PolyBuffer::copy_to_host(uint64_t* dst) const {
    if (!dst) throw Exception(ErrorCode::INVALID_ARGUMENT, "copy_to_host: null destination");
    hip_check(hipMemcpy(dst, impl_->d, impl_->words * sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy D2H");
}

namespace {
const char kMagic[8] = {'D', 'P', 'F', 'H', 'E', 'v', '1', 0};
struct WireHeader {   // all little-endian; x86-64 / gfx950 hosts are little-endian
    char magic[8];
    uint32_t log2_n, n_limbs;
    uint64_t batch, components;
    uint32_t is_ntt, reserved;
};
// what follows a stream's header: the moduli (they must be this context's), then `words` canonical residues [..][L][N]
std::vector<uint64_t> read_payload(std::istream& is, const FheParams& p, size_t words, const std::string& what) {
    std::vector<uint64_t> moduli(p.n_limbs()), host(words);
    is.read(reinterpret_cast<char*>(moduli.data()), (std::streamsize)(moduli.size() * sizeof(uint64_t)));
    if (!is || moduli != p.moduli) throw Exception(ErrorCode::INVALID_ARGUMENT, what + ": moduli differ from this context");
    is.read(reinterpret_cast<char*>(host.data()), (std::streamsize)(host.size() * sizeof(uint64_t)));
    if (!is) throw Exception(ErrorCode::INVALID_ARGUMENT, what + ": truncated stream");
    for (size_t i = 0; i < host.size(); ++i)
        if (host[i] >= p.moduli[(i / p.n()) % p.n_limbs()]) throw Exception(ErrorCode::INVALID_ARGUMENT, what + ": non-canonical residue in the payload");
    return host;
}
}  // namespace

void PolyBuffer::save(std::ostream& os) const {
    const FheParams& p = impl_->ctx->params();
    WireHeader h{};
    std::memcpy(h.magic, kMagic, 8);
    h.log2_n = p.log2_n; h.n_limbs = (uint32_t)p.n_limbs(); h.batch = impl_->batch; h.components = impl_->comps;
    h.is_ntt = impl_->ntt ? 1u : 0u; h.reserved = 0;
    std::vector<uint64_t> host(impl_->words);
    copy_to_host(host.data());
    os.write(reinterpret_cast<const char*>(&h), sizeof h);
    os.write(reinterpret_cast<const char*>(p.moduli.data()), (std::streamsize)(p.n_limbs() * sizeof(uint64_t)));
    os.write(reinterpret_cast<const char*>(host.data()), (std::streamsize)(host.size() * sizeof(uint64_t)));
    if (!os) throw Exception(ErrorCode::RUNTIME_ERROR, "save: stream write failed");
}

void PolyBuffer::load(std::istream& is) {
    const FheParams& p = impl_->ctx->params();
    WireHeader h{};
    is.read(reinterpret_cast<char*>(&h), sizeof h);
    if (!is || std::memcmp(h.magic, kMagic, 8) != 0) throw Exception(ErrorCode::INVALID_ARGUMENT, "load: not a DPFHEv1 stream");
    if (h.log2_n != p.log2_n || h.n_limbs != p.n_limbs() || h.batch != impl_->batch || h.components != impl_->comps)
        throw Exception(ErrorCode::INVALID_ARGUMENT, "load: header does not match this buffer (log2_n / limbs / batch / components)");
    const std::vector<uint64_t> host = read_payload(is, p, impl_->words, "load");
    copy_from_host(host.data());
    impl_->ntt = h.is_ntt != 0;
}

namespace {
const char kSeededMagic[8] = {'D', 'P', 'F', 'H', 'E', 's', '1', 0};
struct SeededHeader {   // DPFHEs1 (wire.py _SHDR): all little-endian
    char magic[8];
    uint32_t log2_n, n_limbs;
    uint64_t batch, components;
    uint32_t is_ntt, expanded_component;
    uint64_t first_item;
    uint8_t seed[32];
};
static_assert(sizeof(SeededHeader) == 80, "the DPFHEs1 header is 80 bytes");
}  // namespace

void PolyBuffer::save_seeded(std::ostream& os, const Seed& seed, uint32_t component, uint64_t first_item) const {
    const FheParams& p = impl_->ctx->params();
    const size_t batch = impl_->batch, comps = impl_->comps, poly = p.n_limbs() * p.n();
    if (component >= comps) throw Exception(ErrorCode::INVALID_ARGUMENT, "save_seeded: component must be < components");
    // re-expand and compare: a buffer that was overwritten or transformed since it was expanded must not go out under its seed
    PolyBuffer ref(*impl_->ctx, batch, comps, impl_->ntt);
    check(dpfhe_expand_uniform(handle_of(*impl_->ctx), ref.data(), batch, comps, component, seed.bytes, first_item, nullptr),
          "dpfhe_expand_uniform");
    std::vector<uint64_t> host(impl_->words), want(impl_->words);
    ref.copy_to_host(want.data());
    copy_to_host(host.data());
    for (size_t b = 0; b < batch; ++b) {
        const size_t off = (b * comps + component) * poly;
        if (std::memcmp(host.data() + off, want.data() + off, poly * sizeof(uint64_t)) != 0)
            throw Exception(ErrorCode::INVALID_STATE, "save_seeded: the buffer's component no longer matches its seed (overwritten or transformed)");
    }
    SeededHeader h{};
    std::memcpy(h.magic, kSeededMagic, 8);
    h.log2_n = p.log2_n; h.n_limbs = (uint32_t)p.n_limbs(); h.batch = batch; h.components = comps;
    h.is_ntt = impl_->ntt ? 1u : 0u; h.expanded_component = component; h.first_item = first_item;
    std::memcpy(h.seed, seed.bytes, 32);
    os.write(reinterpret_cast<const char*>(&h), sizeof h);
    os.write(reinterpret_cast<const char*>(p.moduli.data()), (std::streamsize)(p.n_limbs() * sizeof(uint64_t)));
    for (size_t b = 0; b < batch; ++b)
        for (size_t c = 0; c < comps; ++c)
            if (c != component) os.write(reinterpret_cast<const char*>(host.data() + (b * comps + c) * poly), (std::streamsize)(poly * sizeof(uint64_t)));
    if (!os) throw Exception(ErrorCode::RUNTIME_ERROR, "save_seeded: stream write failed");
}

void PolyBuffer::load_seeded(std::istream& is, Stream* stream) {
    const FheParams& p = impl_->ctx->params();
    SeededHeader h{};
    is.read(reinterpret_cast<char*>(&h), sizeof h);
    if (!is || std::memcmp(h.magic, kSeededMagic, 8) != 0) throw Exception(ErrorCode::INVALID_ARGUMENT, "load_seeded: not a DPFHEs1 stream");
    if (h.log2_n != p.log2_n || h.n_limbs != p.n_limbs() || h.batch != impl_->batch || h.components != impl_->comps)
        throw Exception(ErrorCode::INVALID_ARGUMENT, "load_seeded: header does not match this buffer (log2_n / limbs / batch / components)");
    if (h.expanded_component >= h.components) throw Exception(ErrorCode::INVALID_ARGUMENT, "load_seeded: expanded_component must be < components");
    if (h.first_item > ((uint64_t)1 << 32) || h.batch > ((uint64_t)1 << 32) - h.first_item)
        throw Exception(ErrorCode::INVALID_ARGUMENT, "load_seeded: first_item + batch must be <= 2^32");
    const size_t poly = p.n_limbs() * p.n(), comps = impl_->comps, kept = comps - 1, comp = h.expanded_component;
    const std::vector<uint64_t> host = read_payload(is, p, impl_->batch * kept * poly, "load_seeded");
    hip_check(hipSetDevice(impl_->device_id), "hipSetDevice");
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the stored components of every item: the run before the expanded one and the run after it, one strided copy each
    const size_t row = comps * poly * sizeof(uint64_t), src_row = kept * poly * sizeof(uint64_t);
    if (comp > 0)
        hip_check(hipMemcpy2DAsync(impl_->d, row, host.data(), src_row, comp * poly * sizeof(uint64_t), impl_->batch, hipMemcpyHostToDevice, s), "hipMemcpy2DAsync");
    if (comp + 1 < comps)
        hip_check(hipMemcpy2DAsync(impl_->d + (comp + 1) * poly, row, host.data() + comp * poly, src_row, (comps - 1 - comp) * poly * sizeof(uint64_t),
                                   impl_->batch, hipMemcpyHostToDevice, s), "hipMemcpy2DAsync");
    check(dpfhe_expand_uniform(handle_of(*impl_->ctx), impl_->d, impl_->batch, comps, (uint32_t)comp, h.seed, h.first_item, stream),
          "dpfhe_expand_uniform");
    hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");   // `host` is released on return
    impl_->ntt = h.is_ntt != 0;
}

Ciphertext::Ciphertext(const Context& ctx, size_t size, size_t batch, bool is_ntt) : PolyBuffer(ctx, batch, size, is_ntt) {
    if (size != 2 && size != 3) throw Exception(ErrorCode::INVALID_ARGUMENT, "Ciphertext: size must be 2 or 3");
}

// ---- ScalarMatrix -----------------------------------------------------------------------------------------------------------
class ScalarMatrix::Impl {
public:
    const Context* ctx = nullptr;
    size_t rows = 0, cols = 0;
    uint64_t* d = nullptr;
    ~Impl() { if (d) (void)hipFree(d); }
};
ScalarMatrix::ScalarMatrix(const Context& ctx, size_t rows, size_t cols) : impl_(new Impl) {
    if (rows == 0 || cols == 0) throw Exception(ErrorCode::INVALID_ARGUMENT, "ScalarMatrix: rows and cols must be > 0");
    impl_->ctx = &ctx; impl_->rows = rows; impl_->cols = cols;
    impl_->d = device_alloc<uint64_t>(ctx.device_id(), rows * cols * ctx.params().n_limbs());
}
ScalarMatrix::~ScalarMatrix() = default;
size_t ScalarMatrix::rows() const { return impl_->rows; }
size_t ScalarMatrix::cols() const { return impl_->cols; }
const uint64_t* ScalarMatrix::data() const { return impl_->d; }
void ScalarMatrix::set(const int64_t* w) {
    if (!w) throw Exception(ErrorCode::INVALID_ARGUMENT, "ScalarMatrix::set: null weights");
    const FheParams& p = impl_->ctx->params();
    const size_t L = p.n_limbs(), count = impl_->rows * impl_->cols;
    std::vector<uint64_t> host(count * L);
    for (size_t i = 0; i < count; ++i)
        for (size_t l = 0; l < L; ++l) {
            const uint64_t q = p.moduli[l];
            const uint64_t m = (uint64_t)(w[i] < 0 ? -(w[i] + 1) : w[i]) % q;            // |w| (two's-complement safe), mod q
            host[i * L + l] = w[i] >= 0 ? m : (q - 1 - m);                                 // -(m+1) = q - 1 - m
        }
    hip_check(hipMemcpy(impl_->d, host.data(), host.size() * sizeof(uint64_t), hipMemcpyHostToDevice), "hipMemcpy H2D");
}

// ---- ExactPlaintext ---------------------------------------------------------------------------------------------------------
class ExactPlaintext::Impl {
public:
    const Context* ctx = nullptr;
    uint64_t t = 0;
    size_t items = 0, n = 0;
    uint64_t* d = nullptr;
    ~Impl() { if (d) (void)hipFree(d); }
    void upload(const int64_t* coeffs) {   // items * n values, reduced mod t
        std::vector<uint64_t> host(items * n);
        for (size_t i = 0; i < host.size(); ++i) {
            const int64_t r = coeffs[i] % (int64_t)t;
            host[i] = (uint64_t)(r < 0 ? r + (int64_t)t : r);
        }
        hip_check(hipMemcpy(d, host.data(), host.size() * sizeof(uint64_t), hipMemcpyHostToDevice), "hipMemcpy H2D");
    }
};
ExactPlaintext::ExactPlaintext(const Context& ctx, uint64_t t, size_t items) : impl_(new Impl) {
    if (t < 3 || (t >> 32) || !(t & 1)) throw Exception(ErrorCode::INVALID_ARGUMENT, "ExactPlaintext: plaintext modulus must be odd, >= 3 and < 2^32");
    if (items == 0) throw Exception(ErrorCode::INVALID_ARGUMENT, "ExactPlaintext: items must be > 0");
    impl_->ctx = &ctx; impl_->t = t; impl_->items = items; impl_->n = ctx.params().n();
    impl_->d = device_alloc<uint64_t>(ctx.device_id(), items * impl_->n);
    hip_check(hipMemset(impl_->d, 0, items * impl_->n * sizeof(uint64_t)), "hipMemset");
}
ExactPlaintext::~ExactPlaintext() = default;
size_t ExactPlaintext::items() const { return impl_->items; }
uint64_t ExactPlaintext::plain_modulus() const { return impl_->t; }
size_t ExactPlaintext::ring_degree() const { return impl_->n; }
const uint64_t* ExactPlaintext::data() const { return impl_->d; }
void ExactPlaintext::set_coefficients(const int64_t* coeffs) {
    if (!coeffs) throw Exception(ErrorCode::INVALID_ARGUMENT, "ExactPlaintext::set_coefficients: null coefficients");
    impl_->upload(coeffs);
}
void ExactPlaintext::set_slots(const BatchEncoder& enc, const uint64_t* slots) {
    if (!slots) throw Exception(ErrorCode::INVALID_ARGUMENT, "ExactPlaintext::set_slots: null slots");
    if (enc.plain_modulus() != impl_->t || enc.slot_count() != impl_->n)
        throw Exception(ErrorCode::INVALID_ARGUMENT, "ExactPlaintext::set_slots: the encoder's plaintext modulus or ring degree differs");
    const size_t n = impl_->n;
    std::vector<int64_t> coeffs(impl_->items * n);
    for (size_t i = 0; i < impl_->items; ++i) enc.encode(slots + i * n, coeffs.data() + i * n);
    impl_->upload(coeffs.data());
}
void ExactPlaintext::set_slots_device(const BatchEncoder& enc, const uint32_t* slots, Stream* s) {
    if (enc.plain_modulus() != impl_->t || enc.slot_count() != impl_->n)
        throw Exception(ErrorCode::INVALID_ARGUMENT, "ExactPlaintext::set_slots_device: the encoder's plaintext modulus or ring degree differs");
    enc.encode_device_words(*impl_->ctx, slots, impl_->items, impl_->d, DPFHE_ENCODE_PLAIN, s);
}

// ---- CompactCiphertext ------------------------------------------------------------------------------------------------------
class CompactCiphertext::Impl {
public:
    const Context* ctx = nullptr;
    size_t batch = 0, bytes = 0;
    unsigned bits[2] = {0, 0};
    uint8_t* d = nullptr;
    ~Impl() { if (d) (void)hipFree(d); }
};
CompactCiphertext::CompactCiphertext(const Context& ctx, size_t batch, unsigned bits0, unsigned bits1) : impl_(new Impl) {
    if (batch == 0) throw Exception(ErrorCode::INVALID_ARGUMENT, "CompactCiphertext: batch must be > 0");
    if (bits0 < 8 || bits0 > 60 || bits1 < 8 || bits1 > 60) throw Exception(ErrorCode::INVALID_ARGUMENT, "CompactCiphertext: widths must lie in [8, 60]");
    impl_->ctx = &ctx; impl_->batch = batch; impl_->bits[0] = bits0; impl_->bits[1] = bits1;
    impl_->bytes = batch * (ctx.params().n() * (bits0 + bits1) / 8);
    impl_->d = device_alloc<uint8_t>(ctx.device_id(), impl_->bytes);
}
CompactCiphertext::~CompactCiphertext() = default;
size_t CompactCiphertext::batch() const { return impl_->batch; }
unsigned CompactCiphertext::bits(unsigned c) const {
    if (c > 1) throw Exception(ErrorCode::INVALID_ARGUMENT, "CompactCiphertext::bits: component 0 or 1");
    return impl_->bits[c];
}
size_t CompactCiphertext::ring_degree() const { return impl_->ctx->params().n(); }
size_t CompactCiphertext::bytes() const { return impl_->bytes; }
uint8_t* CompactCiphertext::data() { return impl_->d; }
const uint8_t* CompactCiphertext::data() const { return impl_->d; }
void CompactCiphertext::copy_to_host(uint8_t* dst) const {
    if (!dst) throw Exception(ErrorCode::INVALID_ARGUMENT, "CompactCiphertext::copy_to_host: null destination");
    hip_check(hipMemcpy(dst, impl_->d, impl_->bytes, hipMemcpyDeviceToHost), "hipMemcpy D2H");
}
void CompactCiphertext::copy_from_host(const uint8_t* src) {
    if (!src) throw Exception(ErrorCode::INVALID_ARGUMENT, "CompactCiphertext::copy_from_host: null source");
    hip_check(hipMemcpy(impl_->d, src, impl_->bytes, hipMemcpyHostToDevice), "hipMemcpy H2D");
}

namespace {
const char kCompactMagic[8] = {'D', 'P', 'F', 'H', 'E', 'c', '1', 0};
struct CompactHeader {   // DPFHEc1 (wire.py _CHDR): all little-endian
    char magic[8];
    uint32_t log2_n, bits0, bits1, reserved;
    uint64_t batch;
};
static_assert(sizeof(CompactHeader) == 32, "the DPFHEc1 header is 32 bytes");
}  // namespace

void CompactCiphertext::save(std::ostream& os) const {
    CompactHeader h{};
    std::memcpy(h.magic, kCompactMagic, 8);
    h.log2_n = impl_->ctx->params().log2_n; h.bits0 = impl_->bits[0]; h.bits1 = impl_->bits[1]; h.reserved = 0; h.batch = impl_->batch;
    std::vector<uint8_t> host(impl_->bytes);
    copy_to_host(host.data());
    os.write(reinterpret_cast<const char*>(&h), sizeof h);
    os.write(reinterpret_cast<const char*>(host.data()), (std::streamsize)host.size());
    if (!os) throw Exception(ErrorCode::RUNTIME_ERROR, "CompactCiphertext::save: stream write failed");
}
void CompactCiphertext::load(std::istream& is) {
    CompactHeader h{};
    is.read(reinterpret_cast<char*>(&h), sizeof h);
    if (!is || std::memcmp(h.magic, kCompactMagic, 8) != 0) throw Exception(ErrorCode::INVALID_ARGUMENT, "CompactCiphertext::load: not a DPFHEc1 stream");
    if (h.log2_n != impl_->ctx->params().log2_n || h.bits0 != impl_->bits[0] || h.bits1 != impl_->bits[1] || h.reserved != 0 || h.batch != impl_->batch)
        throw Exception(ErrorCode::INVALID_ARGUMENT, "CompactCiphertext::load: header does not match this object (log2_n / widths / batch)");
    std::vector<uint8_t> host(impl_->bytes);
    is.read(reinterpret_cast<char*>(host.data()), (std::streamsize)host.size());
    if (!is) throw Exception(ErrorCode::INVALID_ARGUMENT, "CompactCiphertext::load: truncated stream");
    copy_from_host(host.data());
}
std::pair<unsigned, unsigned> CompactCiphertext::recommended_bits(unsigned log2_n, uint64_t t) {
    if (log2_n < 8 || log2_n > 16 || t < 2 || (t >> 32)) throw Exception(ErrorCode::INVALID_ARGUMENT, "recommended_bits: log2_n in [8, 16], t in [2, 2^32)");
    const double lt = std::log2((double)t);
    const unsigned k0 = std::max(8u, (unsigned)std::ceil(lt) + 2);
    const unsigned k1 = std::max(8u, (unsigned)std::ceil(lt + 3 + std::log2(std::sqrt((double)(1u << log2_n) * std::log(std::pow(2.0, 65)) / 2))));
    if (k1 > 60) throw Exception(ErrorCode::INVALID_ARGUMENT, "recommended_bits: width above 60 bits");
    return {k0, k1};
}

RelinKeys::RelinKeys(const Context& ctx) : PolyBuffer(ctx, ctx.params().n_limbs(), 2, /*is_ntt=*/true) {}
GaloisKeys::GaloisKeys(const Context& ctx, uint32_t galois_elt) : PolyBuffer(ctx, ctx.params().n_limbs(), 2, /*is_ntt=*/true), galois_elt_(galois_elt) {
    if (!(galois_elt & 1u) || galois_elt >= 2 * ctx.params().n()) throw Exception(ErrorCode::INVALID_ARGUMENT, "GaloisKeys: galois_elt must be odd and < 2N");
}

// ---- Evaluator --------------------------------------------------------------------------------------------
class Evaluator::Impl {
public:
    const Context* ctx = nullptr;
    dpfhe_ctx* h() const { return handle_of(*ctx); }
    size_t npolys(const PolyBuffer& b) const { return b.batch() * b.size(); }
    static void same(const PolyBuffer& a, const PolyBuffer& b, const char* what) {
        if (a.batch() != b.batch() || a.size() != b.size()) throw Exception(ErrorCode::INVALID_ARGUMENT, std::string(what) + ": operand shapes differ");
        if (a.is_ntt() != b.is_ntt()) throw Exception(ErrorCode::INVALID_STATE, std::string(what) + ": operands are in different domains");
    }
};

Evaluator::Evaluator(const Context& ctx) : impl_(new Impl) { impl_->ctx = &ctx; }
Evaluator::~Evaluator() = default;

void Evaluator::transform_to_ntt_inplace(PolyBuffer& x, Stream* s) const {
    if (x.is_ntt()) return;
    check(dpfhe_ntt_fwd(impl_->h(), x.data(), impl_->npolys(x), s), "dpfhe_ntt_fwd");
    x.set_ntt(true);
}
void Evaluator::transform_from_ntt_inplace(PolyBuffer& x, Stream* s) const {
    if (!x.is_ntt()) return;
    check(dpfhe_ntt_inv(impl_->h(), x.data(), impl_->npolys(x), s), "dpfhe_ntt_inv");
    x.set_ntt(false);
}
void Evaluator::add(const PolyBuffer& a, const PolyBuffer& b, PolyBuffer& out, Stream* s) const {
    Impl::same(a, b, "add");
    if (out.words() != a.words()) throw Exception(ErrorCode::INVALID_ARGUMENT, "add: output shape differs");
    check(dpfhe_add(impl_->h(), out.data(), a.data(), b.data(), impl_->npolys(a), s), "dpfhe_add");
    out.set_ntt(a.is_ntt());
}
void Evaluator::sub(const PolyBuffer& a, const PolyBuffer& b, PolyBuffer& out, Stream* s) const {
    Impl::same(a, b, "sub");
    if (out.words() != a.words()) throw Exception(ErrorCode::INVALID_ARGUMENT, "sub: output shape differs");
    check(dpfhe_sub(impl_->h(), out.data(), a.data(), b.data(), impl_->npolys(a), s), "dpfhe_sub");
    out.set_ntt(a.is_ntt());
}
void Evaluator::negate(const PolyBuffer& a, PolyBuffer& out, Stream* s) const {
    if (out.words() != a.words()) throw Exception(ErrorCode::INVALID_ARGUMENT, "negate: output shape differs");
    check(dpfhe_negate(impl_->h(), out.data(), a.data(), impl_->npolys(a), s), "dpfhe_negate");
    out.set_ntt(a.is_ntt());
}
void Evaluator::dyadic_multiply(const PolyBuffer& a, const PolyBuffer& b, PolyBuffer& out, Stream* s) const {
    Impl::same(a, b, "dyadic_multiply");
    if (out.words() != a.words()) throw Exception(ErrorCode::INVALID_ARGUMENT, "dyadic_multiply: output shape differs");
    check(dpfhe_dyadic_mul(impl_->h(), out.data(), a.data(), b.data(), impl_->npolys(a), s), "dpfhe_dyadic_mul");
    out.set_ntt(a.is_ntt());
}
void Evaluator::dyadic_multiply_add(const PolyBuffer& a, const PolyBuffer& b, PolyBuffer& acc, Stream* s) const {
    Impl::same(a, b, "dyadic_multiply_add");
    Impl::same(a, acc, "dyadic_multiply_add");
    check(dpfhe_dyadic_mul_add(impl_->h(), acc.data(), a.data(), b.data(), impl_->npolys(a), s), "dpfhe_dyadic_mul_add");
}
void Evaluator::multiply(const Ciphertext& a, const Ciphertext& b, Ciphertext& out, Stream* s) const {
    Impl::same(a, b, "multiply");
    if (a.size() != 2) throw Exception(ErrorCode::INVALID_ARGUMENT, "multiply: inputs must be 2-component ciphertexts");
    if (out.size() != 3 || out.batch() != a.batch()) throw Exception(ErrorCode::INVALID_ARGUMENT, "multiply: output must be a 3-component ciphertext of the same batch");
    const uint32_t flags = (a.is_ntt() ? (uint32_t)DPFHE_IN_NTT : 0u) | (out.is_ntt() ? (uint32_t)DPFHE_OUT_NTT : 0u);
    check(dpfhe_ct_mul(impl_->h(), out.data(), a.data(), b.data(), a.batch(), flags, s), "dpfhe_ct_mul");
}
void Evaluator::multiply_sum(const Ciphertext& a, const Ciphertext& b, size_t terms, bool b_shared, Ciphertext& out, Stream* s) const {
    if (a.is_ntt() != b.is_ntt()) throw Exception(ErrorCode::INVALID_STATE, "multiply_sum: operands are in different domains");
    if (a.size() != 2 || b.size() != 2) throw Exception(ErrorCode::INVALID_ARGUMENT, "multiply_sum: inputs must be 2-component ciphertexts");
    if (terms == 0 || a.batch() % terms || b.batch() != (b_shared ? terms : a.batch()))
        throw Exception(ErrorCode::INVALID_ARGUMENT, "multiply_sum: a holds groups * terms items, b as many or, shared, terms items");
    const size_t groups = a.batch() / terms;
    if (out.size() != 3 || out.batch() != groups) throw Exception(ErrorCode::INVALID_ARGUMENT, "multiply_sum: output must be a 3-component ciphertext of one item per group");
    const uint32_t flags = (a.is_ntt() ? (uint32_t)DPFHE_IN_NTT : 0u) | (out.is_ntt() ? (uint32_t)DPFHE_OUT_NTT : 0u);
    check(dpfhe_ct_mul_sum(impl_->h(), out.data(), a.data(), b.data(), groups, terms, b_shared ? 1 : groups, flags, s), "dpfhe_ct_mul_sum");
}
void Evaluator::relinearize(const Ciphertext& in3, const RelinKeys& keys, Ciphertext& out2, Stream* s) const {
    if (in3.is_ntt()) throw Exception(ErrorCode::INVALID_STATE, "relinearize: input must be in the coefficient domain");
    if (in3.size() != 3 || out2.size() != 2 || out2.batch() != in3.batch())
        throw Exception(ErrorCode::INVALID_ARGUMENT, "relinearize: 3-component input, 2-component output of the same batch");
    check(dpfhe_relinearize(impl_->h(), out2.data(), in3.data(), keys.data(), in3.batch(), s), "dpfhe_relinearize");
    out2.set_ntt(false);
}
void Evaluator::rescale(const Ciphertext& in, Ciphertext& out, Stream* s) const {
    if (in.is_ntt()) throw Exception(ErrorCode::INVALID_STATE, "rescale: input must be in the coefficient domain");
    const size_t L = impl_->ctx->params().n_limbs(), n = impl_->ctx->params().n();
    if (L < 2) throw Exception(ErrorCode::INVALID_STATE, "rescale: no limb left to drop");
    if (out.size() != in.size() || out.batch() != in.batch() || out.words() != in.batch() * in.size() * (L - 1) * n)
        throw Exception(ErrorCode::INVALID_ARGUMENT, "rescale: output must live on the next-level context (L-1 limbs), same size and batch");
    check(dpfhe_rescale(impl_->h(), out.data(), in.data(), in.batch() * in.size(), s), "dpfhe_rescale");
    out.set_ntt(false);
}
namespace {
void add_plain_exact_impl(const Context& ctx, const Ciphertext& in, const ExactPlaintext& p, Ciphertext& out, bool negate, Stream* s, const char* what) {
    const FheParams& fp = ctx.params();
    if (in.is_ntt()) throw Exception(ErrorCode::INVALID_ARGUMENT, std::string(what) + ": input must be in the coefficient domain");
    if ((in.size() != 2 && in.size() != 3) || in.words() != in.batch() * in.size() * fp.n_limbs() * fp.n())
        throw Exception(ErrorCode::INVALID_ARGUMENT, std::string(what) + ": input must be a 2- or 3-component ciphertext of this context");
    if (out.size() != in.size() || out.batch() != in.batch() || out.words() != in.words())
        throw Exception(ErrorCode::INVALID_ARGUMENT, std::string(what) + ": output shape differs");
    if (p.ring_degree() != fp.n() || in.batch() % p.items())
        throw Exception(ErrorCode::INVALID_ARGUMENT, std::string(what) + ": plaintext of another ring degree, or a batch that is not a multiple of its items");
    check(dpfhe_add_plain_scaled(handle_of(ctx), out.data(), in.data(), p.data(), in.batch(), in.size(), p.items(), p.plain_modulus(),
                                 negate ? 1 : 0, s),
          "dpfhe_add_plain_scaled");
    out.set_ntt(false);
}
void add_plain_impl(const Context& ctx, const Ciphertext& in, const Plaintext& p, Ciphertext& out, bool negate, Stream* s, const char* what) {
    const FheParams& fp = ctx.params();
    const size_t poly = fp.n_limbs() * fp.n();
    if ((in.size() != 2 && in.size() != 3) || in.batch() == 0 || in.words() != in.batch() * in.size() * poly)
        throw Exception(ErrorCode::INVALID_ARGUMENT, std::string(what) + ": input must be a 2- or 3-component ciphertext of this context");
    if (out.size() != in.size() || out.batch() != in.batch() || out.words() != in.words())
        throw Exception(ErrorCode::INVALID_ARGUMENT, std::string(what) + ": output shape differs");
    if (p.batch() == 0 || p.words() != p.batch() * poly || in.batch() % p.batch())
        throw Exception(ErrorCode::INVALID_ARGUMENT, std::string(what) + ": plaintext of another context, or a batch that is not a multiple of its items");
    if (in.is_ntt() != p.is_ntt()) throw Exception(ErrorCode::INVALID_STATE, std::string(what) + ": ciphertext and plaintext are in different domains");
    check(dpfhe_add_plain(handle_of(ctx), out.data(), in.data(), p.data(), in.batch(), in.size(), p.batch(), negate ? 1 : 0, s), "dpfhe_add_plain");
    out.set_ntt(in.is_ntt());
}
}  // namespace
void Evaluator::add_plain(const Ciphertext& in, const Plaintext& p, Ciphertext& out, Stream* s) const {
    add_plain_impl(*impl_->ctx, in, p, out, false, s, "add_plain");
}
void Evaluator::sub_plain(const Ciphertext& in, const Plaintext& p, Ciphertext& out, Stream* s) const {
    add_plain_impl(*impl_->ctx, in, p, out, true, s, "sub_plain");
}
void Evaluator::add_plain_exact(const Ciphertext& in, const ExactPlaintext& p, Ciphertext& out, Stream* s) const {
    add_plain_exact_impl(*impl_->ctx, in, p, out, false, s, "add_plain_exact");
}
void Evaluator::sub_plain_exact(const Ciphertext& in, const ExactPlaintext& p, Ciphertext& out, Stream* s) const {
    add_plain_exact_impl(*impl_->ctx, in, p, out, true, s, "sub_plain_exact");
}
void Evaluator::compact(const Ciphertext& in, CompactCiphertext& out, Stream* s) const {
    const FheParams& fp = impl_->ctx->params();
    if (in.is_ntt()) throw Exception(ErrorCode::INVALID_STATE, "compact: input must be in the coefficient domain");
    if (in.size() != 2 || in.words() != in.batch() * 2 * fp.n_limbs() * fp.n())
        throw Exception(ErrorCode::INVALID_ARGUMENT, "compact: input must be a 2-component ciphertext of this context");
    if (out.batch() != in.batch() || out.ring_degree() != fp.n()) throw Exception(ErrorCode::INVALID_ARGUMENT, "compact: batch or ring degree differs");
    check(dpfhe_compact(impl_->h(), out.data(), in.data(), in.batch(), out.bits(0), out.bits(1), s), "dpfhe_compact");
}
// ---- ExactMultiplier ------------------------------------------------------------------------------------------------------------
class ExactMultiplier::Impl {
public:
    const Context* work = nullptr;
    const Context* level = nullptr;
    uint64_t t = 0;
    size_t ll = 0, L = 0, n = 0;
    std::unique_ptr<Ciphertext> A, B, T;     // operands and tensor product on all work limbs
    std::unique_ptr<PolyBuffer> W;           // scaled product on the workspace limbs: [batch * 3][L - ll][N], kept as a 1-component buffer on `work`-sized storage
    size_t cap = 0;
    void ensure(size_t batch) {
        if (batch <= cap) return;
        A.reset(new Ciphertext(*work, 2, batch));
        B.reset(new Ciphertext(*work, 2, batch));
        T.reset(new Ciphertext(*work, 3, batch));
        W.reset(new PolyBuffer(*work, batch, 3, false));   // 3 L N words per item: room for 3 (L - ll) N
        cap = batch;
    }
};
ExactMultiplier::ExactMultiplier(const Context& work_ctx, const Context& level_ctx, uint64_t plain_modulus) : impl_(new Impl) {
    const FheParams &pw = work_ctx.params(), &pl = level_ctx.params();
    impl_->work = &work_ctx; impl_->level = &level_ctx; impl_->t = plain_modulus;
    impl_->ll = pl.n_limbs(); impl_->L = pw.n_limbs(); impl_->n = pw.n();
    if (pl.log2_n != pw.log2_n || impl_->ll == 0 || impl_->ll >= impl_->L || impl_->ll > (work_ctx.uses_fold() ? 9u : 8u) || impl_->L > 20 || impl_->L - impl_->ll > (work_ctx.uses_fold() ? 10u : 8u) || work_ctx.device_id() != level_ctx.device_id() || plain_modulus < 2)
        throw Exception(ErrorCode::INVALID_ARGUMENT, "ExactMultiplier: the level context must hold the first 1..9 limbs (1..8 with generic primes) of the work context, which has at most 20 and at most 10 (generic primes: 8) beyond the level (same ring degree and device)");
    for (size_t i = 0; i < impl_->ll; ++i)
        if (pl.moduli[i] != pw.moduli[i]) throw Exception(ErrorCode::INVALID_ARGUMENT, "ExactMultiplier: the level's moduli must be the first moduli of the work context");
    double lq = 0, lQ = 0, lW = 0;
    for (size_t i = 0; i < impl_->L; ++i) { const double b = std::log2((double)pw.moduli[i]); lQ += b; if (i < impl_->ll) lq += b; else lW += b; }
    const double lnt = (double)pw.log2_n + std::log2((double)plain_modulus);
    if (lQ - 1 <= lnt + 2 * lq + 1 || lW - 1 <= lnt + lq + 2)
        throw Exception(ErrorCode::INVALID_STATE, "ExactMultiplier: the work context is too small for the integer tensor product of this level (needs Q > 2 N t q^2)");
}
ExactMultiplier::~ExactMultiplier() = default;
void ExactMultiplier::multiply(const Ciphertext& a, const Ciphertext& b, Ciphertext& out3, Stream* s) {
    Impl& I = *impl_;
    const size_t batch = a.batch(), lvl_words = I.ll * I.n;
    if (a.is_ntt() || b.is_ntt()) throw Exception(ErrorCode::INVALID_STATE, "ExactMultiplier::multiply: operands must be in the coefficient domain");
    if (a.size() != 2 || b.size() != 2 || out3.size() != 3 || b.batch() != batch || out3.batch() != batch || a.words() != batch * 2 * lvl_words || out3.words() != batch * 3 * lvl_words)
        throw Exception(ErrorCode::INVALID_ARGUMENT, "ExactMultiplier::multiply: 2-component operands and a 3-component output of one batch on the level context");
    I.ensure(batch);
    dpfhe_ctx* h = handle_of(*I.work);
    const bool square = a.data() == b.data();
    check(dpfhe_base_extend(h, I.A->data(), I.L, a.data(), I.ll, 0, (uint32_t)I.ll, 0, (uint32_t)I.L, batch * 2, s), "dpfhe_base_extend");
    if (!square) check(dpfhe_base_extend(h, I.B->data(), I.L, b.data(), I.ll, 0, (uint32_t)I.ll, 0, (uint32_t)I.L, batch * 2, s), "dpfhe_base_extend");
    check(dpfhe_ct_mul(h, I.T->data(), I.A->data(), square ? I.A->data() : I.B->data(), batch, 0, s), "dpfhe_ct_mul");
    check(dpfhe_scale_round(h, I.W->data(), I.L - I.ll, I.T->data(), 0, (uint32_t)I.ll, (uint32_t)I.ll, (uint32_t)(I.L - I.ll), I.t, batch * 3, s), "dpfhe_scale_round");
    check(dpfhe_base_extend(h, out3.data(), I.ll, I.W->data(), I.L - I.ll, (uint32_t)I.ll, (uint32_t)(I.L - I.ll), 0, (uint32_t)I.ll, batch * 3, s), "dpfhe_base_extend");
    out3.set_ntt(false);
}

void Evaluator::apply_galois(const Ciphertext& in2, const GaloisKeys& keys, Ciphertext& out2, Stream* s) const {
    if (in2.is_ntt()) throw Exception(ErrorCode::INVALID_STATE, "apply_galois: input must be in the coefficient domain");
    if (in2.size() != 2 || out2.size() != 2 || out2.batch() != in2.batch())
        throw Exception(ErrorCode::INVALID_ARGUMENT, "apply_galois: 2-component input and output of the same batch");
    Ciphertext rotated(*impl_->ctx, 2, in2.batch());
    check(dpfhe_apply_galois(impl_->h(), rotated.data(), in2.data(), in2.batch() * 2, keys.galois_elt(), s), "dpfhe_apply_galois");
    check(dpfhe_switch_key(impl_->h(), out2.data(), rotated.data(), keys.data(), in2.batch(), s), "dpfhe_switch_key");
    hip_check(hipStreamSynchronize(static_cast<hipStream_t>(s)), "hipStreamSynchronize");  // `rotated` is freed on return
    out2.set_ntt(false);
}
void Evaluator::multiply_plain(const Ciphertext& a, const Plaintext& p, Ciphertext& out, Stream* s) const {
    if (!a.is_ntt() || !p.is_ntt()) throw Exception(ErrorCode::INVALID_STATE, "multiply_plain: operands must be in the NTT domain");
    if (p.batch() != 1 || out.words() != a.words()) throw Exception(ErrorCode::INVALID_ARGUMENT, "multiply_plain: one plaintext, output shaped like the input");
    check(dpfhe_multiply_plain(impl_->h(), out.data(), a.data(), p.data(), a.batch() * a.size(), s), "dpfhe_multiply_plain");
    out.set_ntt(true);
}
void Evaluator::matvec_plain(const Plaintext& W, const Ciphertext& x, Ciphertext& y, Stream* s) const {
    if (!W.is_ntt() || !x.is_ntt()) throw Exception(ErrorCode::INVALID_STATE, "matvec_plain: operands must be in the NTT domain");
    const size_t cols = x.batch(), rows = y.batch();
    if (x.size() != 2 || y.size() != 2 || cols == 0 || W.batch() != rows * cols) throw Exception(ErrorCode::INVALID_ARGUMENT, "matvec_plain: W batch must be rows*cols, x/y 2-component");
    check(dpfhe_matvec_plain(impl_->h(), y.data(), W.data(), x.data(), rows, cols, s), "dpfhe_matvec_plain");
    y.set_ntt(true);
}
void Evaluator::matvec_plain_multi(const Plaintext& W, const Ciphertext& x, Ciphertext& y, size_t n_rhs, Stream* s) const {
    if (!W.is_ntt() || !x.is_ntt()) throw Exception(ErrorCode::INVALID_STATE, "matvec_plain_multi needs NTT-domain operands");
    if (n_rhs == 0 || x.size() != 2 || y.size() != 2 || x.batch() % n_rhs || y.batch() % n_rhs)
        throw Exception(ErrorCode::INVALID_ARGUMENT, "matvec_plain_multi: x [cols][n_rhs], y [rows][n_rhs] 2-component items");
    const size_t cols = x.batch() / n_rhs, rows = y.batch() / n_rhs;
    if (W.batch() != rows * cols) throw Exception(ErrorCode::INVALID_ARGUMENT, "matvec_plain_multi: W must hold rows * cols plaintexts");
    check(dpfhe_matvec_plain_multi(impl_->h(), y.data(), W.data(), x.data(), rows, cols, n_rhs, s), "dpfhe_matvec_plain_multi");
    y.set_ntt(true);
}

void Evaluator::matvec_scalar(const ScalarMatrix& W, const Ciphertext& x, Ciphertext& y, Stream* s) const {
    if (x.size() != 2 || y.size() != 2 || x.batch() != W.cols() || y.batch() != W.rows())
        throw Exception(ErrorCode::INVALID_ARGUMENT, "matvec_scalar: x batch = cols, y batch = rows, 2-component ciphertexts");
    check(dpfhe_matvec_scalar(impl_->h(), y.data(), W.data(), x.data(), W.rows(), W.cols(), s), "dpfhe_matvec_scalar");
    y.set_ntt(x.is_ntt());
}
void Evaluator::reduce_sum(const PolyBuffer& in, PolyBuffer& out, Stream* s) const {
    if (out.batch() != 1 || out.size() != in.size()) throw Exception(ErrorCode::INVALID_ARGUMENT, "reduce_sum: output must be one item of the same size");
    check(dpfhe_reduce_sum(impl_->h(), out.data(), in.data(), in.batch(), in.size(), s), "dpfhe_reduce_sum");
    out.set_ntt(in.is_ntt());
}

// =====================================================================================================================
// (e) Communicator: dpfhe_comm_* behind the facade
// =====================================================================================================================
class Communicator::Impl {
public:
    dpfhe_comm* h = nullptr;
    int rank = 0, world = 1;
};
std::vector<uint8_t> Communicator::unique_id() {
    std::vector<uint8_t> id(128);
    check(dpfhe_comm_unique_id(id.data()), "dpfhe_comm_unique_id");
    return id;
}
Communicator::Communicator(const std::vector<uint8_t>& id, int rank, int world_size, int device_id) : impl_(new Impl) {
    if (id.size() != 128) throw Exception(ErrorCode::INVALID_ARGUMENT, "Communicator: the id is 128 bytes");
    check(dpfhe_comm_create(&impl_->h, id.data(), rank, world_size, device_id), "dpfhe_comm_create");
    impl_->rank = rank; impl_->world = world_size;
}
Communicator::~Communicator() { if (impl_ && impl_->h) dpfhe_comm_destroy(impl_->h); }
int Communicator::rank() const { return impl_->rank; }
int Communicator::world_size() const { return impl_->world; }
void Communicator::all_gather(const PolyBuffer& send, PolyBuffer& recv, Stream* stream) const {
    if (recv.batch() != send.batch() * (size_t)impl_->world || recv.size() != send.size())
        throw Exception(ErrorCode::INVALID_ARGUMENT, "all_gather: recv must hold world_size x send items of the same size");
    check(dpfhe_comm_allgather(impl_->h, recv.data(), send.data(), send.words(), stream), "dpfhe_comm_allgather");
    recv.set_ntt(send.is_ntt());
}

// kBabyShiftDefault, the packed layers' default baby-step shift, moved to fhe_packed.cpp with the layers that read it.

}  // namespace fhe
}  // namespace deeppowers
