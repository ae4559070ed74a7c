// deeppowers/fhe.hpp - C++ operator API of the FHE ciphertext-arithmetic hot path.
//
// The reference has no Ciphertext/Evaluator to keep, so this is the BUILD-SPEC
// API of SURVEY.md section 8(a)/(b), written in the reference's house style so that it reads like the
// rest of deeppowers:
//   - namespace deeppowers                     (/root/reference/src/core/hal/hal.hpp:8)
//   - pimpl with std::unique_ptr<Impl>         (/root/reference/src/api/cpp/include/deeppowers.hpp:73-75)
//   - heavy objects are non-copyable           (/root/reference/src/core/execution/model.hpp:88-89)
//   - errors are exceptions carrying ErrorCode (/root/reference/src/common/error.hpp:42-53)
//   - device chosen by id                      (/root/reference/src/api/cpp/src/deeppowers.cpp:15)
//   - optional stream as the last argument     (/root/reference/src/core/hal/hal.hpp:95)
// Host code stays C++; every operation is one call through the C ABI of include/dpfhe.h into HIP kernels.
// An encrypted linear layer at the reference's matmul sites
// (/root/reference/src/core/execution/models/gpt_model.cpp:793,848,883) is Evaluator::matvec_plain.
#pragma once

#include <complex>
#include <cstddef>
#include <cstdint>
#include <iosfwd>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace deeppowers {
namespace fhe {

// numbers of deeppowers::common::ErrorCode (/root/reference/src/common/error.hpp:10-40)
enum class ErrorCode { SUCCESS = 0, OUT_OF_MEMORY = 1001, DEVICE_ERROR = 1002, INVALID_ARGUMENT = 2000, INVALID_STATE = 2002, RUNTIME_ERROR = 3000 };

class Exception : public std::runtime_error {
public:
    Exception(ErrorCode code, const std::string& message) : std::runtime_error(message), code_(code) {}
    ErrorCode code() const { return code_; }

private:
    ErrorCode code_;
};

using Stream = void;  // a hipStream_t; nullptr = the null stream

// Seed of a seeded ciphertext or key: its uniform component (c1 of a fresh symmetric ciphertext, a_j of a key) is expand(seed, item, limb, component)
// (include/dpfhe.h dpfhe_expand_uniform) and travels as these 32 bytes instead of L N words per item.  The seed is PUBLIC - it stands for a public
// uniform polynomial; security rests on ChaCha20 as a PRG with a public seed.  It must never be reused under one secret key: equal c1 would make
// c0 - c0' = scale (m - m') + e - e' public.  Every *_seeded call below draws a fresh one (and the item index is part of the nonce).
struct Seed {
    uint8_t bytes[32];
};

struct FheParams {
    uint32_t log2_n = 0;
    std::vector<uint64_t> moduli;  // primes < 2^60, q = 1 (mod 2N)
    std::vector<uint64_t> psi;     // primitive 2N-th roots of unity
    size_t n() const { return size_t(1) << log2_n; }
    size_t n_limbs() const { return moduli.size(); }
    FheParams drop_last_limb() const;  // the level after a rescale
    static FheParams config1();     // N=1024, one 30-bit limb       (BASELINE.json configs[0])
    static FheParams n4096_l4();    // N=4096, 4 x 60-bit limbs      (configs[1..3], the metric)
    static FheParams n8192_l6();    // N=8192, 6 x 60-bit limbs      (configs[4] sizes)
    static FheParams n16384(size_t n_limbs);  // N=16384, the first n_limbs (<= 8) primes below 2^60 that are 1 mod 2^15: a ring with room for a security margin
    static FheParams n8192(size_t n_limbs);   // N=8192, the first n_limbs (<= 20) primes of the same descending chain: deeper levels, multiply workspaces
    // N=32768, the first n_limbs (<= 14) primes below 2^60 that are 1 mod 2^16 (deeppowers_amd/params.py ntt_primes(15, n)): the ring whose 128-bit budget (881
    // bits) holds two or three activated blocks.  The first 8 are fold primes (2^60 - d, d < 2^24: 480 bits on the fast arithmetic); a context that holds any
    // of primes 9..14 runs the context-wide generic arithmetic on every limb, as every mixed context above N = 16384 does.
    static FheParams n32768(size_t n_limbs);
};

class PolyBuffer;
class Context {
public:
    explicit Context(const FheParams& params, int device_id = 0);
    ~Context();
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;

    const FheParams& params() const;
    int device_id() const;
    bool uses_fold() const;
    // arithmetic of limb i in the batched transforms and the fused multiply (dpfhe_ctx_limb_class): 0 Shoup, 1 fold, 2 f64, 3 fold-scaled
    int limb_class(uint32_t limb) const;
    // scratch arenas of the composed large-ring operations, one per stream (dpfhe_ctx_release_scratch / dpfhe_ctx_scratch_bytes)
    void release_scratch(void* stream = nullptr, bool all_streams = false);
    size_t scratch_bytes() const;
    void* handle() const;  // dpfhe_ctx*
    void synchronize() const;
    // set-up call: slice size (MiB of scratch) of the operations composed from the batched transforms at N >= 16384 (dpfhe_ctx_set_scratch_limit; default 1024)
    void set_scratch_limit(size_t mib);
    // Which form of the fused multiply Evaluator::multiply launches (include/dpfhe.h "A0, continued": the ring degree's default; autotune()
    // is the explicit opt-in measurement, in the spirit of the reference's AutoTuner, src/core/inference/auto_tuner.hpp:26-64).  Both forms give the same words.
    struct TuneInfo {
        std::string chosen, source;                                // e.g. "quad", "default"
        std::vector<std::pair<std::string, float>> probe_us;       // microseconds per probe launch of each measured form
        unsigned probe_pairs = 0, probe_reps = 0;
    };
    TuneInfo tune_info() const;
    TuneInfo autotune(PolyBuffer& scratch, unsigned reps = 3);    // re-measure on the caller's buffer (overwritten; >= 7 RNS polynomials)

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// Device-resident words [batch][components][L][N]; owner of its buffer.
class PolyBuffer {
public:
    PolyBuffer(const Context& ctx, size_t batch, size_t components, bool is_ntt);
    ~PolyBuffer();
    PolyBuffer(PolyBuffer&&) noexcept;
    PolyBuffer& operator=(PolyBuffer&&) noexcept;
    PolyBuffer(const PolyBuffer&) = delete;
    PolyBuffer& operator=(const PolyBuffer&) = delete;

    uint64_t* data();
    const uint64_t* data() const;
    size_t batch() const;
    size_t size() const;   // components per item
    size_t words() const;  // batch * size * L * N
    bool is_ntt() const;
    void set_ntt(bool v);
    const Context& context() const;   // the context the buffer was made for
    void copy_from_host(const uint64_t* src);  // words() canonical residues
    void copy_to_host(uint64_t* dst) const;
    // N4: wire format.  Little-endian: "DPFHEv1\0", u32 log2_n, u32 n_limbs, u64 batch, u64 components,
    // u32 is_ntt, u32 reserved, u64 moduli[n_limbs], then batch*components*n_limbs*N u64 words.  load() checks that the
    // header matches this buffer's context and shape (throws INVALID_ARGUMENT otherwise) and sets the domain flag.
    void save(std::ostream& os) const;
    void load(std::istream& is);
    // Seeded stream "DPFHEs1\0": component `component` of items 0 .. batch-1 must be expand(seed, first_item + b, ., component); it is left out.
    // 80-byte header (little-endian): magic, u32 log2_n, u32 n_limbs, u64 batch, u64 components, u32 is_ntt, u32 expanded_component, u64 first_item,
    // u8 seed[32]; then u64 moduli[n_limbs]; then the other components' words [batch][components-1][L][N].  save_seeded re-expands and compares
    // first: a buffer that no longer matches its seed (overwritten, transformed) throws INVALID_STATE, so no stale seed is ever written.
    // load_seeded checks the header as load() does, uploads the stored components and expands the missing one on the device (on `stream`); it
    // synchronises `stream` before returning (the host staging buffer is released).
    void save_seeded(std::ostream& os, const Seed& seed, uint32_t component = 1, uint64_t first_item = 0) const;
    void load_seeded(std::istream& is, Stream* stream = nullptr);

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

class Plaintext : public PolyBuffer {  // A5: one polynomial per item
public:
    explicit Plaintext(const Context& ctx, size_t batch = 1, bool is_ntt = false) : PolyBuffer(ctx, batch, 1, is_ntt) {}
};

class Ciphertext : public PolyBuffer {  // A4: size in {2, 3}
public:
    explicit Ciphertext(const Context& ctx, size_t size = 2, size_t batch = 1, bool is_ntt = false);
};

class BatchEncoder;
// Device plaintext over Z_t for EXACT (BFV-style) ciphertexts - the bias of an encrypted layer: `items` polynomials of N coefficients in [0, t)
// ([items][N] u64 words, include/dpfhe.h dpfhe_add_plain_scaled).  Evaluator::add_plain_exact adds round(Q b / t) to c0, so the ciphertext decrypts to
// (m + b) mod t; item i of a ciphertext batch takes plaintext item i / (batch / items).
class ExactPlaintext {
public:
    // t odd, 3 <= t < 2^32 (coprime to the moduli: checked when it is added); all coefficients start at 0
    ExactPlaintext(const Context& ctx, uint64_t plain_modulus, size_t items = 1);
    ~ExactPlaintext();
    ExactPlaintext(const ExactPlaintext&) = delete;
    ExactPlaintext& operator=(const ExactPlaintext&) = delete;
    void set_coefficients(const int64_t* coeffs);   // items * N values, centred or non-negative: reduced mod t
    void set_slots(const BatchEncoder& enc, const uint64_t* slots);   // items * N slot values < t, encoded on the host with enc (same t)
    // the same coefficients, encoded on the device (include/dpfhe.h dpfhe_encode_slots, DPFHE_ENCODE_PLAIN): items * N 32-bit slot values, a HOST or a
    // DEVICE pointer as for BatchEncoder::encode_device (a device pointer: enqueues on `stream` only; a host pointer: synchronises `stream`)
    void set_slots_device(const BatchEncoder& enc, const uint32_t* slots, Stream* stream = nullptr);
    size_t items() const;
    uint64_t plain_modulus() const;
    size_t ring_degree() const;     // N
    const uint64_t* data() const;   // device, [items][N]

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// Compact result ciphertext (stream "DPFHEc1\0"): a 2-component exact ciphertext switched from Q to 2^k_c per component and bit-packed on the device
// (include/dpfhe.h dpfhe_compact), N (bits0 + bits1) / 8 bytes per item instead of 16 L N.  Device-resident: batch records, item i's record at byte
// i N (bits0 + bits1) / 8, component 0 first, value j of a component at bits [j k, (j + 1) k) of its little-endian bit string.  Only the holder of the
// secret key reads it back (Decryptor::decrypt_exact / noise_budget_bits overloads).  The switch is public: security rests on the secret, as for rescale.
class CompactCiphertext {
public:
    // widths in [8, 60] (recommended_bits); throws INVALID_ARGUMENT otherwise or for batch 0
    CompactCiphertext(const Context& ctx, size_t batch, unsigned bits0, unsigned bits1);
    ~CompactCiphertext();
    CompactCiphertext(const CompactCiphertext&) = delete;
    CompactCiphertext& operator=(const CompactCiphertext&) = delete;
    size_t batch() const;
    unsigned bits(unsigned component) const;
    size_t ring_degree() const;   // N
    size_t bytes() const;         // batch * N (bits0 + bits1) / 8
    uint8_t* data();              // device
    const uint8_t* data() const;
    void copy_to_host(uint8_t* dst) const;        // bytes() bytes
    void copy_from_host(const uint8_t* src);
    // 32-byte little-endian header: magic, u32 log2_n, u32 bits0, u32 bits1, u32 reserved = 0, u64 batch; then the records (32 + bytes() in all).
    // load() checks the header against this object (throws INVALID_ARGUMENT on any difference or a truncated stream).
    void save(std::ostream& os) const;
    void load(std::istream& is);
    // widths for plaintext modulus t at N = 2^log2_n: k0 = ceil(log2 t) + 2, k1 = ceil(log2 t + 3 + log2 sqrt(N ln(2^65) / 2)) (both at least 8).
    // Any ciphertext with a noise budget of at least 2 bits decrypts from them (c0 rounding <= 1/8 of the tolerance, c1 rounding times s <= 1/8 with
    // probability >= 1 - 2^-64 per coefficient).  t = 65537: (19, 27) at N = 2^11, (19, 28) at 2^12 and 2^13, (19, 29) at 2^14.
    static std::pair<unsigned, unsigned> recommended_bits(unsigned log2_n, uint64_t plain_modulus);

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// Plaintext scalar weights of a linear layer: rows x cols integers, stored as one residue per limb ([rows][cols][L]).
class ScalarMatrix {
public:
    ScalarMatrix(const Context& ctx, size_t rows, size_t cols);
    ~ScalarMatrix();
    ScalarMatrix(const ScalarMatrix&) = delete;
    ScalarMatrix& operator=(const ScalarMatrix&) = delete;
    void set(const int64_t* weights);  // rows*cols signed integers, row-major
    size_t rows() const;
    size_t cols() const;
    const uint64_t* data() const;      // device

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// N1: evaluation keys for relinearisation: L digits x 2 polynomials, NTT domain
// (evk_j = (-(a_j s) + e_j + g_j s^2, a_j), g_j = CRT basis element of limb j; layout [L][2][L][N]).
class RelinKeys : public PolyBuffer {
public:
    explicit RelinKeys(const Context& ctx);
};

// N3: switching key from sigma_g(s) to s for one Galois element g (odd, < 2N); same layout as RelinKeys.
class GaloisKeys : public PolyBuffer {
public:
    GaloisKeys(const Context& ctx, uint32_t galois_elt);
    uint32_t galois_elt() const { return galois_elt_; }

private:
    uint32_t galois_elt_;
};

class Evaluator {
public:
    explicit Evaluator(const Context& ctx);
    ~Evaluator();
    Evaluator(const Evaluator&) = delete;
    Evaluator& operator=(const Evaluator&) = delete;

    // The `stream` argument: every method below enqueues its work on `stream` and returns - no host synchronisation, no work on any other stream, and in
    // steady state no allocation (include/dpfhe.h "Conventions": at log2_n >= 14 the composed operations grow the stream's arena only for a larger
    // batch than before).  The one exception is apply_galois, which holds a temporary and synchronises `stream` before it returns.
    // tests/cpp/test_stream_api.cpp holds every one of them to this.
    // A1 / A2 (in place; flips is_ntt)
    void transform_to_ntt_inplace(PolyBuffer& x, Stream* stream = nullptr) const;
    void transform_from_ntt_inplace(PolyBuffer& x, Stream* stream = nullptr) const;
    // A3 / A8 on whole buffers (same shape and domain)
    void add(const PolyBuffer& a, const PolyBuffer& b, PolyBuffer& out, Stream* stream = nullptr) const;
    void sub(const PolyBuffer& a, const PolyBuffer& b, PolyBuffer& out, Stream* stream = nullptr) const;
    void negate(const PolyBuffer& a, PolyBuffer& out, Stream* stream = nullptr) const;
    void dyadic_multiply(const PolyBuffer& a, const PolyBuffer& b, PolyBuffer& out, Stream* stream = nullptr) const;
    void dyadic_multiply_add(const PolyBuffer& a, const PolyBuffer& b, PolyBuffer& acc, Stream* stream = nullptr) const;
    // A6: the metric op.  out must be a 3-component ciphertext of the same batch; its domain flag selects OUT_NTT.
    void multiply(const Ciphertext& a, const Ciphertext& b, Ciphertext& out, Stream* stream = nullptr) const;
    // A sum of products before any relinearisation (dpfhe_ct_mul_sum): out item g = sum_{k < terms} a item g * terms + k (x) b item g * terms + k, or, with
    // b_shared, b item k for every group (b then holds `terms` items).  a: groups * terms items; out: 3 components, `groups` items, its domain flag selects
    // OUT_NTT as in multiply.  a and b may be the same object (a sum of squares).  The words of multiply per pair summed with add.
    void multiply_sum(const Ciphertext& a, const Ciphertext& b, size_t terms, bool b_shared, Ciphertext& out, Stream* stream = nullptr) const;
    // N1: 3 -> 2 components, coefficient domain in and out
    void relinearize(const Ciphertext& in3, const RelinKeys& keys, Ciphertext& out2, Stream* stream = nullptr) const;
    // N1, second half: out = round(in / q_last) at the next level; `out` must have been created on a Context of
    // params().drop_last_limb() with the same size and batch (coefficient domain)
    void rescale(const Ciphertext& in, Ciphertext& out_next_level, Stream* stream = nullptr) const;
    // N3: ciphertext of m(X) -> ciphertext of m(X^g) under the same key (automorphism + key switch), coefficient domain.  Allocates a temporary and
    // SYNCHRONISES `stream` before returning.
    void apply_galois(const Ciphertext& in2, const GaloisKeys& keys, Ciphertext& out2, Stream* stream = nullptr) const;
    // A7: ct (.) pt per component (NTT domain) and the matrix-vector product y_i = sum_j W_ij (.) x_j
    void multiply_plain(const Ciphertext& a, const Plaintext& p, Ciphertext& out, Stream* stream = nullptr) const;
    void matvec_plain(const Plaintext& W /* batch = rows*cols */, const Ciphertext& x /* batch = cols */, Ciphertext& y /* batch = rows */,
                      Stream* stream = nullptr) const;
    // A7 with n_rhs right-hand sides: x batch = cols * n_rhs laid out [cols][n_rhs], y batch = rows * n_rhs laid out [rows][n_rhs]
    void matvec_plain_multi(const Plaintext& W, const Ciphertext& x, Ciphertext& y, size_t n_rhs, Stream* stream = nullptr) const;
    // A7, scalar weights: y_i = sum_j w_ij * x_j (either domain; y takes x's domain).  x: batch = cols, y: batch = rows.
    // With one ciphertext per input feature and one sample per coefficient this IS the encrypted linear layer that
    // replaces the plaintext matvec sites of the reference (gpt_model.cpp:793,848,883).
    void matvec_scalar(const ScalarMatrix& W, const Ciphertext& x, Ciphertext& y, Stream* stream = nullptr) const;
    // A8: modular sum over the batch -> one item
    void reduce_sum(const PolyBuffer& in, PolyBuffer& out, Stream* stream = nullptr) const;
    // exact plaintext addition / subtraction: out = in with c0 +- round(Q b / t) (dpfhe_add_plain_scaled), so it decrypts to (m +- b) mod t.  in: 2 or 3
    // components (an ExactMultiplier product before relinearisation too), coefficient domain, batch a multiple of p.items(); out: same shape (may be in).
    void add_plain_exact(const Ciphertext& in, const ExactPlaintext& p, Ciphertext& out, Stream* stream = nullptr) const;
    void sub_plain_exact(const Ciphertext& in, const ExactPlaintext& p, Ciphertext& out, Stream* stream = nullptr) const;
    // plaintext addition / subtraction on residues: out = in with c0 +- p mod q_l (dpfhe_add_plain) - p an encoding at the ciphertext's own scale (the
    // approximate family: ComplexEncoder::encode_device), or any plaintext whose residues are to be added as they are.  in: 2 or 3 components, batch a
    // multiple of p.batch() (item i takes plaintext item i / (in.batch() / p.batch())); out: same shape (may be in); either domain, INVALID_STATE when the
    // domain flags of in and p differ.  out takes in's domain flag.
    void add_plain(const Ciphertext& in, const Plaintext& p, Ciphertext& out, Stream* stream = nullptr) const;
    void sub_plain(const Ciphertext& in, const Plaintext& p, Ciphertext& out, Stream* stream = nullptr) const;
    // compact result: out = in switched to 2^k_c and bit-packed (dpfhe_compact; enqueue only).  in: 2 components, coefficient domain, in.batch() items
    // (INVALID_STATE for an NTT-domain input, INVALID_ARGUMENT for 3 components, a batch or ring-degree mismatch, or more than 10 limbs: rescale first).
    void compact(const Ciphertext& in, CompactCiphertext& out, Stream* stream = nullptr) const;

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// ---- round 4: EXACT ciphertext x ciphertext multiply (BFV-style) around the fused tensor-product kernel ---------------------------------
// For ciphertexts that carry their message as floor(q / t) * m (Encryptor::encrypt_exact: slot-packed exact arithmetic mod t) a tensor
// product modulo q is not enough: the product carries floor(q/t)^2 and has to be scaled by t / q over the INTEGERS.  ExactMultiplier does
// that with the level's modulus q = the first `level` limbs of a larger work context (the remaining limbs hold the integer product):
//     extend both operands exactly to all work limbs (dpfhe_base_extend)  ->  Evaluator::multiply on the work context (the fused
//     ct x ct kernel: the metric op)  ->  x t / q with rounding on the workspace limbs (dpfhe_scale_round)  ->  back to the level's limbs.
// Needs prod(work limbs) > 2 N t q^2 (N = 8192, t = 65537, a two-limb level: five 60-bit limbs).  The result has 3 components on the LEVEL
// context (relinearise there).  This is what lets a packed layer's output go through a polynomial activation (x -> x^2 between W_up and
// W_down: /root/reference/src/core/execution/models/gpt_model.cpp:842-859 with the square standing in for GELU).
class ExactMultiplier {
public:
    // level_ctx's moduli must be the first level_ctx.params().n_limbs() moduli of work_ctx, same ring degree, same device
    ExactMultiplier(const Context& work_ctx, const Context& level_ctx, uint64_t plain_modulus);
    ~ExactMultiplier();
    ExactMultiplier(const ExactMultiplier&) = delete;
    ExactMultiplier& operator=(const ExactMultiplier&) = delete;
    // a, b: 2 components on level_ctx (coefficient domain; may be the same object: squaring); out3: 3 components on level_ctx, same batch.
    // Enqueues on `stream`; scratch belongs to the object and grows to the largest batch seen (one multiply() at a time per object).
    void multiply(const Ciphertext& a, const Ciphertext& b, Ciphertext& out3, Stream* stream = nullptr);

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// ---- (e) SURVEY.md section 8e: the one collective of the sharded path -------------------------------------------------
// One process per GPU.  Rank 0 obtains an id, ships its 128 bytes to the other ranks by the host program's own rendezvous
// (a file, a pipe, MPI ...), every rank constructs a Communicator.  all_gather is RCCL's all-gather over xGMI on the caller's
// stream: rank r's `send` lands at item range [r * send.batch(), (r + 1) * send.batch()) of `recv` on every rank.  Stands in for
// /root/reference/src/core/distributed/distributed_context.cpp:97-122 (ncclAllGather + stream create + synchronise per call).
class Communicator {
public:
    static std::vector<uint8_t> unique_id();   // 128 bytes
    Communicator(const std::vector<uint8_t>& id, int rank, int world_size, int device_id);
    ~Communicator();
    Communicator(const Communicator&) = delete;
    Communicator& operator=(const Communicator&) = delete;
    int rank() const;
    int world_size() const;
    // recv.batch() == world_size * send.batch(), same components; the domain flag is copied.  Enqueues on `stream` and returns.
    void all_gather(const PolyBuffer& send, PolyBuffer& recv, Stream* stream = nullptr) const;

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// Randomness.  Keys, encryption randomness and errors are drawn from ChaCha20 keyed by the operating system's CSPRNG
// (getrandom(2)): uniform values by rejection sampling, ternary secrets, centred-binomial errors (sigma = 3.24).
// TestSeed selects a DETERMINISTIC, NON-CRYPTOGRAPHIC generator (SplitMix64) instead - for reproducible tests, examples
// and benchmarks ONLY: anyone who knows the seed (64 bits, invertible) knows the secret key and every encryption.
struct TestSeed {
    uint64_t value;
};

// ---- N2: secret key, encryption, decryption, key generation -------------------------------
// Host-side (client-side in the reference's story, /root/reference/README.md:57-60): sampling and CRT decoding run on
// the CPU, polynomial arithmetic goes through the same C ABI as everything else.  Symmetric RLWE:
//   ct = (c0, c1) = (-(a s) + e + 2^log2_scale * m,  a),   s ternary, e centred binomial (sigma = 3.24, |e| <= 21).
// Messages are integer polynomials (N signed coefficients per item); decryption returns round(phase / 2^log2_scale),
// where phase = c0 + c1 s (+ c2 s^2) is CRT-composed over all limbs and centred mod Q = prod q_i.
class SecretKey {
public:
    explicit SecretKey(const Context& ctx);            // fresh ternary secret from the OS CSPRNG
    SecretKey(const Context& ctx, TestSeed seed);      // deterministic - tests only
    SecretKey(const Context& ctx, const std::vector<int8_t>& ternary_coefficients);  // the same secret on another context
    ~SecretKey();
    SecretKey(const SecretKey&) = delete;
    SecretKey& operator=(const SecretKey&) = delete;
    const std::vector<int8_t>& coefficients() const;  // ternary s
    const uint64_t* ntt() const;                        // device, [L][N]: NTT(s)
    const uint64_t* ntt_squared() const;                // device, [L][N]: NTT(s)^2 = NTT(s^2)

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// Public key: pk = (-(a s) + e, a), stored in the NTT domain ([1][2][L][N]).  Whoever holds it can encrypt; only the
// secret key decrypts (the reference's story keeps the secret key with the client, README.md:57-60).
class PublicKey : public PolyBuffer {
public:
    explicit PublicKey(const Context& ctx) : PolyBuffer(ctx, 1, 2, /*is_ntt=*/true) {}
};

class KeyGenerator {
public:
    explicit KeyGenerator(const Context& ctx);          // secret key and all key randomness from the OS CSPRNG
    KeyGenerator(const Context& ctx, TestSeed seed);    // deterministic - tests only
    ~KeyGenerator();
    KeyGenerator(const KeyGenerator&) = delete;
    KeyGenerator& operator=(const KeyGenerator&) = delete;
    const SecretKey& secret_key() const;
    void create_relin_keys(RelinKeys& out);  // evk_j = (-(a_j s) + e_j + g_j s^2, a_j), NTT domain
    void create_galois_keys(GaloisKeys& out);  // key_j = (-(a_j s) + e_j + g_j sigma_g(s), a_j) for out.galois_elt()
    void create_public_key(PublicKey& out);    // (-(a s) + e, a), NTT domain
    // the same with the uniform half expanded from a fresh seed drawn from this generator's randomness: a_j = expand(seed, j, ., 1)
    // (PolyBuffer::save_seeded(os, seed) then ships half of the words)
    void create_relin_keys_seeded(RelinKeys& out, Seed& seed_out);
    void create_galois_keys_seeded(GaloisKeys& out, Seed& seed_out);
    void create_public_key_seeded(PublicKey& out, Seed& seed_out);

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

class Encryptor {
public:
    Encryptor(const Context& ctx, const SecretKey& sk);   // symmetric: c1 uniform, c0 = -(c1 s) + e + scale m
    Encryptor(const Context& ctx, const SecretKey& sk, TestSeed seed);   // deterministic - tests only
    // public-key: (c0, c1) = (u pk0 + e1 + scale m, u pk1 + e2) with u ternary, e1, e2 small; decrypts under the same secret
    Encryptor(const Context& ctx, const PublicKey& pk);
    Encryptor(const Context& ctx, const PublicKey& pk, TestSeed seed);   // deterministic - tests only
    ~Encryptor();
    Encryptor(const Encryptor&) = delete;
    Encryptor& operator=(const Encryptor&) = delete;
    // messages: out.batch() * N signed coefficients; out: 2-component ciphertext(s), coefficient domain
    void encrypt(const int64_t* messages, unsigned log2_scale, Ciphertext& out);
    // exact integer arithmetic mod a plaintext modulus t (BFV-style scaling): c0 = -(a s) + e + floor(Q/t) * m
    void encrypt_exact(const int64_t* messages, uint64_t plain_modulus, Ciphertext& out);
    // Seeded symmetric encryption: one fresh seed per call (from this encryptor's randomness), c1 of item b = expand(seed, b, ., 1) expanded on the
    // device, c0 = -(c1 s) + e + scale m as above.  A public-key Encryptor throws INVALID_STATE (its c1 = u pk1 + e2 is not a PRF output).
    void encrypt_seeded(const int64_t* messages, unsigned log2_scale, Ciphertext& out, Seed& seed_out);
    void encrypt_exact_seeded(const int64_t* messages, uint64_t plain_modulus, Ciphertext& out, Seed& seed_out);

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

class Decryptor {
public:
    Decryptor(const Context& ctx, const SecretKey& sk);
    ~Decryptor();
    Decryptor(const Decryptor&) = delete;
    Decryptor& operator=(const Decryptor&) = delete;
    // ct: 2 or 3 components, coefficient domain.  messages_out: ct.batch() * N values round(phase / 2^log2_scale);
    // throws RUNTIME_ERROR if a value does not fit 62 bits (wrong scale or noise overflow).
    void decrypt(const Ciphertext& ct, unsigned log2_scale, int64_t* messages_out);
    // inverse of encrypt_exact: messages_out[k] = round(t * phase_k / Q) mod t, in [0, t)
    void decrypt_exact(const Ciphertext& ct, uint64_t plain_modulus, uint64_t* messages_out);
    // Remaining noise budget of encrypt_exact-style ciphertexts in bits (the smallest over all items and coefficients):
    // log2(Q / 2) - log2 |t * phase - Q * round(t * phase / Q)|, exact big-integer arithmetic.  Decryption is correct while it is > 0;
    // a fresh ciphertext at N = 8192 with five 60-bit limbs and t = 65537 has ~ 270 bits.  Host-side (whoever holds the secret key).
    double noise_budget_bits(const Ciphertext& ct, uint64_t plain_modulus);
    // the same from compact form, exact on the host: K = max(bits), phase = c0 2^(K - bits0) + (c1 * s) 2^(K - bits1) mod 2^K (negacyclic product in
    // wrapping 64-bit arithmetic), m = round(t phase / 2^K) mod t; the budget is the expression above with 2^K in place of Q.
    void decrypt_exact(const CompactCiphertext& ct, uint64_t plain_modulus, uint64_t* messages_out);
    double noise_budget_bits(const CompactCiphertext& ct, uint64_t plain_modulus);

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// Re-randomised results (include/dpfhe.h dpfhe_rerandomize): before a result leaves the server, add a fresh public-key
// encryption of zero  (u pk0 + e0, u pk1 + e1)  whose c0 error e0 is uniform on [-2^flood_bits, 2^flood_bits): it drowns the noise the circuit left,
// which is a function of the server's weights and the client - who holds the secret key - could otherwise read.  Order: evaluate -> rerandomize ->
// Evaluator::compact.  The noise comes from ChaCha20 on the device under a SECRET 32-byte seed drawn fresh for every call (OS CSPRNG) and never stored.
// What is claimed is the usual flooding argument against a client that follows the protocol, given a correct PUBLIC noise bound; nothing is claimed
// against malformed input ciphertexts, and timing and sizes still show the circuit's shape.
class Rerandomizer {
public:
    // pk: the client's public key on ctx (KeyGenerator::create_public_key); ctx and pk must outlive the object
    Rerandomizer(const Context& ctx, const PublicKey& pk);
    Rerandomizer(const Context& ctx, const PublicKey& pk, TestSeed seed);   // deterministic seeds - tests only
    ~Rerandomizer();
    Rerandomizer(const Rerandomizer&) = delete;
    Rerandomizer& operator=(const Rerandomizer&) = delete;
    // in place on ct (2 components, coefficient domain, encrypt_exact-style with plaintext modulus t); enqueues on `stream`.  The work buffer belongs to
    // the object: grown when a larger batch arrives, never shrunk, so steady-state calls allocate nothing (one rerandomize() at a time per object).
    // INVALID_ARGUMENT for a 3-component or NTT-domain ciphertext, a ciphertext of another context, or flood_bits outside [1, max_flood_bits(t)].
    void rerandomize(Ciphertext& ct, uint64_t plain_modulus, unsigned flood_bits, Stream* stream = nullptr);
    // floor(log2 Q) - ceil(log2 t) - 4 (at most 250): beyond it less than about two bits of budget would remain, which is what compact needs
    unsigned max_flood_bits(uint64_t plain_modulus) const;
    // ceil(noise_bits) + lambda + log2_n: a shift by |v_old| <= 2^B moves a uniform value on [-2^f, 2^f) by statistical distance 2^(B - f - 1) per
    // coefficient; over N coefficients that is at most 2^-lambda.  noise_bits is the caller's PUBLIC bound B for the circuit (log2 Q - 1 - log2 t minus
    // the budget its noise model guarantees): the library does not and cannot measure noise on the server.
    static unsigned flood_bits_for(double noise_bits, unsigned log2_n, unsigned lambda = 40);

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// ScalarWeights: the integer weights of HybridKeySwitcher::multiply_lincomb_rescale_range as residue rows on the device ([K + 2][Ld], the d_w of
// dpfhe_relinearize_lincomb_rescale_hybrid), built once: row 0 the product's weight, rows 1 .. K the terms', row K + 1 the constant
// constant_at_output * q_last - an exact integer product, as ApproxPolynomial builds its own, so that the rescale gives constant_at_output back exactly in
// every slot's coefficient 0 (a constant at the OUTPUT's scale).  INVALID_ARGUMENT for more than 15 terms or a |w| >= 2^62; INVALID_STATE for a data_ctx of
// one limb (nothing to drop).  data_ctx must outlive the object.
class ScalarWeights {
public:
    ScalarWeights(const Context& data_ctx, int64_t product_weight, const std::vector<int64_t>& term_weights, int64_t constant_at_output);
    ~ScalarWeights();
    ScalarWeights(const ScalarWeights&) = delete;
    ScalarWeights& operator=(const ScalarWeights&) = delete;
    size_t terms() const;                 // K
    const Context& context() const;       // data_ctx
    const uint64_t* data() const;         // device, [K + 2][Ld]

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// ComplementConstant: the constant kappa of HybridKeySwitcher::multiply_complement_rescale_range as residues on the device ([Ld], word l = kappa mod q_l: the
// d_kappa of dpfhe_ct_mul_complement), uploaded once at construction.  kappa is the integer the factor kappa X^0 - b complements b to: at b's scale sigma
// the encoding of the constant kappa / sigma in every slot (Goldschmidt's 2 is kappa = llround(2 sigma)).  INVALID_ARGUMENT for kappa < 0 or kappa >= 2^62.
// data_ctx must outlive the object.
class ComplementConstant {
public:
    ComplementConstant(const Context& data_ctx, int64_t kappa);
    ~ComplementConstant();
    ComplementConstant(const ComplementConstant&) = delete;
    ComplementConstant& operator=(const ComplementConstant&) = delete;
    int64_t value() const;                // kappa
    const Context& context() const;       // data_ctx
    const uint64_t* data() const;         // device, [Ld]

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// one addend of multiply_lincomb_rescale_range: items first .. first + count - 1 of ct
struct LincombTerm {
    const Ciphertext* ct;
    size_t first;
};

// Hybrid key switching with one special prime P (SURVEY.md 8f N1 "base extension"): keys live on the extended
// context (data moduli + P) and the switching noise drops from ~ L N q sigma to ~ L N q sigma / P.
class HybridKeySwitcher {
public:
    // data_ctx: the level the ciphertexts live on; (special_prime, special_psi): one more NTT prime and its 2N-th root
    HybridKeySwitcher(const Context& data_ctx, const SecretKey& sk, uint64_t special_prime, uint64_t special_psi);
    HybridKeySwitcher(const Context& data_ctx, const SecretKey& sk, uint64_t special_prime, uint64_t special_psi, TestSeed seed);   // tests only
    ~HybridKeySwitcher();
    HybridKeySwitcher(const HybridKeySwitcher&) = delete;
    HybridKeySwitcher& operator=(const HybridKeySwitcher&) = delete;
    void add_galois_element(uint32_t galois_elt);  // generates and keeps the key for sigma_g
    // the key of an added element: [Ld][2][L][N] on extended_context(), NTT domain - what the C ABI's rotations take (INVALID_STATE: never added)
    const PolyBuffer& galois_key(uint32_t galois_elt) const;
    // The `stream` argument: relinearize and apply_galois allocate their temporaries per call and SYNCHRONISE `stream` before they
    // return.  Every other method below enqueues on `stream` and returns without host synchronisation once its scratch has its size and the keys of its
    // element list are packed: the FIRST call with a new element list packs the keys on `stream` and synchronises it, and a larger batch than ever
    // before reallocates the scratch.
    // 3 -> 2 components, coefficient domain, on data_ctx
    void relinearize(const Ciphertext& in3, Ciphertext& out2, Stream* stream = nullptr) const;
    // ciphertext of m(X) -> ciphertext of m(X^g); the element must have been added
    void apply_galois(const Ciphertext& in2, uint32_t galois_elt, Ciphertext& out2, Stream* stream = nullptr) const;
    // The approximate family's ciphertext x ciphertext step: out = round(relinearize(a * b) / q_last) at the next level - Evaluator::multiply on data_ctx,
    // then dpfhe_relinearize_rescale_hybrid (the division by P and by the last data prime in one pass; the words of relinearize + Evaluator::rescale).
    // a, b: 2 components, coefficient domain, one batch, on data_ctx (they may be the same object: a square); out_next_level: 2 components, same batch, on a
    // Context of data_ctx.params().drop_last_limb().  At scales s_a, s_b the result has scale s_a s_b / q_last.  Enqueues only: the product and the Q P
    // sums live in scratch the object owns, grown only for a larger batch than ever before.  INVALID_STATE when data_ctx has one limb.
    void multiply_rescale(const Ciphertext& a, const Ciphertext& b, Ciphertext& out_next_level, Stream* stream = nullptr) const;
    // the same on item ranges: out item out_first + i = items a_first + i of a times b_first + i of b, i < count (a and b may be one buffer, also one range)
    void multiply_rescale_range(const Ciphertext& a, size_t a_first, const Ciphertext& b, size_t b_first, size_t count, Ciphertext& out_next_level,
                                size_t out_first, Stream* stream = nullptr) const;
    // A product, a scalar linear combination and the rescale in one step (the second half of a Newton step, a Horner step): out item out_first + i =
    //   round((w_0 relinearize(a_i * b_i) + sum_k w_{1+k} z_k,i + constant) / q_last)   at the next level
    // - Evaluator::multiply on data_ctx into the object's scratch, then dpfhe_relinearize_lincomb_rescale_hybrid: the relinearised product is never written,
    // and term k = items terms[k].first + i of *terms[k].ct is read in place on ITS context, whose first limbs must be data_ctx's (the same level, or any level
    // above it on the same prime chain: keeping the first limbs is the level drop; no copy).  The scales are the caller's: the phases summed are
    // w_0 s_a s_b (a b) and w_{1+k} s_k z_k, and the sum is divided by q_last (ApproxInvSqrt shows one choice).  weights: on data_ctx, weights.terms() == terms.size().
    // Terms: 2 components, coefficient domain.  The stream contract is multiply_rescale_range's: enqueues only, scratch grown only for a larger batch.
    void multiply_lincomb_rescale_range(const Ciphertext& a, size_t a_first, const Ciphertext& b, size_t b_first, size_t count, const ScalarWeights& weights,
                                        const std::vector<LincombTerm>& terms, Ciphertext& out_next_level, size_t out_first, Stream* stream = nullptr) const;
    // A SUM of products under one key switch and one rounding (attention's sum_j p_ij v_j, an inner product over several ciphertexts): out item out_first + g =
    //   round(relinearize(sum_{k < terms} a_{g,k} * b_{g,k}) / q_last)   at the next level,   g < groups,
    // a_{g,k} = item a_first + g * terms + k of a; b_{g,k} = item b_first + g * terms + k of b or, with b_shared, item b_first + k for every group.  The tensor
    // products are summed by dpfhe_ct_mul_sum into the object's scratch (3 components per GROUP), then dpfhe_relinearize_rescale_hybrid runs over `groups`
    // items: `terms` times fewer key products, inverse transforms and roundings than `terms` multiply_rescale_range calls and their additions - and NOT their
    // words (one rounding instead of `terms`).  Word for word Evaluator::multiply per pair, Evaluator::add over the pairs, relinearize, Evaluator::rescale.  All
    // pairs of a group must share one scale product s_a s_b; the result has scale s_a s_b / q_last.  a and b may be one buffer (a sum of squares when the ranges
    // coincide).  The stream contract is multiply_rescale_range's.  INVALID_ARGUMENT for terms == 0.
    void multiply_sum_rescale_range(const Ciphertext& a, size_t a_first, const Ciphertext& b, size_t b_first, bool b_shared, size_t groups, size_t terms,
                                    Ciphertext& out_next_level, size_t out_first, Stream* stream = nullptr) const;
    // ... and with multiply_lincomb_rescale_range's second half (the giant-step sum of a Paterson-Stockmeyer evaluation plus scalar terms plus a constant):
    //   round((w_0 relinearize(sum_k a_{g,k} * b_{g,k}) + sum_j w_{1+j} z_j,g + constant) / q_last);   addend j = items addends[j].first + g of *addends[j].ct.
    void multiply_sum_lincomb_rescale_range(const Ciphertext& a, size_t a_first, const Ciphertext& b, size_t b_first, bool b_shared, size_t groups, size_t terms,
                                            const ScalarWeights& weights, const std::vector<LincombTerm>& addends, Ciphertext& out_next_level, size_t out_first,
                                            Stream* stream = nullptr) const;
    // Products that share a COMPLEMENT factor, at the next level (one Goldschmidt division step n_j <- n_j F, D <- D F with F = 2 - D): with
    // F_g = kappa X^0 - b_g, b_g = item b_first + g of b, and a_{g,k} = item a_first + g * terms + k of a,
    //   out item out_first + g * terms + k      = round(relinearize(a_{g,k} * F_g) / q_last),   g < groups, k < terms,
    //   out item out_first + groups * terms + g = round(relinearize(b_g * F_g) / q_last)        when with_self:
    // the numerators group-major, then the denominators - the next step's two item ranges.  dpfhe_ct_mul_complement writes the groups * terms (+ groups) tensor
    // products into the object's scratch - F is never written and never transformed - then dpfhe_relinearize_rescale_hybrid runs over all of them.  Word for
    // word Evaluator::negate on b_g, Evaluator::add_plain of the constant polynomial kappa X^0, and multiply_rescale_range against that factor copied out per
    // item.  At scales s_a of a and sigma of b, with kappa = llround(c sigma), the results have scales s_a sigma / q_last and sigma^2 / q_last and hold
    // a (c - b) and b (c - b).  a and b may be one buffer; terms may be 0 with with_self (the denominators alone).  kappa: on data_ctx.  The stream contract is
    // multiply_rescale_range's.  INVALID_ARGUMENT for terms == 0 without with_self, ranges outside their buffers, a kappa of another context.
    void multiply_complement_rescale_range(const Ciphertext& a, size_t a_first, const Ciphertext& b, size_t b_first, size_t groups, size_t terms, bool with_self,
                                           const ComplementConstant& kappa, Ciphertext& out_next_level, size_t out_first, Stream* stream = nullptr) const;
    // ALL PAIRS of two item ranges at the next level (attention's scores before their slot sum: every query against every key): with a_i = item a_first + i of
    // a (i < a_count) and b_j = item b_first + j of b (j < b_count),
    //   out item out_first + i * b_count + j     = round(relinearize(a_i * b_j) / q_last)                       (every pair), or, with `causal` (a_count == b_count),
    //   out item out_first + i (i + 1) / 2 + j   = the same for j <= i only                                      (a_count (a_count + 1) / 2 items).
    // dpfhe_ct_mul_outer writes the tensor products into the object's scratch - every operand transformed once, a tile of queries kept in registers while the
    // keys stream past - then dpfhe_relinearize_rescale_hybrid runs over all pairs.  Word for word multiply_rescale_range on the two pair lists copied out item
    // by item.  At scales s_a, s_b every result has scale s_a s_b / q_last.  a and b may be one buffer, also one range.  The stream contract is
    // multiply_rescale_range's.  INVALID_ARGUMENT for causal with a_count != b_count and for ranges outside their buffers; a count of 0 is a no-op.
    void multiply_outer_rescale_range(const Ciphertext& a, size_t a_first, size_t a_count, const Ciphertext& b, size_t b_first, size_t b_count, bool causal,
                                      Ciphertext& out_next_level, size_t out_first, Stream* stream = nullptr) const;
    // many rotations in one pass (dpfhe_rotate_hybrid_batch): out item out_first + i = sigma_{elts[i]} of in item i, or of THE
    // item of `in` when it holds one.  All elements must have been added; the keys of a given element list are packed
    // back to back once and cached.
    void apply_galois_many(const Ciphertext& in2, const std::vector<uint32_t>& galois_elts, Ciphertext& out2, size_t out_first = 0,
                           Stream* stream = nullptr) const;
    // same on item ranges: out item out_first + i = sigma_{elts[i]} of in item in_first + i (or of in item in_first when `broadcast`).
    // `in2` and `out2` may be the same buffer as long as the two ranges do not overlap.
    void apply_galois_range(const Ciphertext& in2, size_t in_first, bool broadcast, const std::vector<uint32_t>& galois_elts, Ciphertext& out2,
                            size_t out_first, Stream* stream = nullptr) const;

    // HOISTED: many rotations of ONE item (in2 item in_item): the digit decomposition of c1 and its forward transforms are done
    // once, each rotation is a permutation in the NTT domain + its key inner product (dpfhe_rotate_hybrid_hoisted).  A valid key
    // switch of sigma_g(ct), not word-identical to apply_galois_many (the automorphism acts after the lift, not before it).
    // n_items inputs (in2 items in_first ...) share the rotations; the output is ROTATION-MAJOR: item out_first + r * n_items + t.
    void apply_galois_hoisted(const Ciphertext& in2, size_t in_first, size_t n_items, const std::vector<uint32_t>& galois_elts, Ciphertext& out2,
                              size_t out_first, Stream* stream = nullptr) const;
    // k * group items, item i rotated by galois_elts[i / group] (the giant steps of `group` tokens; keys read once per element)
    void apply_galois_grouped(const Ciphertext& in2, size_t in_first, const std::vector<uint32_t>& galois_elts, size_t group, Ciphertext& out2,
                              size_t out_first, Stream* stream = nullptr) const;

    // The rotate-and-add ladder (dpfhe_rotate_add_hybrid): out item out_first + i = acc_k of in item in_first + i, i < count, where acc_0 is the item and
    // acc_{e+1} = acc_e + sigma_{elts[e]}(acc_e) - the words of apply_galois_grouped with that one element followed by Evaluator::add, step by step, in three
    // launches per step instead of four.  All elements must have been added; `in2` and `out2` may be the same buffer as long as the two ranges do not overlap.
    // Enqueues only after the first call with a given element list; the scratch (the Q P products, the ladder's second accumulator) is the object's own.
    void rotate_add_range(const Ciphertext& in2, size_t in_first, size_t count, const std::vector<uint32_t>& galois_elts, Ciphertext& out2, size_t out_first,
                          Stream* stream = nullptr) const;

    // ---- division by P deferred ("double hoisting"; include/dpfhe.h "N3, round 3") -------------------------------------
    // The context of the data moduli + the special prime: buffers holding terms over Q P live on it.
    const Context& extended_context() const;
    const Context& data_context() const;   // the level the ciphertexts live on (the constructor's data_ctx)
    // n_items inputs (in2 items in_first ...) -> out_qp items out_first + r * n_items + t, r = 0 .. elts.size(): r = 0 is P * ct_t, r >= 1 is
    // P * sigma_{elts[r-1]}(ct_t) + its key-switching term; NTT domain over Q P, NOT divided by P (dpfhe_rotate_hoisted_qp).
    // `out_qp`: 2-component buffer on extended_context().
    void rotate_hoisted_qp(const Ciphertext& in2, size_t in_first, size_t n_items, const std::vector<uint32_t>& galois_elts, PolyBuffer& out_qp,
                           size_t out_first, Stream* stream = nullptr) const;
    // elts.size() * group items (in2 items in_first ...), item i with the key of elts[i / group]: out_qp item out_first + i = the key
    // inner product of item i's c1 alone, NTT domain over Q P (dpfhe_switch_key_qp); the caller sums such terms, transforms back
    // once and finishes with dpfhe_rescale_bsgs.  The items must already carry the automorphism (coefficient domain).
    void switch_key_qp(const Ciphertext& in2, size_t in_first, const std::vector<uint32_t>& galois_elts, size_t group, PolyBuffer& out_qp,
                       size_t out_first, Stream* stream = nullptr) const;
    // One HybridKeySwitcher serves ONE stream at a time: its scratch buffers and its cache of packed keys are shared by every call
    // (and by every PackedLinear built on it); calls on different streams must be ordered by the caller.

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// ---- N3: slot packing and the packed matrix-vector product ------------------------------------
// BatchEncoder: N slots of Z_t (t prime, t = 1 mod 2N) arranged as 2 rows x N/2.  Slot i of row 0 is the value of the
// message polynomial at zeta^(3^i), row 1 at zeta^(-3^i) (zeta a primitive 2N-th root mod t), so the automorphism
// X -> X^(3^s) rotates both rows LEFT by s slots and X -> X^(2N-1) swaps the rows.  Host-side (client-side) code.
class BatchEncoder {
public:
    explicit BatchEncoder(const Context& ctx, uint64_t plain_modulus = 65537);
    ~BatchEncoder();
    BatchEncoder(const BatchEncoder&) = delete;
    BatchEncoder& operator=(const BatchEncoder&) = delete;
    uint64_t plain_modulus() const;
    size_t slot_count() const;   // N
    size_t row_size() const;     // N / 2
    void encode(const uint64_t* slots /* N values < t: row 0 then row 1 */, int64_t* coeffs_out /* N, centred mod t */) const;
    void decode(const uint64_t* coeffs_mod_t /* N */, uint64_t* slots_out /* N */) const;
    uint32_t galois_element(int left_rotation) const;   // 3^s mod 2N (negative s rotates right)
    uint64_t root() const;                              // zeta (include/dpfhe.h dpfhe_encoder_root gives the same number)
    // Encoding ON THE DEVICE (include/dpfhe.h dpfhe_encode_slots): `items` slot vectors of N 32-bit values < t -> the `items` polynomials of `out`, the
    // words encode() + a lift to every limb + an upload would give (to_ntt: transformed as well; out's domain flag is set either way).  `out` may belong to
    // the encoder's context or to ANY context of the same ring degree on the same device (the extended Q P context of a key switcher): the encoder keeps
    // one set of device tables per context it has encoded for.  `slots` is a device pointer (16-byte aligned: the call only enqueues on `stream`, no
    // allocation, no synchronisation - a request-time operand never visits the host) or a host pointer (staged through a temporary device buffer; the
    // call then synchronises `stream`).  Thread-safe.
    void encode_device(const uint32_t* slots, size_t items, Plaintext& out, bool to_ntt = false, Stream* stream = nullptr) const;
    // the building block of the above and of ExactPlaintext::set_slots_device: d_out on ctx's device, flags as for dpfhe_encode_slots; the same rule for
    // `stream` (device pointer: enqueue only; host pointer: synchronises `stream`)
    void encode_device_words(const Context& ctx, const uint32_t* slots, size_t items, uint64_t* d_out, uint32_t flags, Stream* stream = nullptr) const;

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// ComplexEncoder: N/2 complex (or real) slots of the approximate (CKKS-style) family (include/dpfhe.h "complex slot encoding").  Slot i is the value of
// the real message polynomial m at xi^(3^i), xi = exp(i pi / N), and conj(z_i) its value at xi^(-3^i); the encoding is round(scale m).  X -> X^(3^s)
// rotates the slots LEFT by s (cyclically over N/2), X -> X^(2N-1) conjugates them.  The scale is the caller's to track: a product of encodings at
// scales a and b is an encoding at a b, and rescale divides it by the dropped prime.
class ComplexEncoder {
public:
    explicit ComplexEncoder(const Context& ctx);
    ~ComplexEncoder();
    ComplexEncoder(const ComplexEncoder&) = delete;
    ComplexEncoder& operator=(const ComplexEncoder&) = delete;
    size_t slot_count() const;                        // N / 2
    uint32_t galois_element(int steps) const;         // 3^steps mod 2N (negative steps rotate right)
    uint32_t conjugation_element() const;             // 2N - 1
    // host (client) side: N/2 slots -> the N centred coefficients Encryptor::encrypt(coeffs, 0, ct) takes, and back from what Decryptor::decrypt(ct, 0, out)
    // returns; the accuracy bounds are the header's E and D
    void encode(const std::complex<double>* slots, double scale, int64_t* coeffs) const;
    void decode(const int64_t* coeffs, double scale, std::complex<double>* slots) const;
    // Encoding ON THE DEVICE (include/dpfhe.h dpfhe_encode_complex): `items` vectors of N/2 (re, im) pairs, or of N/2 doubles when `real`, -> the `items`
    // polynomials of `out`, word for word what encode() + a lift to every limb + an upload would give (to_ntt: transformed as well; out's domain flag is
    // set either way).  `out` may belong to ANY context of the encoder's ring degree on the same device.  `d_slots` is a DEVICE pointer, 16-byte aligned:
    // the call only enqueues on `stream`, no allocation, no synchronisation.  Thread-safe.
    void encode_device(const double* d_slots, size_t items, double scale, Plaintext& out, bool to_ntt = false, bool real = false, Stream* stream = nullptr) const;
    // the building block of the above: d_out on ctx's device, flags as for dpfhe_encode_complex
    void encode_device_words(const Context& ctx, const double* d_slots, size_t items, double scale, uint64_t* d_out, uint32_t flags, Stream* stream = nullptr) const;

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// SlotSum: sums across the slots of one ciphertext - what LayerNorm's mean and variance, a softmax's denominator and an inner product of two encrypted
// vectors need.  After apply(), slot i holds  sum_{j < block} x[(i + j stride) mod N/2]  (within each of BatchEncoder's two rows, over the one row of a
// ComplexEncoder): log2(block) rotate-and-add steps by 3^(stride 2^e), e < log2(block), as ONE HybridKeySwitcher::rotate_add_range.  On an input of period
// block * stride - what pack_input of the packed layers produces - every slot therefore holds the total of its residue class modulo stride.  Independent of
// the family: both encoders rotate by 3^s.  Exact over Z_t (sums mod t); the approximate family's error:
//
// Error bound.  ApproxPackedLinear's notation and tools T1 - T4: Ld the data limbs, rho = max_j q_j / P, K = 21 Ld N rho (T4), H = (N + 1) / 2 (T3),
//   u8 = 8 log2(N) 2^-53, D = the input's scale, X = max|x_i|, Bin the infinity norm of the input phase's error in coefficients.  A step adds the running sum
//   to its rotation: the automorphism keeps the coefficient norm (T2), its key switch adds K and the division by P's rounding H, so an error e becomes
//   e + (e + K + H) = 2 e + K + H.  After the log2(block) steps:  block Bin + (block - 1) (K + H)  per coefficient, N times that per slot (T1), in units of the
//   values:  pre = N (block Bin + (block - 1) (K + H)) / D.  The scale does not change.  Every slot is at most block X + pre in modulus, so the decrypted
//   coefficients obey max|c_k| <= D (block X + pre) and the client's decode adds u8 N (block X + pre).
//   error_bound(D, X, Bin) = pre + u8 N (block X + pre): a bound on |decoded slot - the sum| for every slot and token, provided the phase does not wrap.
//   (Worst case throughout, like the layers' bounds: key-switch errors add like a random walk, not in absolute value.)
class SlotSum {
public:
    // block, stride: powers of two, block >= 2, block * stride <= N/2 (INVALID_ARGUMENT otherwise).  Adds the elements 3^(stride 2^e) mod 2N, e < log2(block),
    // to `ks` in ascending order of e; `ks` must outlive the object.
    SlotSum(HybridKeySwitcher& ks, size_t block, size_t stride = 1);
    ~SlotSum();
    SlotSum(const SlotSum&) = delete;
    SlotSum& operator=(const SlotSum&) = delete;
    size_t block() const;
    size_t stride() const;
    size_t steps() const;                                    // log2(block): key switches per item
    const std::vector<uint32_t>& galois_elements() const;    // the ladder's elements, in the order they are applied
    // the bound derived above (the approximate family): scale = D, max_abs_input = X, input_noise_bound = Bin
    double error_bound(double scale, double max_abs_input, double input_noise_bound) const;
    // ... and without a device: data_moduli are the limbs of ks.data_context(), special_prime its P
    static double error_bound(uint32_t log2_n, const std::vector<uint64_t>& data_moduli, uint64_t special_prime, size_t block, double scale, double max_abs_input,
                              double input_noise_bound);
    // x: T items on ks.data_context() (2 components, coefficient domain); y: T items on the same context, another buffer.  Level and scale do not change.
    // The stream contract of HybridKeySwitcher::rotate_add_range: enqueues only after the first call; one apply() at a time per key switcher.
    void apply(const Ciphertext& x, Ciphertext& y, Stream* stream = nullptr) const;

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// PackedLinear: encrypted y = W x over Z_t for an out_dim x in_dim matrix in slot packing - the encrypted replacement of the
// dense layers at the reference's matmul sites for a single token (/root/reference/src/core/execution/models/gpt_model.cpp:793
// QKV 768 -> 2304, :848 FFN 768 -> 3072 -> 768, :883 LM head 768 -> 50257; dims /root/reference/src/core/execution/model.hpp:47-50).
//
// Input packing: the vector repeats with period n = 2^ceil(log2 in_dim) along both slot rows (pack_input), so a ciphertext
// holds N / n identical windows.  Diagonal method with baby-step / giant-step rotations over m diagonals:
//   sum_i rot_{i n1}( sum_j rot_{-i n1}(diag_{i n1 + j}) (.) rot_j(x) ),   n1 n2 = m,
//   * out_dim >= n  (m = n): every window computes a DIFFERENT block of n output rows, so one ciphertext delivers N outputs and
//     ceil(out_dim / N) output ciphertexts share the n1 - 1 baby-step rotations; each costs n2 - 1 giant-step rotations;
//   * out_dim <  n  (m = 2^ceil(log2 out_dim)): only the m wrapped diagonals diag_k[r] = W[r mod m][(r + k) mod n] are used and the
//     n / m partial sums are folded with log2(n / m) more rotations; the result repeats with period m (it is a valid input
//     of the next layer);
//   * one block (out_dim <= m = n): every window computes the same block, the result repeats with period n.
// Per application (round 3: the division by P is deferred - "double hoisting"): ONE hoisted rotation pass for the baby steps whose
// results stay in the NTT domain over Q P (dpfhe_rotate_hoisted_qp: gathers + key inner products, no transform), ONE
// dpfhe_matvec_plain_multi over all pre-transformed diagonals (encoded over Q P) of all output ciphertexts, one inverse transform
// that applies the giant-step automorphisms as it loads (dpfhe_ntt_inv_galois) + one divide-by-P pass over the inner sums, then per
// output ciphertext the giant steps' key inner products (dpfhe_switch_key_qp: Ld transforms each instead of Ld + 2), their sum,
// ONE inverse transform and ONE divide-by-P + add (dpfhe_rescale_bsgs).
class PackedLinear {
public:
    // W: out_dim * in_dim values < t, row-major.  The needed Galois keys are added to `ks`.
    // tokens_per_ciphertext = 2 (round 6): the two slot ROWS of a ciphertext carry two different tokens - row 0 repeats token A's vector with period n, row 1
    // token B's.  Every rotation of the diagonal method is a row rotation and the diagonals are the same for both rows, so the layer computes W x_A in row 0 and
    // W x_B in row 1 with the very same kernels: half the cost per token.  It needs the layer's output blocks to fit the windows of ONE row
    // (ceil(out_dim / n) <= N / (2 n) for one output ciphertext: GPT-2 small's layers do at N = 8192 and N = 16384); pack_input_rows / unpack_output_rows.
    PackedLinear(const Context& data_ctx, const BatchEncoder& enc, HybridKeySwitcher& ks, const uint64_t* W, size_t out_dim, size_t in_dim, size_t tokens_per_ciphertext = 1);
    // square d x d (d a power of two dividing N/2)
    PackedLinear(const Context& data_ctx, const BatchEncoder& enc, HybridKeySwitcher& ks, const uint64_t* W, size_t d);
    // y = W x + bias: `bias` holds out_dim values < t (null: exactly the constructor above).  Every slot that holds output row R gets bias[R] (0 where no
    // row is), encoded once per output ciphertext and kept on the device; apply() ends with one exact plaintext addition on its stream.
    PackedLinear(const Context& data_ctx, const BatchEncoder& enc, HybridKeySwitcher& ks, const uint64_t* W, size_t out_dim, size_t in_dim,
                 size_t tokens_per_ciphertext, const uint64_t* bias);
    bool has_bias() const;
    double encode_seconds() const;   // wall time the constructor spent building and encoding the diagonals and the bias (the rest of it generates keys)
    ~PackedLinear();
    PackedLinear(const PackedLinear&) = delete;
    PackedLinear& operator=(const PackedLinear&) = delete;
    size_t dim() const;                 // m: diagonals per output ciphertext
    size_t in_dim() const;
    size_t out_dim() const;
    size_t input_period() const;        // n
    size_t output_ciphertexts() const;  // batch of y
    size_t baby_steps() const;
    size_t giant_steps() const;
    size_t key_switches_per_apply() const;
    // slot vectors (N values each) <-> plain vectors: x (in_dim values) -> the N slots to encode and encrypt;
    // output_ciphertexts() * N decoded slots -> y (out_dim values)
    void pack_input(const uint64_t* x, uint64_t* slots) const;
    void unpack_output(const uint64_t* slots, uint64_t* y) const;
    size_t tokens_per_ciphertext() const;
    // two tokens per ciphertext: x0 -> slot row 0, x1 -> slot row 1 (each repeated with the input period); and back from output_ciphertexts() * N slots
    void pack_input_rows(const uint64_t* x0, const uint64_t* x1, uint64_t* slots) const;
    void unpack_output_rows(const uint64_t* slots, uint64_t* y0, uint64_t* y1) const;
    // x: T items (T tokens, each packed with pack_input), y: output_ciphertexts() * T items, output ciphertext o of token t at item
    // o * T + t; 2 components, coefficient domain.  All tokens share ONE pass over the rotation keys and the diagonals (hoisted
    // baby steps per token, one multi-right-hand-side matvec, the giant steps' key inner products summed before ONE division by P).
    // Enqueues on `stream` and returns (no host synchronisation).  Scratch: the layer's own buffers (they grow only when a larger T
    // than ever before arrives) AND the key switcher's (digit images, packed keys) - so one apply() at a time per LAYER, and all layers
    // built on one HybridKeySwitcher share ONE stream at a time; synchronise before reading y on the host.
    void apply(const Ciphertext& x, Ciphertext& y, Stream* stream = nullptr) const;

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// ApproxPackedLinear: encrypted y = W x + b for REAL weights in the approximate (CKKS-style) family - PackedLinear's geometry (n, m, blocks, passes,
// replication, n1 / n2, fold rotations, pre-rotated diagonals) laid on the ONE row of N/2 complex slots of a ComplexEncoder, where PackedLinear has two
// rows over Z_t: copies = (N/2) / n.  The pipeline is PackedLinear's, kernel for kernel (it does not depend on the plaintext space); the diagonals are
// real slot vectors encoded at weight_scale, the input arrives at input_scale, and apply() ends with the family's fixed-point truncation: one rescale by
// q_last to next_ctx, then - with a bias - one plaintext addition (dpfhe_add_plain) of the bias encoded at output_scale().  3^s is the rotation by s of
// both encoders, so an exact and an approximate layer on one HybridKeySwitcher share keys.
//
// Error bound.  Notation: Dx = input_scale, Dw = weight_scale, Do = output_scale() = Dx Dw / q_last; Ld the data limbs, P the special prime,
//   rho = max_j q_j / P; u8 = 8 log2(N) 2^-53 (the E and D of include/dpfhe.h); w1 = max_R ||W_R||_1; X = max|x_i|, B = max|b_R| (both times sqrt 2 with
//   two tokens per ciphertext: a slot is x_A + i x_B); Bin = the infinity norm of the input phase's error in coefficients (21 + 1/2 + E_x for a fresh
//   symmetric ciphertext of an encoding at Dx: fhe_sampler.h gives |e| <= 21, E_x = u8 Dx X).
//   Tools.  (T1) an integer polynomial with |e_k| <= b has every slot <= N b in modulus.  (T2) slots multiply slot-wise and an automorphism permutes
//   slots and keeps the coefficient norm.  (T3) a division of both components by a prime with rounding adds r0 + r1 s, |r0|, |r1| <= 1/2, s ternary:
//   at most H = (N + 1) / 2 per coefficient.  (T4) a key switch with digits in [0, q_j) and key errors |e| <= 21 adds, over Q P, at most
//   21 Ld N max_j q_j per coefficient: K = 21 Ld N rho after the division by P (whose rounding is counted by T3).
//   The products.  A diagonal's encoding has slot Dw w + eps, |eps| <= G = N (1/2 + u8 Dw max|W|) (E at weight_scale, T1).  A baby step, divided by P,
//   has slot Dx x + delta, |delta| <= S = N Bin + N K (the input's own error; the baby-step key switch, T4 + T1).  An output slot of row R sums the n
//   (diagonal, window) pairs whose weights are the row's entries - m diagonals, then n / m windows folded -, so, at scale Dx Dw, it is off
//   Dx Dw (W x)_R by at most   Dw ||W_R||_1 S + Dx X n G + n G S.   The first term holds the dominant one, ||W_R||_1 21 Ld N^2 rho / Dx after scaling.
//   The additive terms, in coefficients at scale Dx Dw: the n2 inner sums' division by P, n2 H; with giant steps (n2 > 1) their n2 - 1 key switches and
//   rescale_bsgs's rounding, (n2 - 1) K + H: together e0.  A fold step adds the running sum to its rotation, 2 e + K + H: after the log2(n / m) steps
//   eF = (n / m) e0 + (n / m - 1) (K + H).  In slots (T1): N eF.
//   After the rescale by q_last everything above is divided by Dx Dw in units of the output; its rounding adds N H / Do (T3, T1), the bias's encoding
//   N (1/2 + u8 Do B) / Do.  Their sum is `pre`, and it bounds every slot (a slot that holds no row has ||W_R||_1 = 0), so the decrypted coefficients
//   obey max|c_k| <= max slot <= Do (w1 X + B + pre) and the client's decode adds D = u8 N (w1 X + B + pre).
//   error_bound(X, Bin) = pre + D with w1 for ||W_R||_1: a bound on |decoded output row R - (W x + b)_R| for every row, token and output slot of the row.
//   (Worst case throughout: the measured error sits orders of magnitude below it - key-switch errors add like a random walk, not in absolute value.)
//
// Exact on a transparent input.  On a ciphertext with c1 = 0 every key-switch digit is zero, so every key inner product is zero and every division by P
//   divides P (...) exactly: with c0 the residues of an integer polynomial mu, sigma_g a(X) = a(X^g) in Z[X] / (X^N + 1), p[o][i][j] the encoding of
//   pre-rotated diagonal i n1 + j of output ciphertext o at weight_scale and bias_o the bias's at output_scale(), apply() gives c1_o = 0 and
//     S_i = sum_{j < n1} p[o][i][j] sigma_{3^j}(mu),   M_o = sum_{i < n2} sigma_{3^(i n1)}(S_i),   M_o += sigma_{3^s}(M_o) for s = m, 2m, ... < n,
//     c0_o = round(M_o / q_last) + bias_o  mod q_l, l < L - 1,
//   word for word (tests/approx_layer_model.py states it on Python integers, tests/test_gpu_approx_layer_words.py holds the device to it).
class ApproxPackedLinear {
public:
    // W: out_dim * in_dim finite doubles, row-major, weight_scale * max|W| < 2^62 (the encoder's clamp); bias: out_dim doubles or null (null: the words of
    // a layer built without one).  next_ctx: a context on data_ctx.params().drop_last_limb() on the same device (INVALID_ARGUMENT otherwise).  `enc` may be
    // bound to any context of the ring degree.  tokens_per_ciphertext = 2: token A in the real parts, token B in the imaginary parts of the slots - the
    // diagonals are real, so W (x_A + i x_B) = W x_A + i W x_B with the same kernels at half the cost per token; the bias slots are b (1 + i).
    ApproxPackedLinear(const Context& data_ctx, const Context& next_ctx, const ComplexEncoder& enc, HybridKeySwitcher& ks, const double* W, size_t out_dim,
                       size_t in_dim, double weight_scale, double input_scale, size_t tokens_per_ciphertext = 1, const double* bias = nullptr);
    ~ApproxPackedLinear();
    ApproxPackedLinear(const ApproxPackedLinear&) = delete;
    ApproxPackedLinear& operator=(const ApproxPackedLinear&) = delete;
    bool has_bias() const;
    double encode_seconds() const;      // wall time the constructor spent building and encoding the diagonals and the bias
    double output_scale() const;        // input_scale * weight_scale / q_last
    size_t dim() const;                 // m: diagonals per output ciphertext
    size_t in_dim() const;
    size_t out_dim() const;
    size_t input_period() const;        // n
    size_t output_ciphertexts() const;  // batch of y per token
    size_t baby_steps() const;
    size_t giant_steps() const;
    size_t key_switches_per_apply() const;
    size_t tokens_per_ciphertext() const;
    // which output row slot `slot` (< N/2) of output ciphertext `output_ciphertext` holds, or (size_t)-1
    size_t row_of_slot(size_t output_ciphertext, size_t slot) const;
    // slot vectors (N/2 complex values each) <-> plain vectors: x (in_dim values) -> the slots to encode at input_scale and encrypt;
    // output_ciphertexts() * N/2 decoded slots (decode at output_scale()) -> y (out_dim values).  _pair: two tokens, real and imaginary parts.
    void pack_input(const double* x, std::complex<double>* slots) const;
    void pack_input_pair(const double* x_a, const double* x_b, std::complex<double>* slots) const;
    void unpack_output(const std::complex<double>* slots, double* y) const;
    void unpack_output_pair(const std::complex<double>* slots, double* y_a, double* y_b) const;
    // the bound derived above: max_abs_input = the largest |x_i|, input_noise_bound = Bin
    double error_bound(double max_abs_input, double input_noise_bound) const;
    // x: T items on data_ctx (coefficient domain, 2 components, scale input_scale); y: output_ciphertexts() * T items on next_ctx, output ciphertext o of
    // token t at item o * T + t, coefficient domain, scale output_scale().  The stream contract of PackedLinear::apply: enqueues only; the scratch grows
    // only for a larger T than before; one apply() at a time per layer and per key switcher.
    void apply(const Ciphertext& x, Ciphertext& y, Stream* stream = nullptr) const;

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// ApproxPolynomial: slot-wise y = p(x) = sum_{k=0..d} a_k x^k, 2 <= d <= 15, power basis, in the approximate (CKKS-style) family - the non-linearity
// between two ApproxPackedLinear layers.  It needs relinearisation keys only (no Galois keys): one HybridKeySwitcher per level at which a product happens.
//
// Levels.  Depth 0 is the input's context; a product at level r (1 <= r <= r* = ceil(log2 d)) takes operands of depth r - 1, runs on levels[r - 1] (whose
//   data context IS depth r - 1) and leaves its result at depth r, one limb lower.  sum_ctx is depth r*, out_ctx depth r* + 1: depth() = r* + 1 limbs go.
// Schedule.  x^k for k in (2^(r-1), 2^r] is x^(2^(r-1)) * x^(k - 2^(r-1)) at level r; all products of a level are ONE batched
//   HybridKeySwitcher::multiply_rescale_range over (powers x tokens).  An operand of lower depth is first dropped to depth r - 1 by keeping its first limbs
//   (a strided device copy on the stream; the ciphertext and its scale do not change).  All powers are dropped to depth r*, and one dpfhe_lincomb_rescale
//   takes sum_k c_k x^k + c_0 and the rescale by q* (the last prime of sum_ctx) for all tokens.
// Scales, in exactly these double operations (tests/approx_poly_model.py mirrors them):  s_1 = input_scale;  s_k = (s_i * s_j) / (double)q  with
//   i = 2^(ceil(log2 k) - 1), j = k - i and q the prime that product drops (the last prime of depth ceil(log2 k) - 1);  with S = output_scale:
//   c_k = llround(a_k * ((S * (double)q*) / s_k)) for k >= 1, and the constant  c_0 = llround(a_0 * S) q*  as an exact integer product (a_0 S q* itself is
//   far above 2^63 for any useful S under a 60-bit q*; the rescale gives llround(a_0 S) back exactly).  The residues of c_k are the weights; |c_k| >= 2^62
//   (k >= 1) or |llround(a_0 S)| >= 2^62 is INVALID_ARGUMENT.  The output's scale is exactly S.  (Scales near the primes keep s_k near s_1: with
//   s_1 = 2^50 under 60-bit primes s_2 is 2^40.)
//
// Error bound.  ApproxPackedLinear's notation and tools T1 - T4; u = 2^-53, X = max|x|, Bin the input phase's coefficient error; per level r: L_r its data
//   limbs, q_r the prime it drops, rho_r = max_j q_j / P_r, K_r = 21 L_r N rho_r (T4), H = (N + 1) / 2 (T3).  The phase of power k has slot s_k x^k + d_k,
//   |d_k| <= D_k.  D_1 = N Bin (T1).  A tensor product multiplies phases, so slots multiply (T2): (s_i x^i + d_i)(s_j x^j + d_j); the relinearisation
//   adds K_r + H per coefficient after its division by P, the division by q_r divides all of it and adds H, and s_k as a double is off the real
//   s_i s_j / q_r by at most 4 u s_k (two roundings and the conversion of q_r):
//     D_k = (s_i X^i D_j + s_j X^j D_i + D_i D_j + N (K_r + H)) / q_r + N H + 4 u s_k X^k.
//   The weights: c_k = a_k S q* / s_k + r_k with |r_k| <= R_k = 1/2 + 4 u |a_k| S q* / s_k (llround; four roundings in the double expression), and
//   c_0 = a_0 S q* + r_0 with |r_0| <= R_0 = q* (1/2 + 2 u |a_0| S).  A scalar multiple multiplies the phase, the constant is c_0 in every slot, so the sum's slot is S q* p(x) off by at most
//     sum_{k>=1} (R_k s_k X^k + |a_k| (S q* / s_k) D_k + R_k D_k) + R_0;   after the rescale, in units of the output:  pre = that / (S q*) + N H / S  (T3, T1).
//   The decrypted coefficients obey max|c| <= max slot <= S (A + pre), A = sum_k |a_k| X^k, so the client's decode adds D = u8 N (A + pre), u8 = 8 log2(N) u.
//   error_bound(X, Bin) = pre + D bounds |decoded slot - p(x)| for every slot and token, PROVIDED no phase wraps (the caller's choice of limbs: the largest
//   phase, at sum_ctx, is about S q* A).  Worst case throughout; the roundings' N H dominates (2^23 at N = 4096, against scales near 2^60).
//
// Exact on a transparent input (c1 = 0: every relinearisation digit is zero): with mu_1 the input's integer polynomial and (*) the product in
//   Z[X] / (X^N + 1),  mu_k = round(mu_i (*) mu_j / q_r),  M = sum_k c_k mu_k + c_0 X^0,  c0_out = round(M / q*) mod q_l,  c1_out = 0, word for word.
class ApproxPolynomial {
public:
    // levels: ceil(log2 d) key switchers, input level first, levels[r] on the context of the input's limbs without the last r (same ring, same device, same
    // secret); sum_ctx: levels.back()'s data context without its last limb; out_ctx: sum_ctx without its last limb.  coeffs: a_0 .. a_d, finite, d + 1 of
    // them.  INVALID_ARGUMENT for a degree outside [2, 15], a wrong number of levels, contexts that do not form that chain, scales that are not finite and
    // positive, a coefficient that is not finite or a |c_k| >= 2^62.  Everything referenced must outlive the object.
    ApproxPolynomial(const std::vector<HybridKeySwitcher*>& levels, const Context& sum_ctx, const Context& out_ctx, const std::vector<double>& coeffs,
                     double input_scale, double output_scale);
    ~ApproxPolynomial();
    ApproxPolynomial(const ApproxPolynomial&) = delete;
    ApproxPolynomial& operator=(const ApproxPolynomial&) = delete;
    size_t degree() const;                // d
    size_t depth() const;                 // ceil(log2 d) + 1: the limbs between x and y
    double output_scale() const;          // S, exactly
    double power_scale(size_t k) const;   // s_k, 1 <= k <= d
    int64_t weight(size_t k) const;       // c_k, 1 <= k <= d; weight(0) = llround(a_0 S), the constant at the output scale (c_0 = weight(0) q*)
    // the bound derived above; the static form needs no device: data_moduli are the input level's limbs, special_primes one P per level
    double error_bound(double max_abs_input, double input_noise_bound) const;
    static double error_bound(uint32_t log2_n, const std::vector<uint64_t>& data_moduli, const std::vector<uint64_t>& special_primes,
                              const std::vector<double>& coeffs, double input_scale, double output_scale, double max_abs_input, double input_noise_bound);
    // x: T items on levels[0]'s data context (2 components, coefficient domain, scale input_scale); y: T items on out_ctx, scale output_scale().  Enqueues
    // only; the scratch (powers, operands) belongs to the object and grows only for a larger T than before; one apply() at a time per object and per key
    // switcher.
    void apply(const Ciphertext& x, Ciphertext& y, Stream* stream = nullptr) const;

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// ApproxInvSqrt: slot-wise y ~ 1 / sqrt(v) in the approximate family by K Newton steps  y <- y (3 - v y^2) / 2 = 1.5 y - 0.5 (v y)(y y)  on a guess y_0 the
// caller supplies (a low-degree ApproxPolynomial of v: a polynomial alone is a poor 1 / sqrt - on a variance range of 10x a cubic is off by 10 % - while two
// steps take that cubic to 3e-4 and a degree-5 guess to 2e-6).  The division of a LayerNorm by its standard deviation.  Relinearisation keys only.
//
// Levels.  2 K key switchers, input level first, each one limb below the last; y_n lives at scale s_n on level 2 n (the data context of levels[2 n]); out_ctx
//   is level 2 K.  Iteration n, with q_a the last prime of level 2 n and q_b the last prime of level 2 n + 1:
//   1. a = v y_n and b = y_n y_n on levels[2 n] (HybridKeySwitcher::multiply_rescale_range twice; v is brought to the level by keeping its first limbs, as
//      ApproxPolynomial::apply does with its powers), both at level 2 n + 1;
//   2. y_{n+1} = round((-(a (x) b relinearised) + w_n y_n) / q_b) on levels[2 n + 1] in ONE HybridKeySwitcher::multiply_lincomb_rescale_range: the product's
//      weight is exactly -1, so no rounding of a weight touches the product, and y_n is read where it lives, one limb above that level (no copy).
// Scales, in exactly these double operations (tests/invsqrt_model.py mirrors them):  s_0 = guess_scale;
//     s_a = (v_scale * s_n) / (double)q_a;   s_b = (s_n * s_n) / (double)q_a;   top = 2.0 * (s_a * s_b);   w_n = llround(1.5 * (top / s_n));
//     s_{n+1} = top / (double)q_b.
//   -(a b) read at scale top is -0.5 v y^3, and w_n y_n is 1.5 y.  s_{n+1} / s_n = 2 v_scale s_n^2 / (q_a^2 q_b): a guess scale off the balance by a factor c
//   is off by c^3 after one step, c^9 after two - a mismatch grows cubically per step.  balanced_guess_scale(v_scale, q_a, q_b) = sqrt(q_a^2 q_b / (2 v_scale))
//   makes s_1 = s_0 (for primes of one size every s_n then stays there); consult scale(n) before choosing limbs.  INVALID_ARGUMENT when the contexts do not
//   form the chain, a scale is not finite and positive, |w_n| >= 2^62, or any s_n, n <= K, lies outside [2^20, 2^62).
//
// Error bound.  ApproxPolynomial's notation and tools T1 - T4: u = 2^-53, H = (N + 1) / 2 (T3), per level r: L_r its data limbs, rho_r = max_j q_j / P_r,
//   K_r = 21 L_r N rho_r (T4).  V = max|v|, Y a bound on every |y_n| (n <= K, of the real iteration and of its float64 evaluation), Bv and By the coefficient
//   errors of the phases of v and y_0.  The phase of v has slot v_scale v + d_v, |d_v| <= D_v = N Bv (T1; dropping limbs changes nothing); the phase of y_n has
//   slot s_n y_n + e_n with y_n the REAL iterate of the values encrypted, |e_n| <= E_n, E_0 = N By.  One recurrence per iteration.  The products follow
//   ApproxPolynomial's D_k rule (slots multiply (T2), the relinearisation adds K_r + H per coefficient after its division by P, the division by q_a divides all
//   of it and adds H, the scale as a double is off by at most 4 u of itself):
//     D_a = (v_scale V E_n + s_n Y D_v + D_v E_n + N (K_{2n} + H)) / q_a + N H + 4 u s_a V Y
//     D_b = (2 s_n Y E_n + E_n^2             + N (K_{2n} + H)) / q_a + N H + 4 u s_b Y^2
//   The fused step sums  w_n (s_n y_n + e_n) - (s_a v y_n + d_a)(s_b y_n^2 + d_b) = top y_{n+1} + errors: the product of the two phases is off by
//   s_a V Y D_b + s_b Y^2 D_a + D_a D_b, plus N (K_{2n+1} + H) for its relinearisation, plus |w_n| E_n; w_n = 1.5 top / s_n + r with |r| <= R = 1/2 +
//   4 u 1.5 top / s_n (llround; the roundings of the double expression) adds R s_n Y, and top as a double stands for 2 s_a s_b up to u top, which adds
//   u top V Y^3.  The rescale divides all of this by q_b and adds N H; s_{n+1} as a double is off top / q_b by at most 2 u s_{n+1}:
//     E_{n+1} = (s_a V Y D_b + s_b Y^2 D_a + D_a D_b + N (K_{2n+1} + H) + (1.5 top / s_n + R) E_n + R s_n Y + u top V Y^3) / q_b + N H + 2 u s_{n+1} Y.
//   pre = E_K / s_K; the client's decode adds u8 N (Y + pre), u8 = 8 log2(N) u; and the float64 iteration the bound is stated against is itself off the real
//   one by F_K, F_0 = 0, F_{n+1} = 1.5 (1 + V Y^2) F_n + 8 u (1.5 Y + 0.5 V Y^3) (the step's derivative, its five roundings).
//   error_bound(V, Y, Bv, By) = pre + u8 N (Y + pre) + F_K bounds |decoded slot - Y_K| for every slot and token, Y_K the float64 iteration
//   y <- 1.5 y - 0.5 (v y)(y y) from the values actually encrypted, PROVIDED no phase wraps.  How far the GUESS is from 1 / sqrt(v) is the caller's and is
//   not part of it (Newton's own convergence: a relative error e becomes about 1.5 e^2).  Worst case throughout.
//
// Exact on a transparent input (c1 = 0: every relinearisation digit is zero): with mu_v and mu_0 the integer polynomials of v and y_0 and (*) the product in
//   Z[X] / (X^N + 1),  mu_a = round(mu_v (*) mu_n / q_a),  mu_b = round(mu_n (*) mu_n / q_a),  mu_{n+1} = round((w_n mu_n - mu_a (*) mu_b) / q_b),
//   c0_out = mu_K mod q_l,  c1_out = 0, word for word (tests/invsqrt_model.py states it on Python integers, tests/test_gpu_invsqrt_words.py holds the device to it).
class ApproxInvSqrt {
public:
    // levels: 2 K key switchers (K >= 1), input level first, levels[r] on the context of the input's limbs without the last r (same ring, same device, same
    // secret); out_ctx: levels.back()'s data context without its last limb.  Everything referenced must outlive the object.
    ApproxInvSqrt(const std::vector<HybridKeySwitcher*>& levels, const Context& out_ctx, double v_scale, double guess_scale);
    ~ApproxInvSqrt();
    ApproxInvSqrt(const ApproxInvSqrt&) = delete;
    ApproxInvSqrt& operator=(const ApproxInvSqrt&) = delete;
    size_t iterations() const;           // K
    size_t depth() const;                // 2 K: the limbs between (v, y_0) and y
    double scale(size_t n) const;        // s_n, n <= K; scale(K) is the output's
    int64_t weight(size_t n) const;      // w_n, n < K
    // the bound derived above: max_abs_v = V, max_abs_y = Y, v_noise_bound = Bv, guess_noise_bound = By
    double error_bound(double max_abs_v, double max_abs_y, double v_noise_bound, double guess_noise_bound) const;
    // ... and without a device: data_moduli are the input level's limbs (at least 2 K + 1), special_primes one P per level (2 K)
    static double error_bound(uint32_t log2_n, const std::vector<uint64_t>& data_moduli, const std::vector<uint64_t>& special_primes, double v_scale,
                              double guess_scale, double max_abs_v, double max_abs_y, double v_noise_bound, double guess_noise_bound);
    // sqrt(q_a^2 q_b / (2 v_scale)): the guess scale at which s_1 = s_0 (q_a, q_b: the last primes of levels 0 and 1)
    static double balanced_guess_scale(double v_scale, uint64_t q_a, uint64_t q_b);
    // v, y0: T items on levels[0]'s data context (2 components, coefficient domain, scales v_scale and guess_scale); y: T items on out_ctx, scale
    // scale(K).  Enqueues only; the scratch (v at the lower levels, the products, the iterates) belongs to the object and grows only for a larger T than
    // before; one apply() at a time per object and per key switcher.
    void apply(const Ciphertext& v, const Ciphertext& y0, Ciphertext& y, Stream* stream = nullptr) const;

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// ApproxDivide: slot-wise y_{g,j} ~ n_{g,j} / D_g in the approximate family for G groups of T numerators that share a denominator (a softmax's e_j / sum e),
// by K Goldschmidt steps
//     F = 2 - D;    n_j <- n_j F  (j < T);    D <- D F
// on a denominator the caller has brought near 1: D_K = 1 - (1 - D_0)^(2^K) and n_K = (n_0 / D_0) D_K, so K steps leave the relative residual (1 - D_0)^(2^K).
// A constant first guess c ~ 1 / d costs no level - it is a reinterpretation of the scale, s_d d = (s_d / c)(c d): encrypt d at scale s_d and pass
// den_scale = s_d / c.  For d in [lo, hi], guess(lo, hi) = 2 / (lo + hi) puts c d in [1 - rho, 1 + rho], rho = (hi - lo) / (hi + lo), and residual(lo, hi, K) =
// rho^(2^K).  Relinearisation keys only.
//
// Levels.  K key switchers, input level first, each one limb below the last: ONE level per step.  Step n runs on levels[n] in one
//   HybridKeySwitcher::multiply_complement_rescale_range: all T + 1 products of a group share the factor F = kappa_n X^0 - D, which is never written and never
//   transformed; its output - the G T numerators, then the G denominators - is the next step's input as it stands.  The last step runs without the self product.
// Scales, in exactly these double operations (tests/divide_model.py mirrors them):  sigma_0 = den_scale, nu_0 = num_scale; per step n, q_n the prime level n drops:
//     kappa_n = llround(2.0 * sigma_n);    sigma_{n+1} = (sigma_n * sigma_n) / (double)q_n;    nu_{n+1} = (nu_n * sigma_n) / (double)q_n.
//   kappa_n read at scale sigma_n is the constant 2.  sigma_{n+1} / q = (sigma_n / q)^2: a mismatch sigma_0 / q = 1 + delta grows like (1 + delta)^(2^n), so
//   den_scale belongs within about a percent of the primes (consult den_scale(n) before choosing limbs); the numerators' scale is free.  INVALID_ARGUMENT when
//   the contexts do not form the chain, a scale is not finite and positive, a kappa_n >= 2^62, or any sigma_n or nu_n, n <= K, lies outside [2^20, 2^62).
//
// Error bound.  ApproxPolynomial's notation and tools T1 - T4: u = 2^-53, H = (N + 1) / 2 (T3), per level n: L_n its data limbs, rho_n = max_j q_j / P_n,
//   K_n = 21 L_n N rho_n (T4).  Dm a bound on every D_n and X a bound on every |n_{j,n}| (n <= K, of the real iteration and of its float64 evaluation);
//   every D_n lies in [0, Dm] with Dm <= 2 - the iteration's own requirement, it converges for D_0 in (0, 2) only - so that |F_n| = |2 - D_n| <= Fm = 2
//   (error_bound: INVALID_ARGUMENT for Dm > 2); Bd and Bn the coefficient errors of the phases of D_0 and of the numerators.  The phase of D_n has slot
//   sigma_n D_n + e_n with D_n the REAL iterate of the values encrypted, |e_n| <= E_n, E_0 = N Bd (T1); the phase of a numerator has slot nu_n n_n + g_n,
//   |g_n| <= G_n, G_0 = N Bn.  The constant kappa_n X^0 is kappa_n in every slot, exactly, and |kappa_n - 2 sigma_n| <= 1/2 (llround; the doubling is exact):
//   the factor's phase has slot sigma_n F_n + f_n with |f_n| <= E_n + 1/2.  One recurrence per step for each track, by ApproxPolynomial's D_k rule (slots
//   multiply (T2), the relinearisation adds K_n + H per coefficient after its division by P, the division by q_n divides all of it and adds H, a scale as a
//   double is off by at most 4 u of itself: two roundings and the conversion of q_n):
//     E_{n+1} = (sigma_n (Dm (E_n + 1/2) + Fm E_n) + E_n (E_n + 1/2) + N (K_n + H)) / q_n + N H + 4 u sigma_{n+1} Dm
//     G_{n+1} = (nu_n X (E_n + 1/2) + sigma_n Fm G_n + G_n (E_n + 1/2) + N (K_n + H)) / q_n + N H + 4 u nu_{n+1} X
//   (the last step needs no E_K).  pre = G_K / nu_K; the client's decode adds u8 N (X + pre), u8 = 8 log2(N) u; and the float64 iteration the bound is stated
//   against is itself off the real one by Phi_K:  with Psi_n the distance of the float64 D_n, Psi_0 = Phi_0 = 0,
//     Psi_{n+1} = (Fm + Dm) Psi_n + 4 u Dm Fm;    Phi_{n+1} = Fm Phi_n + X Psi_n + 4 u X Fm
//   (each step's derivative; its roundings - one for F, one per product - with a factor 2 of slack for the second-order terms).
//   error_bound(Dm, X, Bd, Bn) = pre + u8 N (X + pre) + Phi_K bounds |decoded slot - n_K| for every slot, numerator and group, n_K the float64 iteration
//   F = 2.0 - D; n = n * F; D = D * F from the values actually encrypted (D_0 = c d, the denominator as read at den_scale), PROVIDED no phase wraps: the phases
//   before a rescale are about nu_n sigma_n X Fm and sigma_n^2 Dm Fm, and a quotient near 1 at a scale near the primes needs TWO limbs on out_ctx (one limb
//   holds |phase| < q / 2 only, and nu_K |y| plus its noise comes within a factor two of that).  How far K steps are from the true quotient is Goldschmidt's
//   own closed form above - |n / D| residual - and is not part of the bound.  Worst case throughout.
//
// Exact on a transparent input (c1 = 0: every relinearisation digit is zero): with mu_D and mu_j the integer polynomials of D and the numerators and (*) the
//   product in Z[X] / (X^N + 1),
//     mu_F = kappa_n X^0 - mu_D (kappa_n on coefficient 0),    mu_j' = round(mu_j (*) mu_F / q_n),    mu_D' = round(mu_D (*) mu_F / q_n),
//   c0_out = mu_j after K steps mod q_l,  c1_out = 0, word for word (tests/divide_model.py states it on Python integers, tests/test_gpu_divide_words.py holds
//   the device to it).
class ApproxDivide {
public:
    // levels: K key switchers (K >= 1), input level first, levels[r] on the context of the input's limbs without the last r (same ring, same device, same
    // secret); out_ctx: levels.back()'s data context without its last limb.  Everything referenced must outlive the object.
    ApproxDivide(const std::vector<HybridKeySwitcher*>& levels, const Context& out_ctx, double num_scale, double den_scale);
    ~ApproxDivide();
    ApproxDivide(const ApproxDivide&) = delete;
    ApproxDivide& operator=(const ApproxDivide&) = delete;
    size_t iterations() const;            // K
    size_t depth() const;                 // K: the limbs between (n, D) and y
    double den_scale(size_t n) const;     // sigma_n, n <= K
    double num_scale(size_t n) const;     // nu_n, n <= K; num_scale(K) is the output's
    int64_t kappa(size_t n) const;        // kappa_n, n < K
    // 2 / (lo + hi): the constant guess for denominators in [lo, hi], 0 < lo <= hi;  ((hi - lo) / (hi + lo))^(2^K): what K steps leave of it
    static double guess(double lo, double hi);
    static double residual(double lo, double hi, size_t K);
    // the bound derived above: max_abs_den = Dm, max_abs_quotient = X, den_noise_bound = Bd, num_noise_bound = Bn
    double error_bound(double max_abs_den, double max_abs_quotient, double den_noise_bound, double num_noise_bound) const;
    // ... and without a device: data_moduli are the input level's limbs (at least K + 1), special_primes one P per level (K)
    static double error_bound(uint32_t log2_n, const std::vector<uint64_t>& data_moduli, const std::vector<uint64_t>& special_primes, double num_scale,
                              double den_scale, double max_abs_den, double max_abs_quotient, double den_noise_bound, double num_noise_bound);
    // num: G T items, group-major, and den: G items (G >= 1, T >= 1), on levels[0]'s data context (2 components, coefficient domain, scales num_scale and
    // den_scale); y: G T items on out_ctx, scale num_scale(K).  Enqueues only; the scratch (the iterates of every level) belongs to the object and grows only
    // for a larger batch than before; one apply() at a time per object and per key switcher.
    void apply(const Ciphertext& num, const Ciphertext& den, Ciphertext& y, Stream* stream = nullptr) const;

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// ApproxProductSum: slot-wise y_g = sum_{k < K} a_{g,k} b_{g,k} in the approximate family, K = terms, under ONE key switch and ONE rescale per group
// (HybridKeySwitcher::multiply_sum_rescale_range: the tensor product is bilinear, so the K products are summed as 3-component ciphertexts in the NTT domain
// before anything else happens to them).  The attention mix out_i = sum_j p_ij v_j (a = the weights, each replicated over its ciphertext's slots; b = the
// values, shared by all queries), a sum of squares or an inner product over several ciphertexts, a giant-step sum.  One level; relinearisation keys only.
//
// Scales.  Every a at a_scale, every b at b_scale;  output_scale() = (a_scale * b_scale) / (double)q_last  in exactly these double operations, q_last the
//   last prime of ks's data context.
//
// Error bound.  ApproxPolynomial's notation and tools T1 - T4: u = 2^-53, H = (N + 1) / 2 (T3), Ld the data limbs, rho = max_j q_j / P, Kr = 21 Ld N rho (T4),
//   q = q_last, S = output_scale().  A = max|a|, B = max|b|, Ba and Bb the coefficient errors of the phases of a and b.  The phase of a_k has slot
//   a_scale a_k + d_a with |d_a| <= D_a = N Ba (T1), that of b_k  b_scale b_k + d_b, |d_b| <= D_b = N Bb.  Term by term:
//   - K product-noise terms.  A tensor product multiplies phases, so slots multiply (T2): (a_scale a_k + d_a)(b_scale b_k + d_b) is off a_scale b_scale a_k b_k
//     by at most a_scale A D_b + b_scale B D_a + D_a D_b, and the K products add up exactly (sums of ciphertexts add phases): K times that.
//   - one key switch: Kr + H per coefficient after its division by P, N (Kr + H) in a slot (T1) - ONCE, where K separate products pay it K times.
//   - one rescale: the division by q divides all of the above and adds H per coefficient, N H in a slot - once, not K times.
//   - S as a double is off the real a_scale b_scale / q by at most 4 u S (two roundings and the conversion of q), which misreads the sum by 4 u S K A B:
//     E = (K (a_scale A D_b + b_scale B D_a + D_a D_b) + N (Kr + H)) / q + N H + 4 u S K A B;    pre = E / S.
//   The client's decode adds u8 N (K A B + pre), u8 = 8 log2(N) u; the float64 sum the bound is stated against is off the real one by at most
//   F = 2 K u K A B (K products and K - 1 additions, (1 + u)^K - 1 <= 2 K u).
//   error_bound(A, B, Ba, Bb) = pre + u8 N (K A B + pre) + F bounds |decoded slot - sum_k a_k b_k| (the float64 sum of the values encrypted, k ascending) for every
//   slot and group, PROVIDED no phase wraps (the phase before the rescale is about a_scale b_scale K A B).  Worst case throughout.
class ApproxProductSum {
public:
    // ks: the key switcher of the level the operands live on (at least two data limbs); it must outlive the object.  INVALID_ARGUMENT for terms == 0 or a scale
    // that is not finite and positive.
    ApproxProductSum(HybridKeySwitcher& ks, size_t terms, bool b_shared, double a_scale, double b_scale);
    ~ApproxProductSum();
    ApproxProductSum(const ApproxProductSum&) = delete;
    ApproxProductSum& operator=(const ApproxProductSum&) = delete;
    size_t terms() const;
    bool b_shared() const;
    double output_scale() const;   // (a_scale * b_scale) / (double)q_last
    // the bound derived above: max_abs_a = A, max_abs_b = B, a_noise_bound = Ba, b_noise_bound = Bb
    double error_bound(double max_abs_a, double max_abs_b, double a_noise_bound, double b_noise_bound) const;
    // ... and without a device: data_moduli are the operands' limbs (at least 2), special_prime the key switcher's P
    static double error_bound(uint32_t log2_n, const std::vector<uint64_t>& data_moduli, uint64_t special_prime, size_t terms, double a_scale, double b_scale,
                              double max_abs_a, double max_abs_b, double a_noise_bound, double b_noise_bound);
    // y: G items on ks's data context without its last limb (2 components), scale output_scale(); a: G * terms items on ks's data context, group-major (2
    // components, coefficient domain, scale a_scale); b: as many at b_scale or, shared, `terms` items every group reads.  Enqueues only; the scratch is the key
    // switcher's (multiply_sum_rescale_range); one apply() at a time per key switcher.
    void apply(const Ciphertext& a, const Ciphertext& b, Ciphertext& y, Stream* stream = nullptr) const;

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// ApproxAttentionScores: the first step of an attention head under encryption, s_ij = post_factor <q_i, k_j>, from T encrypted queries and T encrypted keys: ONE
// all-pairs product step (HybridKeySwitcher::multiply_outer_rescale_range: every operand transformed once, one key switch and one rescale per pair), then ONE
// rotate_add_range over all pairs with SlotSum's elements for (block, stride).  The ladder runs AFTER the rescale, on one limb fewer, so it takes the key
// switcher of the next level (a HybridKeySwitcher is bound to one level: ks_next.data_context() is ks.data_context() without its last limb).
//
// Packings (both: the vector has period block * stride in the slots, so after the ladder every slot holds the total of its residue class modulo stride):
//   one head           the d <= block values of the head in slots 0 .. d - 1 of every period `block`, zeros above d, stride = 1.  The ladder adds the block
//                      slots i, i + 1, ..., i + block - 1 (cyclically inside the period): EVERY slot of pair (i, j) holds sum_d q_i[d] k_j[d].
//   heads interleaved  value `dim` of head `head` in slot dim * stride + head, stride >= the head count (slots head >= heads hold zeros), block = d_head
//                      (GPT-2 small: block 64, stride 16, period 1024).  The ladder adds slots i + e stride, e < block: slot dim * stride + head holds head's
//                      score for every dim - one product and one log2(block)-step ladder give all heads' scores, each replicated over its own head's slots,
//                      the layout a slot-wise mix with v packed the same way needs.
// Output.  Full: T * T items, pair (i, j) at i * T + j; causal: T (T + 1) / 2 items, pair (i, j <= i) at i (i + 1) / 2 + j.
// Scales.  S = (q_scale * k_scale) / (double)q_last is the scale the sums live at;  output_scale() = S / post_factor  in exactly these double operations.  A
//   client that decodes at output_scale() reads post_factor * sum: the factor 1 / sqrt(d_head) (post_factor = 1 / 8 for GPT-2) is folded into the scale and
//   costs no level, as ApproxDivide folds its constant guess.
// Error bound.  A = max|q|, B = max|k| over the slots, Bq, Bk the coefficient errors of the input phases.  The product step is ApproxProductSum at one term:
//   its error_bound(A, B, Bq, Bk) = e1 bounds every slot of a product in units of the values, so S e1 bounds the slot error of its phase, and a coefficient is
//   an average of slots (T1 read backwards: c_k = (2 / N) Re sum_j z_j zeta^(-j k)), so Bin = S e1 bounds the coefficient error that enters the ladder.
//   SlotSum's bound on the next level's limbs, at scale S, with X = A B and that Bin, bounds |decoded slot at scale S - the sum|; reading at output_scale()
//   multiplies values and errors by post_factor, and output_scale() as a double is off S / post_factor by at most 4 u relative:
//   error_bound(A, B, Bq, Bk) = post_factor (SlotSum::error_bound(S, A B, S e1) + 4 u block A B) bounds |decoded slot - post_factor sum_d q_i[d] k_j[d]| (the
//   float64 sum over the class's block slots, ascending) for every slot and pair, provided no phase wraps (the phase is about S block A B).
// Integer model on transparent inputs (c1 = 0, c0 the residues of a known integer polynomial): the product is (a0 b0, 0, 0), every key-switch digit is zero, the
//   division by P is exact, and the words of a pair are round(a0 b0 / q_last) in R followed by the ladder's sums of automorphisms acc <- acc + sigma_g(acc).
class ApproxAttentionScores {
public:
    // ks: the level of q and k (at least two data limbs: the product step drops one); ks_next: the level below it.  Adds SlotSum's
    // elements to ks_next.  Both must outlive the object.  INVALID_ARGUMENT for tokens == 0, a bad (block, stride), scales or a post_factor that are not finite and
    // positive, or a ks_next that is not ks's next level.
    ApproxAttentionScores(HybridKeySwitcher& ks, HybridKeySwitcher& ks_next, size_t tokens, size_t block, size_t stride, bool causal, double q_scale, double k_scale,
                          double post_factor);
    ~ApproxAttentionScores();
    ApproxAttentionScores(const ApproxAttentionScores&) = delete;
    ApproxAttentionScores& operator=(const ApproxAttentionScores&) = delete;
    size_t tokens() const;
    size_t pairs() const;          // tokens^2, or tokens (tokens + 1) / 2 when causal
    bool causal() const;
    double output_scale() const;   // (q_scale * k_scale) / (double)q_last / post_factor
    double error_bound(double max_abs_q, double max_abs_k, double q_noise_bound, double k_noise_bound) const;
    // ... and without a device: data_moduli are the limbs of q and k (at least 2), special_prime the key switchers' P
    static double error_bound(uint32_t log2_n, const std::vector<uint64_t>& data_moduli, uint64_t special_prime, size_t block, double q_scale, double k_scale,
                              double post_factor, double max_abs_q, double max_abs_k, double q_noise_bound, double k_noise_bound);
    // q, k: `tokens` items each on ks's data context (2 components, coefficient domain); scores: pairs() items on ks_next's data context.  Enqueues only after
    // the first call (the ladder's keys are packed then); the product's pairs live in scratch the object owns; one apply() at a time per key switcher.
    void apply(const Ciphertext& q, const Ciphertext& k, Ciphertext& scores, Stream* stream = nullptr) const;

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// PackedSelect: `length` consecutive slots of slot row 0 of a packed ciphertext, starting at `offset`, re-packed as a vector that
// repeats with period `period` (a power of two >= length dividing N/2) along BOTH slot rows - the input packing of a PackedLinear.
// The on-device hand-over between two packed layers when the next layer consumes a SLICE of the previous one's output (the V third of
// a fused QKV product feeding the attention-output projection): one rotation by `offset`, one plaintext mask product (it zeroes
// everything else; costs one multiplicative level of noise, like a layer), log2(N/2 / period) rotate-and-add steps, one row swap.
class PackedSelect {
public:
    // tokens_per_ciphertext = 2: the slice is taken in BOTH slot rows (each row carries its own token) and re-packed inside its row - no row swap at the end
    PackedSelect(const Context& data_ctx, const BatchEncoder& enc, HybridKeySwitcher& ks, size_t offset, size_t length, size_t period, size_t tokens_per_ciphertext = 1);
    ~PackedSelect();
    PackedSelect(const PackedSelect&) = delete;
    PackedSelect& operator=(const PackedSelect&) = delete;
    size_t key_switches_per_apply() const;
    // x, y: T items, 2 components, coefficient domain; enqueues on `stream` and returns, no host synchronisation (scratch belongs to the object and
    // grows only for a larger T than before: one apply() at a time)
    void apply(const Ciphertext& x, Ciphertext& y, Stream* stream = nullptr) const;

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

// PackedTransformerBlock: the LINEAR SKELETON of one GPT-2 block on encrypted, slot-packed hidden states - every dense site of
// /root/reference/src/core/execution/models/gpt_model.cpp:786-859 chained on the device for T tokens:
//     qkv = W_qkv x                      (:793, d -> 3 d, one fused product)
//     a   = v                            attention over ONE position: softmax over a single key is 1, so the attention output IS v
//     h1  = x + W_o a                    attention-output projection + residual
//     h2  = h1 + W_down (W_up h1)        (:848, d -> h -> d) + residual
// over Z_t.  LayerNorm, GELU and the softmax over longer contexts are the non-linear parts an FHE forward cannot take as is
// (SURVEY.md section 7): they are the identity here.  Five multiplicative levels (four matrices + the mask of the v hand-over); the
// caller can watch the budget with Decryptor::noise_budget_bits.  Tokens are independent: a multi-rank driver gives each rank its own
// tokens and needs no collective before the final gather (examples/encrypted_gpt2_block.cpp).
class PackedTransformerBlock {
public:
    // row-major weights with entries < t: W_qkv (3 d x d, rows [q | k | v]), W_o (d x d), W_up (h x d), W_down (d x h)
    PackedTransformerBlock(const Context& data_ctx, const BatchEncoder& enc, HybridKeySwitcher& ks, const uint64_t* W_qkv, const uint64_t* W_o,
                           const uint64_t* W_up, const uint64_t* W_down, size_t d, size_t h);
    // with the biases of the four dense sites (each may be null; values < t): b_qkv (3 d, [q | k | v]), b_o (d), b_up (h), b_down (d):
    //     qkv = W_qkv x + b_qkv,  a = v + b_v,  h1 = x + W_o a + b_o,  h2 = h1 + W_down (W_up h1 + b_up) + b_down   (stage() reports the biased values)
    PackedTransformerBlock(const Context& data_ctx, const BatchEncoder& enc, HybridKeySwitcher& ks, const uint64_t* W_qkv, const uint64_t* W_o,
                           const uint64_t* W_up, const uint64_t* W_down, size_t d, size_t h, const uint64_t* b_qkv, const uint64_t* b_o,
                           const uint64_t* b_up, const uint64_t* b_down);
    ~PackedTransformerBlock();
    PackedTransformerBlock(const PackedTransformerBlock&) = delete;
    PackedTransformerBlock& operator=(const PackedTransformerBlock&) = delete;
    size_t hidden() const;
    size_t inner() const;
    size_t key_switches_per_token() const;
    void pack_input(const uint64_t* x /* d values */, uint64_t* slots /* N */) const;
    void unpack_output(const uint64_t* slots /* N */, uint64_t* y /* d values */) const;
    // x, y: T items (tokens), 2 components, coefficient domain, packed as pack_input packs; y is packed the same way (it can enter the
    // next block as it is).  Enqueues on `stream` and returns (no host synchronisation; the stages and scratch grow only for a larger T than before);
    // one apply() at a time per object.
    void apply(const Ciphertext& x, Ciphertext& y, Stream* stream = nullptr) const;
    // intermediate results of the LAST apply() (T items each; valid until the next one): 0 = qkv (slot r of row 0 = output r), 1 = a = v in
    // the input packing, 2 = h1, 3 = W_up h1 in the input packing of W_down, 4 = h2 (= y)
    const Ciphertext& stage(int index) const;

private:
    class Impl;
    std::unique_ptr<Impl> impl_;
};

}  // namespace fhe
}  // namespace deeppowers
