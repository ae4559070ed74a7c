/*
 * dpfhe.h - C ABI of libdpfhe_hip.so: the MI355X (gfx950) implementation of DeepPowers' FHE
 * ciphertext-arithmetic hot path (negacyclic NTT / inverse NTT over Z_q, coefficient-wise modular
 * mul/add, ciphertext x ciphertext and ciphertext x plaintext multiply).
 *
 * What each entry point replaces in the reference: NOTHING EXISTS THERE.  deeppowers/deeppowers has no
 * Ciphertext/Evaluator/NTT code, so there is no FFI surface to bind to.  These are
 * the entry points SURVEY.md section 8(b) specifies for the path, shaped by the reference's plugin seam
 * and conventions:
 *   - device placement + raw device pointers + optional stream last:
 *       /root/reference/src/core/hal/hal.hpp:36-57 (Device::allocate/memcpy), :95 (launch(cfg, Stream*))
 *   - error numbers are deeppowers::common::ErrorCode values:
 *       /root/reference/src/common/error.hpp:10-40 (SUCCESS=0, OUT_OF_MEMORY=1001, DEVICE_ERROR=1002,
 *       INVALID_ARGUMENT=2000, INVALID_STATE=2002, RUNTIME_ERROR=3000)
 *   - the encrypted matmul sites an Evaluator would serve (callers of dpfhe_matvec_plain):
 *       /root/reference/src/core/execution/models/gpt_model.cpp:793 (QKV), :848 (FFN), :883 (logits)
 *   - the one collective kept (dpfhe_comm_allgather):
 *       /root/reference/src/core/distributed/distributed_context.cpp:97-122 (ncclAllGather), without its
 *       per-call cudaMalloc/stream-create (:109, :88).
 *
 * Conventions
 *   - All data buffers are DEVICE pointers owned by the caller, 16-byte aligned, holding little-endian
 *     u64 words that are canonical residues in [0, q_limb).  Layout: [batch][component][limb][N], contiguous.
 *     "n_rns_polys" counts RNS polynomials (L limbs x N words each); a 2-component ciphertext is 2 of them.
 *   - sizes: every count (batch, n_rns_polys, rows, items, groups, n_words) is a size_t.  A batch is limited by the launch grid of its entry (2^31 - 1
 *     workgroups: "too large for one launch"; first_item + batch <= 2^32 for the seeded samplers) and by nothing else - never by its bytes.  Buffers beyond
 *     4 GiB are supported and tested for every batched entry, buffers beyond 2^32 words (32 GiB) for the flat-indexed ones; the table at the head of
 *     tests/test_gpu_wide_batch.py says which pointer of which entry crosses which line (three calls whose buffers cannot all pass 4 GiB within the
 *     test's memory cap hold their smallest buffer past 2 GiB only).
 *   - forward NTT: natural order in, BIT-REVERSED order out, ahat[k] = sum_j a[j] psi^((2 brv(k)+1) j);
 *     inverse NTT: bit-reversed in, natural out, including N^-1.  Outputs are canonical.
 *   - `stream` is a hipStream_t (NULL = the null stream).  Compute calls only enqueue work and never synchronise.  At log2_n <= 13 (every
 *     BASELINE configuration) they never allocate either: all scratch is caller-provided (d_work / d_digits / ... arguments).  The ONE
 *     exception is spelled out at dpfhe_ctx_create below: at log2_n >= 14 dpfhe_ct_mul, dpfhe_relinearize, dpfhe_switch_key and the two
 *     hybrid entries take their scratch from an arena the context keeps PER STREAM: allocated (hipMalloc) the first time that stream runs such an
 *     operation, grown - after waiting for that arena's own last work only - when a larger slice than ever before arrives, kept until
 *     dpfhe_ctx_destroy; in steady state they neither allocate nor synchronise (one hipEventRecord per call marks the arena's last work).  An arena in
 *     use by a call in progress is never released, by eviction or by dpfhe_ctx_release_scratch (see there).  dpfhe_ctx_create (uploads the tables: one allocation, one copy, no kernel), dpfhe_ctx_autotune
 *     (times kernels on caller scratch) and dpfhe_comm_create are set-up calls: they may allocate and synchronise.  After set-up a dpfhe_ctx is immutable: concurrent calls from different host threads on
 *     different streams are allowed.
 *   - digits: wherever a formula below writes [c]_{q_j} (key switching, relinearisation, the hoisted rotations), it means limb j of c taken as it
 *     is stored - every word read as the integer in [0, q_j), NOT centred on zero - and that integer polynomial reduced modulo each limb of the
 *     context it is then multiplied on ("lift").  A centred digit would differ by q_j in the words above q_j / 2 and give other output words.
 *   - rounding: every round(x / D) below divides by a product D of odd primes, so x / D is never a half-integer and no tie rule is involved:
 *     round(x / D) = floor((2 x + D) / (2 D)).  Where the result is only kept modulo limbs that divide Q / D (dpfhe_rescale, the hybrid entries'
 *     division by P, dpfhe_scale_round) it does not depend on whether x is read centred or in [0, Q): the two readings differ by a multiple of Q / D.
 *   - No C++ types and no exceptions cross this boundary.
 */
#ifndef DPFHE_H
#define DPFHE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dpfhe_ctx dpfhe_ctx;
typedef struct dpfhe_comm dpfhe_comm;

/* deeppowers::common::ErrorCode numbers (/root/reference/src/common/error.hpp:10-40) */
enum {
    DPFHE_SUCCESS = 0,
    DPFHE_OUT_OF_MEMORY = 1001,
    DPFHE_DEVICE_ERROR = 1002,
    DPFHE_INVALID_ARGUMENT = 2000,
    DPFHE_INVALID_STATE = 2002,
    DPFHE_RUNTIME_ERROR = 3000
};

/* dpfhe_ct_mul flags: which domain the inputs are in / the output is wanted in */
enum { DPFHE_IN_NTT = 1u, DPFHE_OUT_NTT = 2u };

/* -- A0: context ----------------------------------------------------------------------------------
 * log2_n in [8, 16] (N > 16384 runs a two-kernel split transform; the fused ct x ct / key-switch kernels stop at 13: above it dpfhe_ct_mul,
 * dpfhe_relinearize and dpfhe_switch_key compose the batched transforms with one-pass streaming kernels and take their scratch from the
 * context's scratch arena of the caller's stream (see "Conventions"; kept until dpfhe_ctx_destroy; large batches run in slices of at most
 * 1 GiB of scratch, or what dpfhe_ctx_set_scratch_limit said); so do the hybrid entries - dpfhe_relinearize_hybrid / dpfhe_switch_key_hybrid, and since round 5 the per-item-key ones:
 * dpfhe_rotate_hybrid_batch / dpfhe_rotate_hybrid_grouped and dpfhe_switch_key_qp; dpfhe_rotate_hoisted_qp and dpfhe_ntt_inv_galois run at every ring degree
 * (the whole packed-layer pipeline at N = 16384, 32768 and 65536; above 16384 dpfhe_ntt_inv_galois is the Galois form of the split inverse and, in place,
 * stages through the arena), and so does dpfhe_rotate_hybrid_hoisted (above N = 8192: the deferred-division pipeline + one inverse transform
 * and division by P per rotation, scratch from the arena; d_work / d_rotated0 are not used there and may be NULL)); n_limbs >= 1; moduli[i] prime < 2^60 with q = 1 (mod 2N); psi[i] a primitive
 * 2N-th root of unity mod q_i (psi^N = -1).  Builds twiddle / Shoup / Barrett tables on device_id. */
int dpfhe_ctx_create(dpfhe_ctx** out, uint32_t log2_n, uint32_t n_limbs, const uint64_t* moduli,
                     const uint64_t* psi, int device_id);
int dpfhe_ctx_destroy(dpfhe_ctx* ctx);
/* set-up call (before the context is shared between threads): the composed large-ring operations (log2_n >= 14) slice their batches so that
 * one slice's scratch stays below `mib` MiB (default 1024).  The library reads NO environment variable. */
int dpfhe_ctx_set_scratch_limit(dpfhe_ctx* ctx, size_t mib);
/* The composed operations take their scratch from one ARENA per (context, stream): a device allocation made at that stream's first composed call (<= the
 * scratch limit above, in 16 MiB steps), grown only for a larger slice than ever before, reused without allocation or synchronisation from then on.
 * A composed call holds its stream's arena for as long as it runs on the host, and an arena in use by a call in progress is never released.  Every call
 * ends by recording an event on its stream; eviction, growth and release wait for the arena's last recorded work - that event - and not for a stream
 * handle, so a stream may be destroyed before its arena is released.  A context keeps at most 16 arenas - when a 17th stream arrives, the least
 * recently used arena that is not in use is released - and more than 16 exist only while more than 16 calls are in progress at once (the next new
 * stream brings the count back).  All of them stay until dpfhe_ctx_destroy unless told otherwise:
 *   dpfhe_ctx_release_scratch(ctx, stream, 0)                  releases the arena of `stream` (NULL = the default stream) - when a phase is over, or a
 *                                                               stream that ran composed operations is gone;
 *   dpfhe_ctx_release_scratch(ctx, NULL, DPFHE_SCRATCH_ALL)    releases every arena of the context.
 * Both wait on the host for the work recorded on what they release.  An arena in use by a call in progress stays, and the call returns
 * DPFHE_INVALID_STATE (after releasing the others); a stream without an arena is no error.
 * dpfhe_ctx_scratch_bytes: device bytes the context's arenas hold right now.  Thread-safe (one mutex per context, not held while waiting or freeing). */
enum { DPFHE_SCRATCH_ALL = 1 };
int dpfhe_ctx_release_scratch(dpfhe_ctx* ctx, void* stream, uint32_t flags);
size_t dpfhe_ctx_scratch_bytes(const dpfhe_ctx* ctx);
uint32_t dpfhe_ctx_log2n(const dpfhe_ctx* ctx);
uint32_t dpfhe_ctx_limbs(const dpfhe_ctx* ctx);
/* 1 if every limb is of the form 2^60 - d, d < 2^24, and the fold-reduction kernels are in use */
int dpfhe_ctx_uses_fold(const dpfhe_ctx* ctx);
/* Which arithmetic the batched transforms and the fused multiply run limb `limb` on (round 6: chosen PER LIMB, not per context):
 *   DPFHE_ARITH_FOLD 2^60 - d, d < 2^24;  DPFHE_ARITH_F64 any prime below 2^47 (residues as IEEE doubles inside a transform, error-free FMA products);
 *   DPFHE_ARITH_FOLD_SCALED 2^k - d0 with 48 <= k < 60 and d0 2^(60-k) < 2^24 (carried scaled to 2^60 - d);  DPFHE_ARITH_F64_WIDE any other prime below 2^50
 *   (doubles again, with reductions inside the transforms);  DPFHE_ARITH_SHOUP every other prime (51 ... 59 bits far from a power of two: Harvey / Shoup
 *   butterflies, 128-bit Barrett products).  Results are the same words whatever the class.  A context of more than 16 limbs, or
 *   with log2_n > 14, is uniform: fold if every limb is, Shoup otherwise.  -1: null context or no such limb.
 * The reference's widest integer type is INT32 (src/core/hal/hal.hpp:27-33): its own parameter sets would land in DPFHE_ARITH_F64. */
enum { DPFHE_ARITH_SHOUP = 0, DPFHE_ARITH_FOLD = 1, DPFHE_ARITH_F64 = 2, DPFHE_ARITH_FOLD_SCALED = 3, DPFHE_ARITH_F64_WIDE = 4 };
int dpfhe_ctx_limb_class(const dpfhe_ctx* ctx, uint32_t limb);

/* -- A0, continued: which FORM of the fused multiply a context launches -------------------------------------------------
 * dpfhe_ct_mul(flags = 0) has two forms at N = 4096 / 8192 on fold-reduction contexts - "quad" (all four forward and all three inverse
 * transforms of a workgroup share twiddle fetches; the default at N = 4096) and "dual" (transforms in pairs; the default at N = 8192) -
 * with identical results and identical HBM traffic.
 * dpfhe_ctx_create takes the default (or the result an earlier dpfhe_ctx_autotune in this process found for the same device, log2_n and
 * n_limbs): it measures nothing, launches nothing and allocates nothing besides the tables.
 * dpfhe_ctx_autotune is the explicit opt-in: it times both forms on CALLER-provided scratch (work_words >= 7 L N; pairs = work_words /
 * (7 L N) synthetic ciphertext pairs; contents are overwritten; synchronises `stream`) and keeps the default unless the other form is
 * >= 3 % faster.  It changes the context: call it before the context is shared between threads.  Other contexts (generic primes, other
 * ring degrees) have one form; the call is a no-op there. */
/* DPFHE_TUNE_CACHED: a PROCESS-WIDE cache, keyed (device, log2_n, n_limbs), remembers what the last explicit dpfhe_ctx_autotune of that shape found;
 * contexts of the same shape created LATER in the process start from it (so behaviour depends on call order: both forms give the same words, only the
 * speed can differ).  dpfhe_tune_cache_clear() empties it.  (Value 1 was DPFHE_TUNE_AT_CREATE until round 4 and is retired: the cached state got a
 * fresh number so that an old caller never misreads it.) */
enum { DPFHE_TUNE_DEFAULT = 0, DPFHE_TUNE_EXPLICIT = 2, DPFHE_TUNE_FORCED = 3, DPFHE_TUNE_CACHED = 4 };
void dpfhe_tune_cache_clear(void);
typedef struct dpfhe_tune_info {
    int32_t chosen;        /* form in use (index for dpfhe_ct_mul_variant_name) */
    int32_t n_variants;    /* forms this context can run (0: one form, nothing measured) */
    int32_t source;        /* DPFHE_TUNE_* : how `chosen` was decided */
    uint32_t probe_pairs;  /* ciphertext pairs per probe launch */
    uint32_t probe_reps;   /* launches per form and pass */
    float probe_us[8];     /* best-pass microseconds per launch of each form (< 0: not measured) */
} dpfhe_tune_info;
int dpfhe_ctx_autotune(dpfhe_ctx* ctx, uint64_t* d_work, size_t work_words, uint32_t reps, void* stream);
int dpfhe_ctx_tune_info(const dpfhe_ctx* ctx, dpfhe_tune_info* out);
int dpfhe_ctx_set_ct_mul_variant(dpfhe_ctx* ctx, int variant);
const char* dpfhe_ct_mul_variant_name(int variant);

/* -- A1 / A2: batched negacyclic NTT, in place and out of place -------------------------------------- */
int dpfhe_ntt_fwd(dpfhe_ctx* ctx, uint64_t* d_io, size_t n_rns_polys, void* stream);
int dpfhe_ntt_inv(dpfhe_ctx* ctx, uint64_t* d_io, size_t n_rns_polys, void* stream);
int dpfhe_ntt_fwd_oop(dpfhe_ctx* ctx, uint64_t* d_out, const uint64_t* d_in, size_t n_rns_polys, void* stream);
int dpfhe_ntt_inv_oop(dpfhe_ctx* ctx, uint64_t* d_out, const uint64_t* d_in, size_t n_rns_polys, void* stream);

/* -- A3: coefficient-wise modular ops (either domain); out may alias a or b ----------------------------- */
int dpfhe_dyadic_mul(dpfhe_ctx* ctx, uint64_t* d_out, const uint64_t* d_a, const uint64_t* d_b, size_t n_rns_polys, void* stream);
int dpfhe_dyadic_mul_add(dpfhe_ctx* ctx, uint64_t* d_acc, const uint64_t* d_a, const uint64_t* d_b, size_t n_rns_polys, void* stream);
int dpfhe_add(dpfhe_ctx* ctx, uint64_t* d_out, const uint64_t* d_a, const uint64_t* d_b, size_t n_rns_polys, void* stream);
int dpfhe_sub(dpfhe_ctx* ctx, uint64_t* d_out, const uint64_t* d_a, const uint64_t* d_b, size_t n_rns_polys, void* stream);
int dpfhe_negate(dpfhe_ctx* ctx, uint64_t* d_out, const uint64_t* d_a, size_t n_rns_polys, void* stream);
/* -- A7 (Evaluator::multiply_plain): d_out[i] = d_a[i] (.) d_pt for the n_rns_polys RNS polynomials of d_a (the components of a batch of
 *    ciphertexts, NTT domain) and ONE plaintext d_pt ([L][N], NTT domain).  One launch; the plaintext's L tiles are re-read from L2.
 *    d_out may alias d_a. */
int dpfhe_multiply_plain(dpfhe_ctx* ctx, uint64_t* d_out, const uint64_t* d_a, const uint64_t* d_pt, size_t n_rns_polys, void* stream);

/* -- A6: ciphertext x ciphertext tensor product, no relinearisation (THE METRIC OP) -----------------
 * d_a2, d_b2: [batch][2][L][N];  d_out3: [batch][3][L][N] = (a0 b0, a0 b1 + a1 b0, a1 b1) in R_q.
 * flags = 0: coefficient domain in and out (4 NTT + 4 dyadic mul + 1 add + 3 inverse NTT per limb, one
 * fused kernel: 7 residue polynomials of HBM traffic per limb).  d_a2 and d_b2 may be the same buffer (squaring); d_out3 must
 * not overlap either operand (DPFHE_INVALID_ARGUMENT). */
int dpfhe_ct_mul(dpfhe_ctx* ctx, uint64_t* d_out3, const uint64_t* d_a2, const uint64_t* d_b2, size_t batch,
                 uint32_t flags, void* stream);

/* -- a SUM of tensor products, one relinearisation later (attention's sum_j p_ij (.) v_j, inner products over several ciphertexts, the giant-step sum of a
 * Paterson-Stockmeyer evaluation): the tensor product is bilinear, so K products are summed BEFORE the key switch, the inverse transforms and the rounding.
 *   d_a2: [groups][terms][2][L][N];  d_b2: [b_groups][terms][2][L][N], b_groups = groups, or 1: every group reads the same `terms` items (shared);
 *   d_out3: [groups][3][L][N],  d_out3[g] = sum_{k < terms} a[g][k] (x) b[g][k]   with (x) dpfhe_ct_mul's (a0 b0, a0 b1 + a1 b0, a1 b1) in R_q.
 * flags: dpfhe_ct_mul's DPFHE_IN_NTT / DPFHE_OUT_NTT; 0 = coefficient domain in and out.  The words are those of the sum taken mod every q_l, however it is
 * taken; with terms = 1 they are dpfhe_ct_mul's.  Every log2_n (8 ... 16) and limb class.
 * Aliasing: the operands are read-only and may alias each other in any way (d_a2 == d_b2 with b_groups == groups is a sum of squares and transforms once);
 * d_out3 must not overlap either operand.
 * Always composed: batched forward transforms of the operands into the arena of the caller's stream (see "Conventions" - here at EVERY log2_n; a shared d_b2
 * is transformed once), one streaming pass, three inverse transforms per group.  Scratch: what the transformed operands take, in slices that honour
 * dpfhe_ctx_set_scratch_limit - whole groups first; when one group does not fit, that group in ranges of terms that accumulate into d_out3 in the NTT domain,
 * its inverse transforms after the last range.  With DPFHE_IN_NTT there is no scratch at all (DPFHE_OUT_NTT only skips the inverse transforms, in place).
 * Enqueues only; allocates only when the stream's arena grows.
 * Algorithmic traffic of the streaming pass per group and limb, in rows of N words: 4 terms + 3 (2 terms + 3 and the shared 2 terms rows once, when shared),
 * against 10 terms + 3 for dpfhe_ct_mul(DPFHE_OUT_NTT) over the pairs, dpfhe_reduce_sum and dpfhe_ntt_inv: that composition writes and re-reads 3 terms rows.
 * DPFHE_INVALID_ARGUMENT, before the device is touched: a null or misaligned (16 bytes) buffer, terms == 0, b_groups not in {1, groups}, an unknown flag, d_out3
 * overlapping an operand, groups * terms too large for one launch.  groups == 0 returns success. */
int dpfhe_ct_mul_sum(dpfhe_ctx* ctx, uint64_t* d_out3, const uint64_t* d_a2, const uint64_t* d_b2, size_t groups, size_t terms, size_t b_groups, uint32_t flags,
                     void* stream);

/* -- products that share a COMPLEMENT factor (a Goldschmidt division step n_j <- n_j F, D <- D F with F = 2 - D, at D's scale): per group g the factor is
 *   F_g = kappa X^0 - b[g] = (kappa - b0, -b1)      - dpfhe_negate on b[g], kappa added to coefficient 0 of component 0 -
 * and every item of the group is multiplied by it; F is never written and never transformed (the transform of kappa X^0 is kappa in every word).
 *   d_a2: [groups][terms][2][L][N];  d_b2: [groups][2][L][N];  d_kappa: [L] canonical residues ON THE DEVICE, word l = kappa mod q_l (dpfhe_lincomb_rescale's d_w convention);
 *   d_out3: [groups * terms + (with_self ? groups : 0)][3][L][N]:  d_out3[g * terms + k] = a[g][k] (x) F_g for k < terms, group-major, then, with_self != 0,
 *   d_out3[groups * terms + g] = b[g] (x) F_g, with (x) dpfhe_ct_mul's (x0 y0, x0 y1 + x1 y0, x1 y1) in R_q.  A relinearisation + rescale over the whole buffer
 *   leaves the next step's numerators and denominators as two contiguous item ranges.
 * flags: dpfhe_ct_mul_sum's.  0 = coefficient domain in and out: the words of dpfhe_negate on b[g], kappa added to coefficient 0 of component 0, and dpfhe_ct_mul
 * of each item with that factor.  In the NTT domain the constant is kappa in every word.  Every log2_n (8 ... 16) and limb class.
 * Aliasing: the operands are read-only and may alias each other in any way; d_out3 must overlap none of d_a2, d_b2, d_kappa.
 * Always composed: batched forward transforms of b and a into the arena of the caller's stream (see "Conventions" - here at EVERY log2_n), one streaming
 * pass, three inverse transforms per output item.  Scratch: what the transformed operands take, in slices of whole groups that honour
 * dpfhe_ctx_set_scratch_limit; when one group does not fit, that group's numerators in ranges, b[g]'s transform kept across the ranges.  With DPFHE_IN_NTT
 * there is no scratch at all (DPFHE_OUT_NTT only skips the inverse transforms, in place).  Enqueues only; allocates only when the stream's arena grows.
 * Algorithmic traffic of the streaming pass per group and limb, in rows of N words: 2 terms + 2 read, 3 (terms + with_self) written - against 4 (terms + with_self)
 * read for dpfhe_ct_mul over the items and a factor copied out per item, after two passes that write the factor.  d_a2 is not read when terms == 0 (it may be NULL).
 * DPFHE_INVALID_ARGUMENT, before the device is touched: a null or misaligned (16 bytes) buffer, terms == 0 without with_self, an unknown flag, d_out3
 * overlapping an operand or d_kappa, groups * (terms + 1) too large for one launch.  groups == 0 returns success. */
int dpfhe_ct_mul_complement(dpfhe_ctx* ctx, uint64_t* d_out3, const uint64_t* d_a2, const uint64_t* d_b2, const uint64_t* d_kappa, size_t groups, size_t terms,
                            int with_self, uint32_t flags, void* stream);

/* -- ALL PAIRS of two lists of ciphertexts, the OUTER product (attention's scores s_ij = <q_i, k_j>: T queries against T keys are T^2 tensor products of 2 T
 * distinct operands): every operand is transformed ONCE, and one streaming pass keeps a tile of 4 queries in registers while the keys stream past.
 *   d_a2: [a_items][2][L][N] (queries);  d_b2: [b_items][2][L][N] (keys);  (x) is dpfhe_ct_mul's (a0 b0, a0 b1 + a1 b0, a1 b1) in R_q;
 *   full form:    d_out3: [a_items * b_items][3][L][N],          d_out3[i * b_items + j] = a[i] (x) b[j];
 *   causal form:  d_out3: [a_items (a_items + 1) / 2][3][L][N],  d_out3[i (i + 1) / 2 + j] = a[i] (x) b[j] for j <= i  (DPFHE_OUTER_CAUSAL; a_items == b_items).
 * flags: dpfhe_ct_mul_sum's DPFHE_IN_NTT / DPFHE_OUT_NTT, and DPFHE_OUTER_CAUSAL.  With flags 0 (coefficient domain in and out) the words are those of
 * dpfhe_ct_mul on the two pair lists a[i], b[j] copied out pair by pair.  Every log2_n (8 ... 16) and limb class.
 * Aliasing: the operands are read-only and may alias each other in any way (d_a2 == d_b2 with a_items == b_items is every product of a list with itself and,
 * when the list fits the scratch limit, transforms once); d_out3 must not overlap either operand.
 * Always composed: batched forward transforms of a and of b into the arena of the caller's stream (see "Conventions" - here at EVERY log2_n), one streaming
 * launch, three inverse transforms per pair, in place.  Scratch, in items of 2 L N words, with fit = the limit of dpfhe_ctx_set_scratch_limit in such items:
 *   a_items + b_items (a_items when d_a2 == d_b2 and a_items == b_items) when that is <= fit: one launch;
 *   otherwise a_items + min(b_items, fit - a_items) when a_items + 1 <= fit: a whole, b in ranges of keys, one launch per range;
 *   otherwise min(a_items, ta) + min(b_items, max(2, fit - ta)) with ta = max(4, fit / 2 rounded down to a multiple of 4): a in ranges of whole tiles of 4
 *   queries, b in ranges of keys, one launch per pair of ranges - 6 items at least, whatever the limit.
 * How the limit is treated: it is honoured whenever it holds 6 items (one tile of 4 queries and 2 keys: the smallest ranges the entry works in); a limit below
 * that is EXCEEDED, to exactly 6 items (min(a_items, 4) + min(b_items, 2) for fewer), as the other composed entries exceed a limit below one item.
 * The products of different ranges are independent (nothing accumulates); under DPFHE_OUTER_CAUSAL the blocks wholly above the diagonal are skipped, keys
 * and all.  With DPFHE_IN_NTT there is no scratch at all (DPFHE_OUT_NTT only skips the inverse transforms, in place).  Enqueues only; allocates only when
 * the stream's arena grows.
 * Algorithmic traffic of the streaming pass per limb, in rows of N words: 2 a_items + 2 b_items ceil(a_items / 4) read, 3 per pair written - against 4 per pair
 * read for dpfhe_ct_mul over pair lists, after the copies that build them (4 rows read and written per pair).
 * DPFHE_INVALID_ARGUMENT, before the device is touched: an unknown flag, DPFHE_OUTER_CAUSAL with a_items != b_items, a null or misaligned (16 bytes) buffer,
 * d_out3 overlapping an operand, a_items * b_items too large for one launch.  The rejections that the arguments alone decide come before the context is
 * looked at.  a_items == 0 or b_items == 0 returns success. */
enum { DPFHE_OUTER_CAUSAL = 4u };
int dpfhe_ct_mul_outer(dpfhe_ctx* ctx, uint64_t* d_out3, const uint64_t* d_a2, const uint64_t* d_b2, size_t a_items, size_t b_items, uint32_t flags, void* stream);

/* diagnostics (tools/ctmul_trace.py): the "quad" form of dpfhe_ct_mul(flags = 0) with timestamps - thread 0 of workgroup w (= pair w / L, limb w % L)
 * writes d_trace[12 w .. 12 w + 11]: s_memrealtime (100 MHz) at start / first operand word arrived / forward transforms done / tensor
 * product done / inverse transforms done / stores issued / stores drained, then HW_ID | XCC_ID << 32, then prologue done / first operand's
 * loads issued / all loads issued / whole first operand arrived.  d_trace: batch * L * 12 words.  N = 4096 fold contexts only. */
int dpfhe_debug_ct_mul_trace(dpfhe_ctx* ctx, uint64_t* d_out3, const uint64_t* d_a2, const uint64_t* d_b2, size_t batch, uint64_t* d_trace, void* stream);

/* -- N1 (first "next" row): relinearisation 3 -> 2 components with RNS-digit evaluation keys ----
 * d_in3: [batch][3][L][N], d_out2: [batch][2][L][N], both coefficient domain.
 * d_evk: [L digits][2][L][N] in the NTT domain: evk_j = (-(a_j s) + e_j + g_j s^2, a_j) with g_j the CRT basis
 * element of limb j (1 mod q_j, 0 mod the others).  (c0', c1') = (c0, c1) + sum_j [c2]_{q_j} (.) evk_j. */
int dpfhe_relinearize(dpfhe_ctx* ctx, uint64_t* d_out2, const uint64_t* d_in3, const uint64_t* d_evk, size_t batch, void* stream);

/* -- N1, second half: rescale (exact RNS "divide by the last prime and round"), coefficient domain.
 * d_in: [n_rns_polys][L][N]  ->  d_out: [n_rns_polys][L-1][N] = round(x / q_{L-1}) limb by limb; requires L >= 2.
 * The result lives at the next level: use a context created with the first L-1 moduli for further work on it. */
int dpfhe_rescale(dpfhe_ctx* ctx, uint64_t* d_out, const uint64_t* d_in, size_t n_rns_polys, void* stream);

/* -- N1, hybrid key switching with ONE special prime P: ctx is the EXTENDED context whose last limb is P (L = Ld + 1
 * limbs); ciphertext data live on the first Ld limbs.  Keys: [Ld digits][2][L][N], NTT domain,
 *   key_j = (-(a_j s) + e_j + P g_j T, a_j)  over all L limbs (T = s^2 for relinearisation, sigma_g(s) for rotations).
 * d_work: caller-provided scratch of batch * 2 * L * N words.  Result (coefficient domain, Ld limbs):
 *   relinearize_hybrid : d_in3 [batch][3][Ld][N] -> d_out2 [batch][2][Ld][N] = (c0, c1) + round(sum_j [c2]_{q_j} key_j / P)
 *   switch_key_hybrid  : d_in2 [batch][2][Ld][N] -> d_out2 = (c0, 0) + round(sum_j [c1]_{q_j} key_j / P)
 * The noise added is ~ Ld N q sigma / P instead of ~ Ld N q sigma. */
int dpfhe_relinearize_hybrid(dpfhe_ctx* ctx_ext, uint64_t* d_out2, const uint64_t* d_in3, const uint64_t* d_key, uint64_t* d_work,
                             size_t batch, void* stream);
int dpfhe_switch_key_hybrid(dpfhe_ctx* ctx_ext, uint64_t* d_out2, const uint64_t* d_in2, const uint64_t* d_key, uint64_t* d_work,
                            size_t batch, void* stream);

/* -- a relinearised product at the next level in one call (the approximate family's ciphertext x ciphertext step): dpfhe_relinearize_hybrid and the
 * dpfhe_rescale that follows it, with ONE rounding pass instead of two.  ctx_ext, d_in3, d_key, d_work (batch * 2 * L * N words) and the overlap rules are
 * dpfhe_relinearize_hybrid's; d_out2 is [batch][2][Ld-1][N], coefficient domain, on the data context's first Ld - 1 limbs:
 *   d_out2 = round( ((c0, c1) + round(sum_j [c2]_{q_j} key_j / P)) / q_{Ld-1} )
 * word for word what dpfhe_rescale on the Ld data limbs makes of dpfhe_relinearize_hybrid's output: the last pass reads the Q P sums on limbs i, Ld-1 and P
 * and (c0, c1) on limbs i and Ld-1, and applies both divisions to the coefficient in registers (each is modular and local to the coefficient).  Every ring
 * degree (above N = 8192 the sums are composed as for dpfhe_relinearize_hybrid, scratch from the stream's arena).  Enqueues only; at log2_n <= 13 it
 * never allocates.  DPFHE_INVALID_STATE when Ld < 2 (no data limb left to drop).
 * dpfhe_relinearize_rescale_pass_host: the host twin of that last pass alone (no device, no context): moduli are the n_limbs = Ld + 1 >= 3 limbs of the
 *   extended basis (odd, >= 3, < 2^60, pairwise coprime), work_qp [batch][2][L][N] the sums over Q P in the coefficient domain, in3 [batch][3][Ld][N]
 *   (components 0 and 1 are read), out [batch][2][Ld-1][N].  Words that are not canonical residues are rejected. */
int dpfhe_relinearize_rescale_hybrid(dpfhe_ctx* ctx_ext, uint64_t* d_out2, const uint64_t* d_in3, const uint64_t* d_key, uint64_t* d_work,
                                     size_t batch, void* stream);
int dpfhe_relinearize_rescale_pass_host(const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n, uint64_t* out, const uint64_t* work_qp,
                                        const uint64_t* in3, size_t batch);

/* -- scalar linear combination + constant + rescale (the final sum of a polynomial in a ciphertext): per item t and component c, coefficient domain,
 *   d_out[t][c] = round( (sum_{k < n_terms} w_k * x[k][t][c]  +  [c = 0] w_K X^0) / q_{L-1} ),   K = n_terms, 1 <= n_terms <= 16
 * d_x: [n_terms][batch][2][L][N] canonical residues (term-major: term k of every item, then term k + 1); d_w: [n_terms + 1][L] canonical residues ON THE
 * DEVICE, word [k][l] = w_k mod q_l, the last row the constant (added to coefficient 0 of component 0 only; a row of zeros for none); d_out:
 * [batch][2][L-1][N].  The rounding is dpfhe_rescale's; the words are those of the sum taken mod every q_l and then rescaled, however the sum is taken.
 * One launch for all items, one pass: 2 n_terms reads and one write per output word.  Enqueues only (no allocation, no synchronise), every log2_n and limb
 * class.  DPFHE_INVALID_STATE when L < 2; DPFHE_INVALID_ARGUMENT, before touching the device, on a null pointer, n_terms outside [1, 16], batch 0, a buffer
 * not 16-byte aligned, d_out overlapping d_x or d_w, or a grid too large for one launch.
 * dpfhe_lincomb_rescale_host: the same words on the host (no device, no context; moduli odd, >= 3, < 2^60 and pairwise coprime, log2_n in [8, 16]; no
 *   alignment rule; words that are not canonical residues are rejected there, on the device they are a caller error). */
int dpfhe_lincomb_rescale(dpfhe_ctx* ctx, uint64_t* d_out, const uint64_t* d_x, const uint64_t* d_w, size_t n_terms, size_t batch, void* stream);
int dpfhe_lincomb_rescale_host(const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n, uint64_t* out, const uint64_t* x, const uint64_t* w,
                               size_t n_terms, size_t batch);

/* -- a relinearised product, a scalar linear combination and the rescale in one call (the second half of a Newton step y (3 - v y^2) / 2, a Horner or
 * Paterson-Stockmeyer step p x + c_k z + c_0, a Chebyshev doubling 2 T_k^2 - 1): ctx_ext, d_in3, d_key, d_work and d_out2 ([batch][2][Ld-1][N]) are exactly
 * dpfhe_relinearize_rescale_hybrid's.  With t = (c0, c1) + round(sum_j [c2]_{q_j} key_j / P) on the Ld data limbs - the words dpfhe_relinearize_hybrid
 * writes - and K = n_terms, per item, component and coefficient
 *   s_l   = w[0][l] t_l + sum_{k<K} w[1+k][l] z_k,l + [component 0, coefficient 0] w[K+1][l]   mod q_l,   l < Ld
 *   out_i = round(s / q_{Ld-1}) mod q_i,   i < Ld - 1        (dpfhe_rescale's rounding)
 * d_terms: HOST array of K device pointers, term_limbs: HOST array of K limb counts; term k is [batch][2][term_limbs[k]][N], coefficient domain, canonical
 *   residues, term_limbs[k] >= Ld, and only the first Ld limbs of each of its polynomials are read: a ciphertext that lives higher up the same prime chain is an
 *   addend as it stands (keeping the first limbs IS the level drop; nothing is copied).  0 <= K <= 15: with the product at most 16 multiply-adds and one
 *   constant, dpfhe_lincomb_rescale's bound on the 128-bit lazy sum.  Both arrays are read during the call only and may be NULL when K = 0.
 * d_w: DEVICE array [K + 2][Ld] of canonical residues: dpfhe_lincomb_rescale's rows with the product's weight in front - row 0 the product's, rows 1 .. K the
 *   terms', row K + 1 the constant (zeros for none).
 * Identities: with K = 0, w[0] = 1 and a zero constant row the result is the words of dpfhe_relinearize_rescale_hybrid; in general it is the words of
 *   dpfhe_relinearize_hybrid followed by dpfhe_lincomb_rescale on the data context over [t, z_0, ..., z_{K-1}] (each z_k cut to its first Ld limbs), however the
 *   sum is taken: all results are canonical residues.
 * One last pass after the key products: t is never written.  Algorithmic traffic of that pass per item, in rows of N words, every row counted once: it reads
 *   the sums (2 L), c0 and c1 (2 Ld) and the first Ld limbs of every term (2 K Ld) and writes 2 (Ld - 1):  2 (L + (K + 2) Ld - 1) rows.  The three entries it
 *   replaces - dpfhe_relinearize_hybrid's last pass, a strided copy of each of the K' terms that are taller or not yet next to t, dpfhe_lincomb_rescale - read
 *   and write the same rows and on top write and re-read t (4 Ld) and every copied term (4 Ld each):  2 (L + (K + 2) Ld - 1) + 4 (1 + K') Ld rows.  At K = K' = 1,
 *   Ld = 4, L = 5: 32 rows against 64.
 * The term pointers travel in the kernel's arguments: nothing is uploaded or allocated per call.  Enqueues only; at log2_n <= 13 it never allocates (above, the
 * key products take arena scratch as in dpfhe_relinearize_hybrid).  Every log2_n (8 ... 16) and limb class.  DPFHE_INVALID_STATE without a special prime or with
 * Ld < 2; DPFHE_INVALID_ARGUMENT, before the device is touched, on a null or misaligned (16 bytes) buffer, n_terms > 15, a term_limbs[k] < Ld, d_out2 or d_work
 * overlapping each other or anything else, or a grid too large for one launch.  batch == 0 returns success.  Read-only buffers may alias each other.
 * dpfhe_relinearize_lincomb_rescale_pass_host: the host twin of that last pass alone (no device, no context, no alignment rule): moduli, work_qp, in3 and out as
 *   for dpfhe_relinearize_rescale_pass_host, terms / term_limbs / w as above but in host memory.  Words that are not canonical residues are rejected (of a
 *   term, the first Ld limbs - the ones that are read). */
int dpfhe_relinearize_lincomb_rescale_hybrid(dpfhe_ctx* ctx_ext, uint64_t* d_out2, const uint64_t* d_in3, const uint64_t* d_key, uint64_t* d_work,
                                             const uint64_t* const* d_terms, const uint32_t* term_limbs, size_t n_terms, const uint64_t* d_w,
                                             size_t batch, void* stream);
int dpfhe_relinearize_lincomb_rescale_pass_host(const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n, uint64_t* out, const uint64_t* work_qp,
                                                const uint64_t* in3, const uint64_t* const* terms, const uint32_t* term_limbs, size_t n_terms,
                                                const uint64_t* w, size_t batch);

/* -- N3, batched rotations (the baby / giant steps of a packed matrix-vector product): item i of the output is the
 * hybrid-key-switched sigma_{galois_elts[i]} of input item i (n_in == batch) or of THE input item (n_in == 1).
 * galois_elts: HOST array of `batch` odd elements < 2N.  d_keys: `batch` keys back to back, each [Ld][2][L][N] as for
 * dpfhe_switch_key_hybrid, key i for element i.  d_work: batch * 2 * L * N words; d_rotated: batch * 2 * Ld * N words
 * (scratch, must not alias the input).  One automorphism launch per 64 items + one key-switch pass for all of them. */
int dpfhe_rotate_hybrid_batch(dpfhe_ctx* ctx_ext, uint64_t* d_out2, const uint64_t* d_in2, size_t n_in, const uint32_t* galois_elts,
                              const uint64_t* d_keys, uint64_t* d_work, uint64_t* d_rotated, size_t batch, void* stream);

/* -- N3, HOISTED rotations: `batch` rotations of ONE ciphertext (d_in2: [2][Ld][N], coefficient domain) sharing the digit
 * decomposition: the Ld digits of c1 are lifted to the L limbs and transformed once (d_digits: Ld * L * N words of scratch), every
 * rotation is then a permutation of those words in the NTT domain, its key inner product and two inverse transforms per limb
 * (instead of Ld + 2), followed by the divide-by-P pass.  Keys and d_work as for dpfhe_rotate_hybrid_batch; d_rotated0:
 * batch * Ld * N words of scratch (sigma_g(c0)).  The result is a valid key switch of sigma_g(ct) but NOT word-identical to
 * dpfhe_rotate_hybrid_batch: here the automorphism acts on the lifted digits (sigma_g after the lift), there on c1 before it.
 * log2_n >= 14 (up to 16): composed from dpfhe_rotate_hoisted_qp, one batched inverse transform and the division by P per rotation - the same words -, in
 * slices of rotations under the scratch limit, scratch from the stream's arena; d_work and d_rotated0 are not touched and may be NULL. */
int dpfhe_rotate_hybrid_hoisted(dpfhe_ctx* ctx_ext, uint64_t* d_out2, const uint64_t* d_in2, size_t n_items, const uint32_t* galois_elts,
                                const uint64_t* d_keys, uint64_t* d_work, uint64_t* d_rotated0, uint64_t* d_digits, size_t batch, void* stream);
/*    n_items input ciphertexts (tokens) share the `batch` rotations and their keys: d_in2 is [n_items][2][Ld][N], the output is
 *    ROTATION-MAJOR, item r * n_items + t = sigma_{galois_elts[r]}(input t); scratch sizes scale with n_items (d_work, d_rotated0:
 *    batch * n_items items; d_digits: n_items * Ld * L * N words).  Workgroups that read the same key tile run next to each other. */

/* -- N3, grouped rotations (giant steps of several tokens): batch = n_elts * group items, item i rotated by galois_elts[i / group]
 *    with key i / group; otherwise as dpfhe_rotate_hybrid_batch with n_in == batch. */
int dpfhe_rotate_hybrid_grouped(dpfhe_ctx* ctx_ext, uint64_t* d_out2, const uint64_t* d_in2, const uint32_t* galois_elts, size_t n_elts, size_t group,
                                const uint64_t* d_keys, uint64_t* d_work, uint64_t* d_rotated, void* stream);

/* -- N3, the rotate-and-add ladder (sums across the slots of one ciphertext): acc_0 = d_in2, acc_{e+1} = acc_e + R_e mod q_l for e < n_steps, d_out2 = acc_{n_steps},
 * where R_e is what dpfhe_rotate_hybrid_grouped(n_elts = 1, group = batch, element galois_elts[e], key e) makes of acc_e:
 *   R_e = (sigma_g c0, 0) + round(sum_j [sigma_g c1]_{q_j} key_j / P),  the automorphism before the digit lift as in dpfhe_rotate_hybrid_batch
 * - word for word that rotation followed by dpfhe_add.  All buffers [batch][2][Ld][N], coefficient domain, canonical residues; every item of a step shares the
 * step's element and key.  galois_elts: HOST array of n_steps odd elements < 2N; d_keys: n_steps keys back to back, each [Ld][2][L][N] as for
 * dpfhe_switch_key_hybrid.  Per step three launches instead of four: sigma_g(c1) alone is materialised (in the c1 slots of the step's output buffer, where
 * the key switch reads it and the last pass overwrites it: no buffer of its own), the key products, and ONE last pass that divides by P, adds the un-rotated
 * input and gathers sigma_g(c0) itself - 7 Ld + 4 L words of N per item and step instead of 14 Ld + 4 L.
 * Scratch, exactly: d_work batch * 2 * L * N words; d_acc batch * 2 * Ld * N words, the ping-pong partner of d_out2 (the last step lands in d_out2; d_out2
 * holds intermediate sums before that) - not read when n_steps == 1, where it may be NULL.  No buffer overlaps another or the input.
 * Enqueues only, every log2_n (8 ... 16) and limb class; above N = 8192 the key products are composed and take arena scratch, exactly as in
 * dpfhe_switch_key_hybrid.  DPFHE_INVALID_STATE on a context without a special prime; DPFHE_INVALID_ARGUMENT, before the device is touched, on n_steps == 0, a
 * null or misaligned buffer, an even element or one >= 2N, overlapping buffers, or a grid too large for one launch.  batch == 0 returns success.
 * dpfhe_rotate_add_pass_host: the host twin of the last pass of ONE step alone (no device, no context): moduli are the n_limbs = Ld + 1 >= 2 limbs of the
 *   extended basis (odd, >= 3, < 2^60, P coprime to every data limb), work_qp [batch][2][L][N] the key products over Q P in the coefficient domain, in2 [batch][2][Ld][N] the
 *   step's input, out [batch][2][Ld][N]:  out.c0 = round(work.c0 / P) + in.c0 + sigma_g(in.c0),  out.c1 = round(work.c1 / P) + in.c1.  Words that are not
 *   canonical residues are rejected. */
int dpfhe_rotate_add_hybrid(dpfhe_ctx* ctx_ext, uint64_t* d_out2, const uint64_t* d_in2, const uint32_t* galois_elts, const uint64_t* d_keys, uint64_t* d_work,
                            uint64_t* d_acc, size_t n_steps, size_t batch, void* stream);
int dpfhe_rotate_add_pass_host(const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n, uint64_t* out, const uint64_t* work_qp, const uint64_t* in2,
                               uint32_t galois_elt, size_t batch);

/* -- N3, round 3: baby-step / giant-step sums with the division by P DEFERRED ("double hoisting", Bossuat-Mouchet-Troncoso-Pastoriza-
 * Hubaux 2021).  A rotated term is kept in the NTT domain over the extended basis Q P as  P sigma_g(ct) + key-switching noise;
 * plaintext products and sums are taken there, and one inverse transform + divide-by-P is paid per SUM, not per rotation.
 * Stages (ctx_ext = data moduli + special prime P as its last limb; QP buffers are [..][2][L][N], data buffers [..][2][Ld][N]):
 *
 * dpfhe_rotate_hoisted_qp: n_items coefficient-domain inputs d_in2 [n_items][2][Ld][N] -> d_out_qp [(1 + batch)][n_items][2][L][N], NTT
 *   domain (forward-output order), canonical:  block 0 = (P c0, P c1) (the input itself);  block 1 + r, r < batch =
 *     ( sum_j NTT(sigma_g lift([c1]_{q_j})) (.) key_{g,j,0} + P NTT(sigma_g c0),  sum_j NTT(sigma_g lift([c1]_{q_j})) (.) key_{g,j,1} ),  g = galois_elts[r]
 *   (the P c0 term is 0 on the special limb).  Keys as for dpfhe_rotate_hybrid_hoisted.  Scratch: d_in_ntt n_items * 2 * Ld * N words,
 *   d_digits n_items * Ld * L * N words.  round(block / P) after an inverse transform equals dpfhe_rotate_hybrid_hoisted's output.
 *   Every ring degree: the stream kernels take log2_n at run time; at log2_n = 15, 16 the transforms of the inputs and digits are the split ones.
 * dpfhe_ntt_inv_galois (any context): block e of rns_polys_per_elt RNS polynomials:  d_out = sigma_{galois_elts[e]}(INTT(d_in)), the
 *   automorphism applied as a gather in the NTT domain (no separate pass).  d_out == d_in, or disjoint from it.  log2_n = 15, 16 (split transform,
 *   uniform fold / generic contexts): sub-transform b of NTT(sigma_g a) gathers from ONE other sub-block of NTT(a), then the column stages run unchanged -
 *   two kernels and the plain split inverse's 4 N words of traffic per polynomial.  There a call with d_out == d_in MAY TAKE ARENA SCRATCH: the
 *   sub-transforms' output is staged in the stream's arena (one launch group of at most 64 elements at a time, fewer under dpfhe_ctx_set_scratch_limit);
 *   no allocation and no synchronisation once the arena has that size.  Out of place it writes straight to d_out.
 * dpfhe_switch_key_qp: batch = n_keys * group coefficient-domain items d_in2 [batch][2][Ld][N], item i with key i / group ->
 *   d_out_qp [batch][2][L][N] = sum_j NTT(lift([c1]_{q_j})) (.) key_j, NTT domain, nothing added, no division: the giant steps'
 *   terms, to be summed (dpfhe_reduce_sum on ctx_ext), inverse-transformed once and finished by
 * dpfhe_rescale_bsgs: d_in_qp [batch][2][L][N] (coefficient domain) -> d_out2 [batch][2][Ld][N] = round(in / P) + addends, where
 *   d_addends is [n_add][batch][2][Ld][N]: component 0 adds component 0 of ALL n_add items, component 1 adds component 1 of item 0
 *   only (the rotated inner sums of a baby-step / giant-step product: item 0 is not rotated; the c1 of the others went into
 *   dpfhe_switch_key_qp). */
int dpfhe_rotate_hoisted_qp(dpfhe_ctx* ctx_ext, uint64_t* d_out_qp, const uint64_t* d_in2, size_t n_items, const uint32_t* galois_elts,
                            const uint64_t* d_keys, uint64_t* d_in_ntt, uint64_t* d_digits, size_t batch, void* stream);
int dpfhe_ntt_inv_galois(dpfhe_ctx* ctx, uint64_t* d_out, const uint64_t* d_in, size_t rns_polys_per_elt, const uint32_t* galois_elts, size_t n_elts,
                         void* stream);
int dpfhe_switch_key_qp(dpfhe_ctx* ctx_ext, uint64_t* d_out_qp, const uint64_t* d_in2, const uint64_t* d_keys, size_t n_keys, size_t group, void* stream);
int dpfhe_rescale_bsgs(dpfhe_ctx* ctx_ext, uint64_t* d_out2, const uint64_t* d_in_qp, const uint64_t* d_addends, size_t n_add, size_t batch,
                       void* stream);

/* -- round 4 (what an EXACT ciphertext x ciphertext multiply needs around dpfhe_ct_mul): limb ranges of one context ------------
 * dpfhe_base_extend: per coefficient, the integer X in (-Qs/2, Qs/2] whose residues modulo the source limbs [src_limb0, src_limb0 + n_src)
 *   are given (Qs their product, n_src <= 10) is reduced modulo the destination limbs [dst_limb0, dst_limb0 + n_dst) (n_dst <= 20; the ranges may
 *   overlap - a destination limb that is also a source limb gets its own residue back).  Exact (mixed-radix reconstruction), not approximate.
 *   d_in: item p's source residues at d_in + (p * in_stride_limbs + i) * N, i < n_src;  d_out: item p's results at d_out + (p * out_stride_limbs + j) * N.
 * dpfhe_scale_round: d_in [n_polys][L][N] holds ALL limbs of the context;  d_out (item stride out_stride_limbs) receives, on the kept limbs
 *   [keep_limb0, keep_limb0 + n_keep),  round(multiplier * X / Qd)  where X is the (centred) integer the L limbs represent and Qd the product of the
 *   dropped limbs [drop_limb0, drop_limb0 + n_drop) (n_drop <= 10, disjoint from the kept ones) - exact as long as |multiplier * X| < Q / 2.
 *   With multiplier = the plaintext modulus t and Qd = the operands' ciphertext modulus this is the scale-and-round of a BFV-style multiply:
 *   extend both operands to the whole context, dpfhe_ct_mul there, dpfhe_scale_round, dpfhe_base_extend back (Evaluator::multiply_exact). */
int dpfhe_base_extend(dpfhe_ctx* ctx, uint64_t* d_out, size_t out_stride_limbs, const uint64_t* d_in, size_t in_stride_limbs, uint32_t src_limb0, uint32_t n_src,
                      uint32_t dst_limb0, uint32_t n_dst, size_t n_polys, void* stream);
int dpfhe_scale_round(dpfhe_ctx* ctx, uint64_t* d_out, size_t out_stride_limbs, const uint64_t* d_in, uint32_t drop_limb0, uint32_t n_drop, uint32_t keep_limb0,
                      uint32_t n_keep, uint64_t multiplier, size_t n_polys, void* stream);

/* -- N3: Galois automorphism a(X) -> a(X^galois_elt) (galois_elt odd, < 2N), coefficient domain, d_out != d_in;
 *        and the key switch that follows it:  (c0', c1') = (c0 + sum_j [c1]_{q_j} (.) key_j[0], sum_j [c1]_{q_j} (.) key_j[1]),
 *        key_j = (-(a_j s) + e_j + g_j sigma(s), a_j) in the NTT domain, layout [L][2][L][N] like the relinearisation keys. */
int dpfhe_apply_galois(dpfhe_ctx* ctx, uint64_t* d_out, const uint64_t* d_in, size_t n_rns_polys, uint32_t galois_elt, void* stream);
int dpfhe_switch_key(dpfhe_ctx* ctx, uint64_t* d_out2, const uint64_t* d_in2, const uint64_t* d_key, size_t batch, void* stream);

/* -- A7: ciphertext x plaintext matrix-vector product, everything in the NTT domain ------------------
 * d_W: [rows][cols][L][N] plaintext polys; d_x: [cols][2][L][N]; d_y: [rows][2][L][N],
 * y_i = sum_j W_ij (.) x_j  with 128-bit lazy accumulation and one reduction at the end. */
int dpfhe_matvec_plain(dpfhe_ctx* ctx, uint64_t* d_y, const uint64_t* d_W, const uint64_t* d_x, size_t rows,
                       size_t cols, void* stream);

/* -- A7 with n_rhs right-hand sides (tokens): x is [cols][n_rhs][2][L][N], y is [rows][n_rhs][2][L][N] (the token index sits between
 *    the column / row and the component); y[i][t] = sum_j W[i][j] (.) x[j][t].  W is streamed from HBM once: 2 right-hand sides (4 polynomials) x 4 rows per workgroup, the groups of a W tile adjacent on one XCD. */
int dpfhe_matvec_plain_multi(dpfhe_ctx* ctx, uint64_t* d_y, const uint64_t* d_W, const uint64_t* d_x, size_t rows, size_t cols, size_t n_rhs,
                             void* stream);

/* scalar-weight variant (the realistic plaintext linear layer: W_ij in Z_q, given as one residue per limb):
 * d_w: [rows][cols][L] words;  y_i = sum_j w_ij * x_j.  Works in either domain (scalars commute with the NTT). */
int dpfhe_matvec_scalar(dpfhe_ctx* ctx, uint64_t* d_y, const uint64_t* d_w, const uint64_t* d_x, size_t rows,
                        size_t cols, void* stream);

/* -- A8: modular sum of `count` ciphertexts of `components` RNS polys each into one ------------------
 * d_in: [count][components][L][N] -> d_out: [components][L][N].  (shard-local reduce before the all-gather) */
int dpfhe_reduce_sum(dpfhe_ctx* ctx, uint64_t* d_out, const uint64_t* d_in, size_t count, size_t components, void* stream);

/* -- measurement aid (SURVEY.md 8(d) "also report a measured device-copy bandwidth as the practical ceiling"): a plain device-to-device
 * copy of n_words (even) u64 words with the access shape of the library's streaming kernels (16 bytes per lane, eight loads in
 * flight per thread).  bench.py reads the transforms' HBM rates against it. */
int dpfhe_copy(dpfhe_ctx* ctx, uint64_t* d_dst, const uint64_t* d_src, size_t n_words, void* stream);

/* -- (e): the one collective - RCCL all-gather of one partial ciphertext per rank over xGMI ----------
 * One process per GPU.  Rank 0 calls dpfhe_comm_unique_id, ships the 128 bytes to the other ranks by any
 * means (the host program's own rendezvous), every rank calls dpfhe_comm_create.  d_recv holds
 * world_size * words_per_rank words; rank r's contribution lands at offset r * words_per_rank. */
int dpfhe_comm_unique_id(uint8_t out_id[128]);
int dpfhe_comm_create(dpfhe_comm** out, const uint8_t id[128], int rank, int world_size, int device_id);
int dpfhe_comm_destroy(dpfhe_comm* comm);
int dpfhe_comm_allgather(dpfhe_comm* comm, uint64_t* d_recv, const uint64_t* d_send, size_t words_per_rank, void* stream);
/* (SURVEY.md section 8(b) lists this exchange as `dpfhe_allgather_partials`; it is exported under the dpfhe_comm_* names above, with the communicator's
 *  life cycle next to it.)
 * The alternative SURVEY.md section 8(e) asks to have measured: ncclAllReduce(ncclUint64, ncclSum) of the ranks' partial ciphertexts IN PLACE, then one
 * mod-q pass (dpfhe_canonicalize_sum) - world_size <= 15, since 15 q < 2^64 for q < 2^60.  The result is what all-gather + the local sum give.
 * dpfhe_canonicalize_sum alone: words that are sums of at most 15 canonical residues -> canonical residues, in place (the pass after a
 * torch.distributed all_reduce of the partials). */
int dpfhe_comm_allreduce_sum(dpfhe_comm* comm, dpfhe_ctx* ctx, uint64_t* d_io, size_t n_rns_polys, void* stream);
int dpfhe_canonicalize_sum(dpfhe_ctx* ctx, uint64_t* d_io, size_t n_rns_polys, void* stream);

/* -- seeded uniform polynomials: the uniform half of a fresh symmetric ciphertext (c1) or of a key (a_j) travels as a 32-byte seed.
 * expand(seed, item, limb, component) has N coefficients mod q_limb: ChaCha20 block function of RFC 8439 section 2.3 with key = seed (8 little-endian
 * words), 32-bit block counter = k / 4 and nonce = (item, limb, component) as u32 words; coefficient k is output words 4 (k mod 4) .. +3 read as one
 * 128-bit little-endian integer X, reduced exactly: X mod q_limb.  `limb` is the limb's index in the context (a context of the first m moduli expands the
 * first m limbs of the full one).  The words are the same whatever the limb's arithmetic class and whichever domain the buffer is in.
 * The seed is public: security rests on ChaCha20 as a PRG with a public seed.  Never reuse a seed under one secret key (equal c1 leak c0 - c0').
 * dpfhe_expand_uniform: writes component `component` of items 0 .. batch-1 of d_buf [batch][components][L][N] as expand(seed, first_item + b, l, component)
 *   and leaves every other word untouched.  DPFHE_INVALID_ARGUMENT on null pointers, component >= components, first_item + batch > 2^32.
 * dpfhe_expand_uniform_host: the same on the host (no device, no context); moduli odd, >= 3 and < 2^60, log2_n in [8, 16]. */
int dpfhe_expand_uniform(dpfhe_ctx* ctx, uint64_t* d_buf, size_t batch, size_t components, uint32_t component, const uint8_t seed[32],
                         uint64_t first_item, void* stream);
int dpfhe_expand_uniform_host(const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n, uint64_t* out, size_t batch, size_t components,
                              uint32_t component, const uint8_t seed[32], uint64_t first_item);

/* -- exact plaintext addition: a plaintext b over Z_t added to (or, negate != 0, subtracted from) exact BFV-style ciphertexts - the bias of an encrypted
 * linear layer.  d_in, d_out: [batch][comps][L][N] coefficient-domain ciphertexts (comps 2 or 3: also an unrelinearised product); d_plain: [plain_items][N]
 * words b in [0, 2^32) (BatchEncoder::decode's input convention); ciphertext item i uses plaintext item i / (batch / plain_items).
 * Component 0 becomes c0 +- round(Q b / t) mod q_l, Q = prod q_l; the other components are copied when d_out != d_in (in place is allowed).
 * t odd, 3 <= t < 2^32, coprime to every q_l.  DPFHE_INVALID_ARGUMENT, before touching the device, on a null pointer, comps not 2 or 3, batch not a
 * multiple of plain_items, such a t, or out and in overlapping without being the same buffer.
 * dpfhe_add_plain_scaled_host: the same words on the host (no device, no context; moduli odd, >= 3 and < 2^60, log2_n in [8, 16]; plaintext words
 * >= 2^32 are rejected there, on the device they are a caller error). */
int dpfhe_add_plain_scaled(dpfhe_ctx* ctx, uint64_t* d_out, const uint64_t* d_in, const uint64_t* d_plain, size_t batch, size_t comps, size_t plain_items,
                           uint64_t t, int negate, void* stream);
int dpfhe_add_plain_scaled_host(const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n, uint64_t* out, const uint64_t* in, const uint64_t* plain,
                                size_t batch, size_t comps, size_t plain_items, uint64_t t, int negate);

/* -- plaintext addition on residues: a plaintext polynomial p, given as residues over the ciphertext's own limbs, added to (or, negate != 0, subtracted
 * from) component 0 - the bias of an approximate (CKKS-style) layer at the ciphertext's scale, or any plaintext add where no scaling by Q / t applies.
 * d_in, d_out: [batch][comps][L][N] canonical residues (comps 2 or 3); d_plain: [plain_items][L][N] canonical residues, word [item][l][k] in [0, q_l) -
 *   the default output of dpfhe_encode_complex or dpfhe_encode_slots, or their DPFHE_ENCODE_NTT output.  The entry works in either domain (addition
 *   commutes with the transform): the caller passes operands of the SAME domain.  Ciphertext item i uses plaintext item i / (batch / plain_items).
 * Component 0 becomes c0 +- p mod q_l, canonical; the other components are copied when d_out != d_in (in place is allowed).
 * dpfhe_add_plain enqueues only (no allocation, no synchronise) on every log2_n and every limb class.  DPFHE_INVALID_ARGUMENT, before touching the
 *   device, on a null pointer, comps not 2 or 3, batch 0, batch not a multiple of plain_items, a buffer not 16-byte aligned, out and in overlapping
 *   without being the same buffer, out overlapping the plaintext, or a grid too large for one launch (batch max(N / 512, 1) > 2^31 - 1).
 * dpfhe_add_plain_host: the same words on the host (no device, no context; moduli odd, >= 3 and < 2^60, log2_n in [8, 16]; no alignment rule; a
 *   plaintext word >= q_l is rejected there, on the device it is a caller error). */
int dpfhe_add_plain(dpfhe_ctx* ctx, uint64_t* d_out, const uint64_t* d_in, const uint64_t* d_plain, size_t batch, size_t comps, size_t plain_items,
                    int negate, void* stream);
int dpfhe_add_plain_host(const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n, uint64_t* out, const uint64_t* in, const uint64_t* plain,
                         size_t batch, size_t comps, size_t plain_items, int negate);

/* -- compact result ciphertexts (stream DPFHEc1): a public modulus switch of 2-component ciphertexts from Q = prod q_l to 2^k, then bit-packing.
 * d_in: [batch][2][L][N] coefficient-domain canonical residues, X in [0, Q) a coefficient's CRT value; component c becomes, with k = bits_c,
 *   round(2^k X / Q) mod 2^k  (Q is odd: no tie).  d_out: batch records of N (bits0 + bits1) / 8 bytes; item i's record starts at byte i N (bits0 + bits1) / 8,
 *   component 0 (N bits0 / 8 bytes) first; value j holds bits [j k, (j + 1) k) of its component's little-endian bit string (bit b: bit b % 8 of byte b / 8).
 * Decryption (client): K = max(bits), phase = c0 2^(K - bits0) + (c1 * s) 2^(K - bits1) mod 2^K, m = round(t phase / 2^K) mod t.
 * dpfhe_compact enqueues only (no allocation, no synchronise).  DPFHE_INVALID_ARGUMENT on a null pointer, batch 0, a width outside [8, 60],
 *   more than 10 limbs (rescale first), in or out not 16-byte aligned, in and out overlapping, or a grid too large for one launch.
 * dpfhe_compact_host: the same bytes on the host (no device, no context); also rejects log2_n outside [8, 16] and moduli that are even, < 3, >= 2^60
 *   or not pairwise coprime. */
int dpfhe_compact(dpfhe_ctx* ctx, uint8_t* d_out, const uint64_t* d_in, size_t batch, uint32_t bits0, uint32_t bits1, void* stream);
int dpfhe_compact_host(const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n, uint8_t* out, const uint64_t* in, size_t batch,
                       uint32_t bits0, uint32_t bits1);

/* -- slot encoding over Z_t: slot vectors -> message polynomials on the device (what BatchEncoder::encode + lift_signed + an upload did on the host).
 * Definition.  N = 2^log2_n; t prime, t < 2^32, t = 1 mod 2N.  zeta = g^((t-1)/2N) mod t for the smallest g >= 2 with zeta^N = -1 mod t (dpfhe_encoder_root).
 *   The N slots are 2 rows of N/2.  The message polynomial m (degree < N, coefficients mod t) is the one with
 *       m(zeta^(3^i)) = slots[i],   m(zeta^(-3^i)) = slots[N/2 + i],   0 <= i < N/2, exponents mod 2N
 *   (N values fix a polynomial of degree < N; X -> X^(3^s) rotates both rows left by s slots, X -> X^(2N-1) swaps them).
 *   DPFHE_ENCODE_PLAIN: out is [items][N], word k = coefficient a_k of m in [0, t) - the operand of dpfhe_add_plain_scaled.
 *   default (flags 0):  out is [items][L][N], word [item][l][k] = c_k mod q_l in [0, q_l), c_k = a_k - t if a_k > floor(t/2), else a_k (the centred
 *       coefficient), for every limb l of the context.  A limb may be smaller than t, and t need not be coprime to the q_l: the residue is exact either way.
 *   DPFHE_ENCODE_NTT:   the residue output, then the context's forward transform of it in place (the words dpfhe_ntt_fwd makes of the default output);
 *       invalid together with DPFHE_ENCODE_PLAIN.
 * dpfhe_encoder_create is a set-up call (one allocation, one copy: the powers of zeta^-1 with their quotients, the slot -> position table, the limb
 *   constants).  The encoder is bound to `ctx` (its N and limbs), which must outlive it; it is immutable afterwards and may be shared between threads.
 *   DPFHE_INVALID_ARGUMENT, before touching the device, on a null pointer, t >= 2^32, t not prime, t != 1 mod 2N.  Destroying null is safe.
 * dpfhe_encode_slots enqueues only (no allocation, no synchronise): d_slots is [items][N] 32-bit slot values, 16-byte aligned like d_out.  A slot value
 *   >= t is a caller error; the device REDUCES it mod t (it never faults).  DPFHE_INVALID_ARGUMENT on a null pointer, items 0, an unknown flag bit, PLAIN
 *   with NTT, a misaligned buffer, out and slots overlapping, or more than (2^31 - 1) / N items (one launch).  At log2_n >= 15 the transform is two kernels
 *   and parks its intermediate words in d_out itself.
 * dpfhe_encode_slots_host: the same words on the host (no device, no context; moduli odd, >= 3 and < 2^60, log2_n in [8, 16]); rejects a slot value
 *   >= t and DPFHE_ENCODE_NTT as well. */
typedef struct dpfhe_encoder dpfhe_encoder;
enum { DPFHE_ENCODE_PLAIN = 1u, DPFHE_ENCODE_NTT = 2u };
int dpfhe_encoder_create(dpfhe_encoder** out, dpfhe_ctx* ctx, uint64_t t);
int dpfhe_encoder_destroy(dpfhe_encoder* enc);
uint64_t dpfhe_encoder_root(const dpfhe_encoder* enc);
int dpfhe_encode_slots(dpfhe_encoder* enc, uint64_t* d_out, const uint32_t* d_slots, size_t items, uint32_t flags, void* stream);
int dpfhe_encode_slots_host(const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n, uint64_t t, uint64_t* out, const uint32_t* slots, size_t items,
                            uint32_t flags);

/* -- complex slot encoding: vectors of real or complex numbers -> the integer polynomials of the approximate (CKKS-style) family, on the device.
 * Definition.  N = 2^log2_n, n = N/2, xi = exp(i pi / N), a primitive 2N-th root of unity in C.  A vector of n complex slots z_0 .. z_(n-1) fixes the
 *   real polynomial m of degree < N with
 *       m(xi^(3^i)) = z_i,   m(xi^(-3^i)) = conj(z_i),   0 <= i < n, exponents mod 2N
 *   (the slot generator is 3, as for Z_t; X -> X^(3^s) rotates the slots left by s, cyclically over n, and X -> X^(2N-1) conjugates them).  Its
 *   coefficients are m_k = (2/N) Re( sum_i z_i xi^(-3^i k) ).  With a scale Delta (a positive finite double) the encoding is c_k = round(Delta m_k).
 * Accuracy.  The transform is FP64 and cannot be pinned word for word by a formula; it is pinned by a bound and by an identity.
 *   Bound: |c_k - Delta m_k| <= 1/2 + E,  E = 8 log2(N) 2^-53 Delta max_i |z_i|   (no intermediate overflowing or subnormal).
 *   Derivation (u = 2^-53).  The schedule is log2(N) - 1 levels of radix-2 butterflies (a + b, (a - b) w) on n complex words, then one multiplication of
 *   every word by Delta / n (a power-of-two fraction of Delta: exact).  Per level a word takes one complex addition (relative error u), and on one branch
 *   one complex product of 4 multiplications and 2 additions (sqrt(8) u) with a twiddle whose components are correctly rounded (u / sqrt(2)): at most
 *   g = (1 + sqrt(8) + 1/sqrt(2)) u < 4.54 u of its modulus.  The exact word after l levels is a sum of 2^l slots times unit factors, at most 2^l max|z|,
 *   and reaches an output through 2^(levels - l) unit factors, so each level adds at most g n max|z| to an output before the scaling, g Delta max|z|
 *   after it; the scaling adds u.  First order total (4.54 (log2(N) - 1) + 1) u Delta max|z|; the second-order terms are below 2^-40 of that.  8 holds.
 *   Identity: the device gives the words of dpfhe_encode_complex_host, bit for bit: both run the same IEEE additions, multiplications and rint in the
 *   same order (no fused multiply-add, no division, no sincos on the device) on one twiddle table built on the host.
 * Conversion.  y_k is the double the transform gives for Delta m_k: NaN -> 0; otherwise clamped to [-2^62, 2^62], then rint (ties to even).  Values outside
 *   that range (or non-finite slots) are a caller error with this defined result; the entry never faults on any input.
 * Output forms (the DPFHE_ENCODE_* flags above, and):
 *   default (flags 0):  [items][L][N], word [item][l][k] = c_k mod q_l in [0, q_l) for every limb of the context (|c_k| may exceed q_l).
 *   DPFHE_ENCODE_PLAIN: [items][N], c_k as two's-complement 64-bit words - what a client hands to Encryptor::encrypt(coeffs, 0, ct).
 *   DPFHE_ENCODE_NTT:   the residues, then the context's forward transform in place; invalid together with PLAIN.
 *   DPFHE_ENCODE_REAL:  the input is [items][n] doubles (imaginary parts zero) instead of [items][n] (re, im) pairs.
 * dpfhe_cencoder_create is a set-up call (one allocation, one copy: n twiddles, the slot -> position table, the limb constants).  The encoder is bound to
 *   `ctx`, which must outlive it; it is immutable afterwards and may be shared between threads.  Destroying null is safe.
 * dpfhe_encode_complex enqueues only (no allocation, no synchronise).  DPFHE_INVALID_ARGUMENT, with nothing written, on a null pointer, items 0, an unknown
 *   flag bit, PLAIN with NTT, a buffer not 16-byte aligned, out overlapping slots, a scale that is not finite and positive, or more than (2^31 - 1) / N
 *   items (one launch).  At log2_n >= 15 the transform is two kernels and parks its n intermediate complex words in row 0 of each item of d_out itself.
 * dpfhe_encode_complex_host: the same words on the host (no device, no context; moduli odd, >= 3 and < 2^60, log2_n in [8, 16]); rejects the same, and
 *   DPFHE_ENCODE_NTT as well.
 * dpfhe_decode_complex_host: z_i = m(xi^(3^i)) / scale for centred integer coefficients c_k [items][N] (what Decryptor::decrypt(ct, 0, out) returns), as
 *   [items][n] (re, im) pairs, or with DPFHE_ENCODE_REAL [items][n] real parts.  Bound: |z_i - exact| <= D = 8 log2(N) 2^-53 N max_k |c_k| / scale: the same
 *   levels run forwards on words c_j + i c_(j+n) of modulus <= sqrt(2) max|c|, a word after l levels being a sum of 2^l of them, so each level adds at most
 *   g sqrt(2) n max|c| = g N max|c| / sqrt(2); the conversion of |c_k| >= 2^53 and the division add u each.  DPFHE_INVALID_ARGUMENT on a null pointer,
 *   items 0, an unknown flag, log2_n outside [8, 16], overlapping buffers or a scale that is not finite and positive. */
typedef struct dpfhe_cencoder dpfhe_cencoder;
enum { DPFHE_ENCODE_REAL = 4u };
int dpfhe_cencoder_create(dpfhe_cencoder** out, dpfhe_ctx* ctx);
int dpfhe_cencoder_destroy(dpfhe_cencoder* enc);
int dpfhe_encode_complex(dpfhe_cencoder* enc, uint64_t* d_out, const double* d_slots, size_t items, double scale, uint32_t flags, void* stream);
int dpfhe_encode_complex_host(const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n, uint64_t* out, const double* slots, size_t items, double scale,
                              uint32_t flags);
int dpfhe_decode_complex_host(uint32_t log2_n, double* slots_out, const int64_t* coeffs, size_t items, double scale, uint32_t flags);

/* -- re-randomised results: noise polynomials from a SECRET seed, and a fresh public-key encryption of zero with a flooding error added to result
 * ciphertexts before they leave the server (order: evaluate -> dpfhe_rerandomize -> dpfhe_compact).
 * Definition.  noise(seed, item, stream_id, kind, param) is a polynomial of N SIGNED INTEGERS v_k; every limb of the output holds the same integer as its
 *   canonical residue v_k mod q_limb in [0, q_limb).  Coefficient k takes the ChaCha20 block (RFC 8439 section 2.3) with key = the 32-byte seed (8
 *   little-endian words), 32-bit block counter k >> 1 and nonce = (u32 item, u32 stream_id, u32 0x6b73616d), and of that block the output words
 *   8 (k & 1) .. 8 (k & 1) + 7 read as ONE 256-bit little-endian integer X.  (The third nonce word keeps these streams apart from expand(seed, item, limb,
 *   component), component < 3, even if a caller misuses one seed for both.)
 *     DPFHE_NOISE_TERNARY:  v = floor(3 (X mod 2^64) / 2^64) - 1                                   bias at most 2^-63 per coefficient, no rejection
 *     DPFHE_NOISE_CBD21:    v = popcount(X & 0x1fffff) - popcount((X >> 21) & 0x1fffff)             centred binomial, eta = 21: sigma = 3.24, |v| <= 21
 *     DPFHE_NOISE_FLOOD:    v = (X mod 2^(f + 1)) - 2^f,  f = param, 1 <= f <= 250                  exactly uniform on [-2^f, 2^f)
 *   The words do not depend on the limbs' arithmetic classes.  The seed is SECRET: it is a kernel argument and is never written to memory or to a
 *   stream.  One seed must never serve two calls: equal masks would make the difference of two results equal the difference of their inputs.
 * dpfhe_sample_noise: component `comp` of items 0 .. batch-1 of d_out [batch][comps][L][N] = noise(seed, first_item + b, stream_id, kind, param), or
 *   += noise mod q_limb with DPFHE_NOISE_ADD; every other word is untouched.  Enqueues only (no allocation, no synchronise).  DPFHE_INVALID_ARGUMENT,
 *   nothing written, on a null pointer, batch 0, a misaligned buffer, kind > 2, f outside [1, 250], comp >= comps, an unknown flag bit,
 *   first_item + batch > 2^32, or a batch too large for one launch.  param is ignored for the other two kinds.
 * dpfhe_sample_noise_host: the same words on the host (no device, no context; moduli odd, >= 3 and < 2^60, log2_n in [8, 16]).
 * dpfhe_rerandomize: in place on `batch` 2-component coefficient-domain ciphertexts d_ct2 [batch][2][L][N]; d_pk = [2][L][N], NTT domain (a public key
 *   (-(a s) + e, a)); d_work: 3 batch L N words of scratch.  Word for word, with item = first_item + b:
 *       u  = noise(seed, item, 0, TERNARY)           u^ = NTT(u)
 *       e0 = noise(seed, item, 2, FLOOD, flood_bits)
 *       e1 = noise(seed, item, 1, CBD21)
 *       c0 += INTT(pk0 (.) u^) + e0                   c1 += INTT(pk1 (.) u^) + e1            (mod every q_limb)
 *   Enqueues only (no allocation, no synchronise), every log2_n and limb class.  DPFHE_INVALID_ARGUMENT, nothing written, on a null pointer, batch 0,
 *   a misaligned buffer, d_work / d_ct2 / d_pk overlapping, first_item + batch > 2^32, or flood_bits outside [1, min(250, floor(log2 Q) - 3)] (the mask
 *   alone would wrap; the entry does not know the plaintext modulus - Rerandomizer in fhe.hpp applies the bound that leaves a decryptable result).
 *   Three-component inputs are out of scope: relinearise first.  Nothing is claimed against malformed input ciphertexts. */
enum { DPFHE_NOISE_TERNARY = 0u, DPFHE_NOISE_CBD21 = 1u, DPFHE_NOISE_FLOOD = 2u };
enum { DPFHE_NOISE_ADD = 1u };
int dpfhe_sample_noise(dpfhe_ctx* ctx, uint64_t* d_out, size_t batch, size_t comps, uint32_t comp, uint32_t kind, uint32_t param, uint32_t stream_id,
                       const uint8_t seed[32], uint32_t first_item, uint32_t flags, void* stream);
int dpfhe_sample_noise_host(const uint64_t* moduli, uint32_t n_limbs, uint32_t log2_n, uint64_t* out, size_t batch, size_t comps, uint32_t comp,
                            uint32_t kind, uint32_t param, uint32_t stream_id, const uint8_t seed[32], uint32_t first_item, uint32_t flags);
int dpfhe_rerandomize(dpfhe_ctx* ctx, uint64_t* d_ct2, const uint64_t* d_pk, size_t batch, uint32_t flood_bits, const uint8_t seed[32],
                      uint32_t first_item, uint64_t* d_work, void* stream);

const char* dpfhe_strerror(int code);
/* text of the last HIP/RCCL failure on the calling thread ("" if none) */
const char* dpfhe_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* DPFHE_H */
