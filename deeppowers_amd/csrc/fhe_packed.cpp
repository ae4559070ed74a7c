// fhe_packed.cpp - the facade's packed encrypted layers over the slot encodings and the hybrid key switcher: PackedLinear, ApproxPackedLinear,
// PackedSelect, PackedTransformerBlock.  Part of libdpfhe_api.so (fhe_api.cpp names the other units).
#include <algorithm>
#include <chrono>
#include <cmath>

#include "fhe_internal.h"

namespace deeppowers {
namespace fhe {

using namespace detail;

// ---- N3: packed matrix-vector product (diagonal method, baby-step / giant-step) -------------------------------------------
constexpr int kBabyShiftDefault = 1;

namespace {

// What the exact and the approximate layer share: the geometry of the diagonal method on slot rows of N / 2 slots, its rotation keys, the per-layer
// scratch and the body of apply() up to the level-L result - nothing in it depends on the plaintext space; only the encoding of the diagonals and of
// the bias does, and that stays with the two classes.
struct PackedCore {
    const Context* ctx = nullptr;
    HybridKeySwitcher* ks = nullptr;
    size_t out_dim = 0, in_dim = 0;
    size_t row = 0;      // slots per slot row, N / 2
    size_t rows = 2;     // slot rows of the encoding: 2 over Z_t, 1 for complex slots
    size_t n = 0;        // input period: the input vector repeats every n slots of a row (power of two >= in_dim)
    size_t m = 0;        // diagonals per pass = output period (n, or the padded out_dim of a wide-input layer)
    size_t tpc = 1;      // tokens per ciphertext: 2 = the two slot rows (complex slots: the real and imaginary parts) carry two tokens
    size_t copies = 0;   // independent n-slot windows that share the output blocks: rows * N / 2 / n, or those of ONE row when each row has its own token
    size_t blocks = 0;   // output row blocks of m rows
    size_t passes = 0;   // output ciphertexts
    bool replicate = false;   // one block: every window computes it (the output is again a periodic vector)
    size_t n1 = 0, n2 = 0;
    std::unique_ptr<Plaintext> diag;   // [passes][n2][n1] pre-rotated diagonals, NTT domain
    std::vector<uint32_t> baby_elts, giant_elts, fold_elts;
    // per-layer scratch, reused by every apply() (one caller at a time).  Terms over Q P live on the key switcher's extended context.
    std::unique_ptr<PolyBuffer> babies_qp, inner_qp, terms_qp, ksum_qp;
    std::unique_ptr<Ciphertext> rot, fold;
    std::vector<uint32_t> inner_elts;                            // element of inner sum (pass, i): 1 for i = 0, the giant step's otherwise
    size_t tokens = 0;                                           // scratch capacity in tokens

    // the split, the Galois elements (added to `ks` in the order baby, giant, fold) and the check that `ks` extends `ctx`; `galois(s)` = 3^s mod 2N
    template <class Galois>
    void plan(const char* who, const Context& c, HybridKeySwitcher& k, size_t out_d, size_t in_d, size_t slot_rows, size_t tokens_per_ciphertext, Galois galois) {
        const std::string name(who);
        if (tokens_per_ciphertext != 1 && tokens_per_ciphertext != 2) throw Exception(ErrorCode::INVALID_ARGUMENT, name + ": one or two tokens per ciphertext");
        if (out_d == 0 || in_d == 0) throw Exception(ErrorCode::INVALID_ARGUMENT, name + ": empty matrix");
        auto pow2 = [](size_t v) { size_t x = 1; while (x < v) x <<= 1; return x; };
        ctx = &c; ks = &k; out_dim = out_d; in_dim = in_d;
        row = c.params().n() / 2; rows = slot_rows;
        n = pow2(in_dim) < 2 ? 2 : pow2(in_dim);
        if (n > row) throw Exception(ErrorCode::INVALID_ARGUMENT, name + ": in_dim (padded to a power of two) must be <= N/2");
        tpc = tokens_per_ciphertext;
        copies = (tpc == 2 ? row : rows * row) / n;
        const size_t mo = pow2(out_dim) < 2 ? 2 : pow2(out_dim);
        m = mo < n ? mo : n;                                    // wide-input layer: only m wrapped diagonals, folded afterwards
        blocks = (out_dim + m - 1) / m;
        replicate = blocks == 1;
        passes = replicate ? 1 : (blocks + copies - 1) / copies;
        size_t b = 1;
        while (b * b < m) b <<= 1;
        // A hoisted baby step (gathers + key inner products, no transform) costs about a third of a giant step (Ld transforms per limb + its
        // share of the inverse transform and the division by P), so the split leans towards baby steps: n1 = 2 sqrt(m) when m allows.
        int shift = kBabyShiftDefault;
        // (the split sweep behind this default: profiles/r03_bsgs_split_sweep.txt)
        for (; shift > 0 && b * 2 < m; --shift) b <<= 1;
        for (; shift < 0 && b > 2; ++shift) b >>= 1;
        n1 = b; n2 = m / n1;
        for (size_t j = 1; j < n1; ++j) baby_elts.push_back(galois((int)j));
        for (size_t i = 1; i < n2; ++i) giant_elts.push_back(galois((int)(i * n1)));
        for (size_t sft = m; sft < n; sft <<= 1) fold_elts.push_back(galois((int)sft));
        for (uint32_t g : baby_elts) k.add_galois_element(g);
        for (uint32_t g : giant_elts) k.add_galois_element(g);
        for (uint32_t g : fold_elts) k.add_galois_element(g);
        const FheParams &p = c.params(), &pe = k.extended_context().params();
        if (pe.log2_n != p.log2_n || pe.n_limbs() != p.n_limbs() + 1 || !std::equal(p.moduli.begin(), p.moduli.end(), pe.moduli.begin()))
            throw Exception(ErrorCode::INVALID_ARGUMENT, name + ": the key switcher was built for another context");
    }
    // after the diagonals: the inner sums' elements
    void finish_plan() {
        for (size_t pass = 0; pass < passes; ++pass) {
            inner_elts.push_back(1u);
            inner_elts.insert(inner_elts.end(), giant_elts.begin(), giant_elts.end());
        }
    }

    void ensure_tokens(size_t T) {
        if (T <= tokens) return;
        const Context& ext = ks->extended_context();
        babies_qp.reset(new PolyBuffer(ext, n1 * T, 2, true));                      // [n1][T]: P rot_j(x_t) + key-switching terms, NTT domain
        inner_qp.reset(new PolyBuffer(ext, passes * n2 * T, 2, true));              // [passes * n2][T]
        rot.reset(new Ciphertext(*ctx, 2, passes * n2 * T));                        // the inner sums, rotated by their giant step, divided by P
        if (n2 > 1) {
            terms_qp.reset(new PolyBuffer(ext, (n2 - 1) * T, 2, true));             // key inner products of one output ciphertext's giant steps
            ksum_qp.reset(new PolyBuffer(ext, T, 2, true));
        }
        if (!fold_elts.empty()) fold.reset(new Ciphertext(*ctx, 2, T));             // the block sums before the fold
        tokens = T;
    }

    // which output row a slot of pass `pass` holds (or npos); slot < rows * N / 2
    size_t row_of_slot(size_t pass, size_t slot) const {
        const size_t r = slot % row, rho = slot / row;
        const size_t c = r / n + (tpc == 2 ? 0 : rho * (row / n));
        const size_t b = replicate || m < n ? 0 : pass * copies + c;
        const size_t R = b * m + r % m;
        return R < out_dim ? R : (size_t)-1;
    }
    // Pre-rotated diagonals.  The product of giant step i lands on output slot r = r' - i n1 (row rotation), so position r' of
    // diagonal (i, j) carries the weight of the output row that slot r holds and of input index (r + k) mod n, k = i n1 + j.
    // -> the index into W of what slot `slot` (position r' of its row) of that diagonal holds, or npos for a zero
    size_t diag_weight(size_t pass, size_t i, size_t j, size_t slot) const {
        const size_t rho = slot / row, rp = slot % row, k = i * n1 + j;
        const size_t r = (rp + row - (i * n1) % row) % row;
        const size_t R = row_of_slot(pass, rho * row + r), col = (r + k) % n;
        return (R != (size_t)-1 && col < in_dim) ? R * in_dim + col : (size_t)-1;
    }

    // x: T items on ctx -> sums: passes * T items on ctx (output ciphertext o of token t at item o * T + t), 2 components, coefficient domain, L limbs
    void run(const Ciphertext& x, Ciphertext& y_ct, Stream* s) {
        const size_t T = x.batch();
        uint64_t* y = y_ct.data();
        const FheParams& p = ctx->params();
        const size_t ct_words = 2 * p.n_limbs() * p.n();
        hipStream_t hs = static_cast<hipStream_t>(s);
        dpfhe_ctx* he = handle_of(ks->extended_context());
        // Layout of every intermediate: [rotation or diagonal index][token][component] - the token index sits where the plaintext
        // matvec sees "more components", so keys and diagonals are read once for all tokens.
        // baby steps: P rot_j(x_t) + key-switching term, j < n1, all tokens, ONE hoisted pass; they stay in the NTT domain over Q P
        ks->rotate_hoisted_qp(x, 0, T, baby_elts, *babies_qp, 0, s);
        // inner sums of all giant steps of all output ciphertexts of all tokens: ONE matrix-vector product over the pre-rotated diagonals
        check(dpfhe_matvec_plain_multi(he, inner_qp->data(), diag->data(), babies_qp->data(), passes * n2, n1, T, s), "dpfhe_matvec_plain_multi");
        // back to the coefficient domain, the giant step's automorphism applied by the transform's loads; then the ONE division by P
        // the baby steps and the plaintext products share
        check(dpfhe_ntt_inv_galois(he, inner_qp->data(), inner_qp->data(), T * 2, inner_elts.data(), passes * n2, s), "dpfhe_ntt_inv_galois");
        Ciphertext& rt = *rot;
        check(dpfhe_rescale(he, rt.data(), inner_qp->data(), passes * n2 * T * 2, s), "dpfhe_rescale");
        rt.set_ntt(false);
        // giant steps: key inner products of the rotated inner sums (i >= 1), summed over Q P; one inverse transform and one
        // division by P per output ciphertext, which also adds the c0 parts and the un-rotated inner sum
        uint64_t* sums = fold_elts.empty() ? y : fold->data();   // wide-input layer: the block sum is folded below before it becomes y
        if (n2 > 1) {
            for (size_t pass = 0; pass < passes; ++pass) {
                const size_t base = pass * n2 * T;
                ks->switch_key_qp(rt, base + T, giant_elts, T, *terms_qp, 0, s);
                check(dpfhe_reduce_sum(he, ksum_qp->data(), terms_qp->data(), n2 - 1, 2 * T, s), "dpfhe_reduce_sum");
                check(dpfhe_ntt_inv(he, ksum_qp->data(), T * 2, s), "dpfhe_ntt_inv");
                check(dpfhe_rescale_bsgs(he, sums + pass * T * ct_words, ksum_qp->data(), rt.data() + base * ct_words, n2, T, s), "dpfhe_rescale_bsgs");
            }
        } else {
            hip_check(hipMemcpyAsync(sums, rt.data(), passes * T * ct_words * sizeof(uint64_t), hipMemcpyDeviceToDevice, hs), "hipMemcpyAsync");
        }
        // wide input (m < n): slot r holds the partial sum over input indices congruent to r + k; fold the n/m windows together
        // (one rotate-and-add ladder: the words of a grouped rotation and an addition per step, dpfhe_rotate_add_hybrid)
        if (!fold_elts.empty()) {
            fold->set_ntt(false);
            ks->rotate_add_range(*fold, 0, T, fold_elts, y_ct, 0, s);
        }
    }
};

}  // namespace

class PackedLinear::Impl : public PackedCore {
public:
    const BatchEncoder* enc = nullptr;
    std::unique_ptr<ExactPlaintext> bias;   // [passes][N]: bias[R] on every slot that holds output row R, or null
    double encode_s = 0;                    // wall time the constructor spent building and encoding the diagonals and the bias (device work included)
};

PackedLinear::PackedLinear(const Context& ctx, const BatchEncoder& enc, HybridKeySwitcher& ks, const uint64_t* W, size_t d)
    : PackedLinear(ctx, enc, ks, W, d, d) {
    if (d < 2 || (d & (d - 1))) throw Exception(ErrorCode::INVALID_ARGUMENT, "PackedLinear: d must be a power of two dividing N/2");
}

PackedLinear::PackedLinear(const Context& ctx, const BatchEncoder& enc, HybridKeySwitcher& ks, const uint64_t* W, size_t out_dim, size_t in_dim, size_t tokens_per_ciphertext)
    : PackedLinear(ctx, enc, ks, W, out_dim, in_dim, tokens_per_ciphertext, nullptr) {}

PackedLinear::PackedLinear(const Context& ctx, const BatchEncoder& enc, HybridKeySwitcher& ks, const uint64_t* W, size_t out_dim, size_t in_dim, size_t tokens_per_ciphertext,
                           const uint64_t* bias)
    : impl_(new Impl) {
    const FheParams& p = ctx.params();
    const size_t N = p.n(), L = p.n_limbs();
    if (!W) throw Exception(ErrorCode::INVALID_ARGUMENT, "PackedLinear: empty matrix");
    if (tokens_per_ciphertext != 1 && tokens_per_ciphertext != 2) throw Exception(ErrorCode::INVALID_ARGUMENT, "PackedLinear: one or two tokens per ciphertext");
    if (enc.slot_count() != N) throw Exception(ErrorCode::INVALID_ARGUMENT, "PackedLinear: encoder and context disagree on N");
    Impl& I = *impl_;
    I.enc = &enc;
    const uint64_t t = enc.plain_modulus();
    // (the weights are looked at only after the keys exist, as before: a refused matrix leaves the key switcher with the layer's elements)
    I.plan("PackedLinear", ctx, ks, out_dim, in_dim, 2, tokens_per_ciphertext, [&](int s) { return enc.galois_element(s); });
    const size_t n1 = I.n1;
    for (size_t i = 0; i < out_dim * in_dim; ++i)
        if (W[i] >= t) throw Exception(ErrorCode::INVALID_ARGUMENT, "PackedLinear: weight >= plaintext modulus");
    if (bias)
        for (size_t i = 0; i < out_dim; ++i)
            if (bias[i] >= t) throw Exception(ErrorCode::INVALID_ARGUMENT, "PackedLinear: bias >= plaintext modulus");

    // The diagonals (PackedCore::diag_weight) are multiplied with terms over Q P (the division by P comes after the sum), so they are encoded over
    // all limbs of the key switcher's extended context.
    const Context& ext = ks.extended_context();
    const size_t Le = L + 1;
    I.diag.reset(new Plaintext(ext, I.passes * I.n2 * n1, /*is_ntt=*/false));
    // the slot vectors are built here as 32-bit values and encoded on the device: inverse transform over Z_t, lift to the Le limbs and the forward
    // transform, one call per giant step's n1 diagonals (the words BatchEncoder::encode + lift_signed + transform_to_ntt gave)
    const auto encode_t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> slots(n1 * N);
    void* stage = nullptr;
    hip_check(hipSetDevice(ext.device_id()), "hipSetDevice");
    hip_check(hipMalloc(&stage, slots.size() * sizeof(uint32_t)), "hipMalloc");
    try {
        for (size_t pass = 0; pass < I.passes; ++pass) {
            for (size_t i = 0; i < I.n2; ++i) {
                for (size_t j = 0; j < n1; ++j)
                    for (size_t sl = 0; sl < N; ++sl) {
                        const size_t w = I.diag_weight(pass, i, j, sl);
                        slots[j * N + sl] = w != (size_t)-1 ? (uint32_t)W[w] : 0u;
                    }
                // the copy is ordered behind the previous encode on the null stream; the host builds the next vectors while the device encodes these
                uint32_t* d_slots = static_cast<uint32_t*>(stage);
                hip_check(hipMemcpy(d_slots, slots.data(), slots.size() * sizeof(uint32_t), hipMemcpyHostToDevice), "hipMemcpy H2D");
                enc.encode_device_words(ext, d_slots, n1, I.diag->data() + ((pass * I.n2 + i) * n1) * Le * N, DPFHE_ENCODE_NTT, nullptr);
            }
        }
        hip_check(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
    } catch (...) {
        (void)hipFree(stage);
        throw;
    }
    (void)hipFree(stage);
    I.diag->set_ntt(true);
    I.finish_plan();
    // the bias: one slot vector per output ciphertext, in the layout the output itself has (row_of_slot - so also the replicated, folded and two-token ones)
    if (bias) {
        std::vector<uint32_t> bslots(I.passes * N);
        for (size_t pass = 0; pass < I.passes; ++pass)
            for (size_t sl = 0; sl < N; ++sl) {
                const size_t R = I.row_of_slot(pass, sl);
                bslots[pass * N + sl] = R != (size_t)-1 ? (uint32_t)bias[R] : 0u;
            }
        I.bias.reset(new ExactPlaintext(ctx, t, I.passes));
        I.bias->set_slots_device(enc, bslots.data());
    }
    I.encode_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - encode_t0).count();
    I.ensure_tokens(1);
    ext.synchronize();
}
bool PackedLinear::has_bias() const { return impl_->bias != nullptr; }
double PackedLinear::encode_seconds() const { return impl_->encode_s; }
PackedLinear::~PackedLinear() = default;
size_t PackedLinear::dim() const { return impl_->m; }
size_t PackedLinear::in_dim() const { return impl_->in_dim; }
size_t PackedLinear::out_dim() const { return impl_->out_dim; }
size_t PackedLinear::input_period() const { return impl_->n; }
size_t PackedLinear::output_ciphertexts() const { return impl_->passes; }
size_t PackedLinear::baby_steps() const { return impl_->n1; }
size_t PackedLinear::giant_steps() const { return impl_->n2; }
size_t PackedLinear::key_switches_per_apply() const {
    return impl_->baby_elts.size() + impl_->passes * impl_->giant_elts.size() + impl_->fold_elts.size();
}

void PackedLinear::pack_input(const uint64_t* x, uint64_t* slots) const {
    const size_t N = impl_->enc->slot_count();
    for (size_t s = 0; s < N; ++s) {
        const size_t c = (s % (N / 2)) % impl_->n;
        slots[s] = c < impl_->in_dim ? x[c] : 0;
    }
}
size_t PackedLinear::tokens_per_ciphertext() const { return impl_->tpc; }
void PackedLinear::pack_input_rows(const uint64_t* x0, const uint64_t* x1, uint64_t* slots) const {
    const size_t N = impl_->enc->slot_count(), row = N / 2;
    for (size_t s = 0; s < N; ++s) {
        const size_t c = (s % row) % impl_->n;
        slots[s] = c < impl_->in_dim ? (s < row ? x0[c] : x1[c]) : 0;
    }
}
void PackedLinear::unpack_output_rows(const uint64_t* slots, uint64_t* y0, uint64_t* y1) const {
    const size_t N = impl_->enc->slot_count(), row = N / 2;
    for (size_t rho = 0; rho < 2; ++rho) {
        std::vector<char> seen(impl_->out_dim, 0);
        uint64_t* y = rho ? y1 : y0;
        for (size_t pass = 0; pass < impl_->passes; ++pass)
            for (size_t s = rho * row; s < (rho + 1) * row; ++s) {
                const size_t R = impl_->row_of_slot(pass, s);
                if (R != (size_t)-1 && !seen[R]) { y[R] = slots[pass * N + s]; seen[R] = 1; }
            }
    }
}
void PackedLinear::unpack_output(const uint64_t* slots, uint64_t* y) const {
    const size_t N = impl_->enc->slot_count();
    std::vector<char> seen(impl_->out_dim, 0);
    for (size_t pass = 0; pass < impl_->passes; ++pass)
        for (size_t s = 0; s < N; ++s) {
            const size_t R = impl_->row_of_slot(pass, s);
            if (R != (size_t)-1 && !seen[R]) { y[R] = slots[pass * N + s]; seen[R] = 1; }
        }
}

void PackedLinear::apply(const Ciphertext& x, Ciphertext& y, Stream* s) const {
    Impl& I = *impl_;
    const size_t T = x.batch();
    if (x.is_ntt() || x.size() != 2 || T == 0 || y.size() != 2 || y.batch() != I.passes * T)
        throw Exception(ErrorCode::INVALID_ARGUMENT, "PackedLinear::apply: T 2-component coefficient-domain ciphertexts in, output_ciphertexts() * T out");
    I.ensure_tokens(T);   // (re)allocates only when a larger batch than ever before arrives
    I.run(x, y, s);
    dpfhe_ctx* h = handle_of(*I.ctx);
    // + bias: output ciphertext o of every token (item o * T + t) takes bias item o
    if (I.bias)
        check(dpfhe_add_plain_scaled(h, y.data(), y.data(), I.bias->data(), I.passes * T, 2, I.passes, I.bias->plain_modulus(), 0, s), "dpfhe_add_plain_scaled");
    y.set_ntt(false);
    // enqueue only: the scratch belongs to the layer, the caller synchronises (Context::synchronize) before reading y
}

// ---- the approximate (CKKS-style) layer: real weights on the one row of N / 2 complex slots, rescale, plaintext add ---------------------------
class ApproxPackedLinear::Impl : public PackedCore {
public:
    const Context* next = nullptr;
    const ComplexEncoder* enc = nullptr;
    double w_scale = 0, x_scale = 0, q_last = 0;
    double rho = 0;          // max_j q_j / P over the data limbs
    double w_max = 0;        // max |W_ij|
    double w_row1 = 0;       // max_R ||W_R||_1
    double b_max = 0;        // max |bias_R| (0 without a bias)
    std::unique_ptr<Plaintext> bias;    // on `next`: [passes] polynomials at output_scale(), coefficient domain, or null
    std::unique_ptr<Ciphertext> full;   // the level-L result before the rescale: passes * T items
    double encode_s = 0;
    void ensure(size_t T) {
        grow_scratch(full, passes * T, [&](size_t b) { return new Ciphertext(*ctx, 2, b); });
        ensure_tokens(T);
    }
};

ApproxPackedLinear::ApproxPackedLinear(const Context& ctx, const Context& next_ctx, const ComplexEncoder& enc, HybridKeySwitcher& ks, const double* W, size_t out_dim,
                                       size_t in_dim, double weight_scale, double input_scale, size_t tokens_per_ciphertext, const double* bias)
    : impl_(new Impl) {
    const FheParams& p = ctx.params();
    const size_t N = p.n(), L = p.n_limbs(), row = N / 2;
    if (!W || out_dim == 0 || in_dim == 0) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxPackedLinear: empty matrix");
    if (enc.slot_count() != row) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxPackedLinear: encoder and context disagree on N");
    if (!(weight_scale > 0) || !(input_scale > 0) || !std::isfinite(weight_scale) || !std::isfinite(input_scale))
        throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxPackedLinear: the scales must be finite and positive");
    if (L < 2) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxPackedLinear: no limb to rescale by");
    const FheParams pn = p.drop_last_limb();
    if (next_ctx.params().log2_n != pn.log2_n || next_ctx.params().moduli != pn.moduli || next_ctx.params().psi != pn.psi || next_ctx.device_id() != ctx.device_id())
        throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxPackedLinear: next_ctx must be a context on data_ctx.params().drop_last_limb(), on the same device");
    Impl& I = *impl_;
    I.next = &next_ctx; I.enc = &enc; I.w_scale = weight_scale; I.x_scale = input_scale; I.q_last = (double)p.moduli.back();
    const double out_scale = input_scale * weight_scale / I.q_last, clamp = std::ldexp(1.0, 62);
    for (size_t R = 0; R < out_dim; ++R) {
        double sum = 0;
        for (size_t c = 0; c < in_dim; ++c) {
            const double w = W[R * in_dim + c];
            if (!std::isfinite(w)) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxPackedLinear: a weight is not finite");
            sum += std::fabs(w);
            I.w_max = std::max(I.w_max, std::fabs(w));
        }
        I.w_row1 = std::max(I.w_row1, sum);
    }
    if (weight_scale * I.w_max >= clamp) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxPackedLinear: weight_scale * max|W| must stay below 2^62 (the encoder's clamp)");
    if (bias) {
        for (size_t R = 0; R < out_dim; ++R) {
            if (!std::isfinite(bias[R])) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxPackedLinear: a bias value is not finite");
            I.b_max = std::max(I.b_max, std::fabs(bias[R]));
        }
        if (out_scale * I.b_max * 2 >= clamp) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxPackedLinear: output_scale() * max|bias| must stay below 2^61");
    }
    // the geometry of PackedLinear on the ONE slot row: 3^s rotates it as it rotates the rows over Z_t, so both families share keys on one key switcher
    I.plan("ApproxPackedLinear", ctx, ks, out_dim, in_dim, 1, tokens_per_ciphertext, [&](int s) { return enc.galois_element(s); });
    const FheParams& pe = ks.extended_context().params();
    for (size_t l = 0; l < L; ++l) I.rho = std::max(I.rho, (double)p.moduli[l] / (double)pe.moduli.back());

    // the diagonals are real slot vectors at weight_scale, encoded over all limbs of the extended context, n1 per call
    const Context& ext = ks.extended_context();
    const size_t Le = L + 1, n1 = I.n1;
    I.diag.reset(new Plaintext(ext, I.passes * I.n2 * n1, /*is_ntt=*/false));
    const auto encode_t0 = std::chrono::steady_clock::now();
    std::vector<double> slots(std::max(n1 * row, bias ? I.passes * N : (size_t)0));
    double* stage = device_alloc<double>(ext.device_id(), slots.size());
    try {
        for (size_t pass = 0; pass < I.passes; ++pass)
            for (size_t i = 0; i < I.n2; ++i) {
                for (size_t j = 0; j < n1; ++j)
                    for (size_t sl = 0; sl < row; ++sl) {
                        const size_t w = I.diag_weight(pass, i, j, sl);
                        slots[j * row + sl] = w != (size_t)-1 ? W[w] : 0.0;
                    }
                // the copy is ordered behind the previous encode on the null stream; the host builds the next vectors while the device encodes these
                hip_check(hipMemcpy(stage, slots.data(), n1 * row * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy H2D");
                enc.encode_device_words(ext, stage, n1, weight_scale, I.diag->data() + ((pass * I.n2 + i) * n1) * Le * N, DPFHE_ENCODE_NTT | DPFHE_ENCODE_REAL, nullptr);
            }
        I.diag->set_ntt(true);
        I.finish_plan();
        // the bias: one vector of (re, im) slots per output ciphertext at output_scale(), in the layout the output has (row_of_slot); two tokens: b (1 + i)
        if (bias) {
            for (size_t pass = 0; pass < I.passes; ++pass)
                for (size_t sl = 0; sl < row; ++sl) {
                    const size_t R = I.row_of_slot(pass, sl);
                    const double b = R != (size_t)-1 ? bias[R] : 0.0;
                    slots[(pass * row + sl) * 2] = b;
                    slots[(pass * row + sl) * 2 + 1] = I.tpc == 2 ? b : 0.0;
                }
            hip_check(hipMemcpy(stage, slots.data(), I.passes * N * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy H2D");
            I.bias.reset(new Plaintext(next_ctx, I.passes, false));
            enc.encode_device(stage, I.passes, out_scale, *I.bias, /*to_ntt=*/false, /*real=*/false, nullptr);
        }
        hip_check(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
    } catch (...) {
        (void)hipFree(stage);
        throw;
    }
    (void)hipFree(stage);
    I.encode_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - encode_t0).count();
    I.ensure(1);
    ext.synchronize();
}
ApproxPackedLinear::~ApproxPackedLinear() = default;
bool ApproxPackedLinear::has_bias() const { return impl_->bias != nullptr; }
double ApproxPackedLinear::encode_seconds() const { return impl_->encode_s; }
double ApproxPackedLinear::output_scale() const { return impl_->x_scale * impl_->w_scale / impl_->q_last; }
size_t ApproxPackedLinear::dim() const { return impl_->m; }
size_t ApproxPackedLinear::in_dim() const { return impl_->in_dim; }
size_t ApproxPackedLinear::out_dim() const { return impl_->out_dim; }
size_t ApproxPackedLinear::input_period() const { return impl_->n; }
size_t ApproxPackedLinear::output_ciphertexts() const { return impl_->passes; }
size_t ApproxPackedLinear::baby_steps() const { return impl_->n1; }
size_t ApproxPackedLinear::giant_steps() const { return impl_->n2; }
size_t ApproxPackedLinear::tokens_per_ciphertext() const { return impl_->tpc; }
size_t ApproxPackedLinear::key_switches_per_apply() const {
    return impl_->baby_elts.size() + impl_->passes * impl_->giant_elts.size() + impl_->fold_elts.size();
}

void ApproxPackedLinear::pack_input_pair(const double* xa, const double* xb, std::complex<double>* slots) const {
    for (size_t s = 0; s < impl_->row; ++s) {
        const size_t c = s % impl_->n;
        slots[s] = c < impl_->in_dim ? std::complex<double>(xa[c], xb ? xb[c] : 0.0) : std::complex<double>(0.0, 0.0);
    }
}
void ApproxPackedLinear::pack_input(const double* x, std::complex<double>* slots) const { pack_input_pair(x, nullptr, slots); }
void ApproxPackedLinear::unpack_output_pair(const std::complex<double>* slots, double* ya, double* yb) const {
    std::vector<char> seen(impl_->out_dim, 0);
    for (size_t pass = 0; pass < impl_->passes; ++pass)
        for (size_t s = 0; s < impl_->row; ++s) {
            const size_t R = impl_->row_of_slot(pass, s);
            if (R == (size_t)-1 || seen[R]) continue;
            ya[R] = slots[pass * impl_->row + s].real();
            if (yb) yb[R] = slots[pass * impl_->row + s].imag();
            seen[R] = 1;
        }
}
void ApproxPackedLinear::unpack_output(const std::complex<double>* slots, double* y) const { unpack_output_pair(slots, y, nullptr); }
size_t ApproxPackedLinear::row_of_slot(size_t output_ciphertext, size_t slot) const {
    if (output_ciphertext >= impl_->passes || slot >= impl_->row) throw Exception(ErrorCode::INVALID_ARGUMENT, "ApproxPackedLinear::row_of_slot: index out of range");
    return impl_->row_of_slot(output_ciphertext, slot);
}

// the bound of include/deeppowers/fhe.hpp, term by term in that order
double ApproxPackedLinear::error_bound(double max_abs_input, double input_noise_bound) const {
    const Impl& I = *impl_;
    const FheParams& p = I.ctx->params();
    const BoundUnits bu(p.log2_n);
    const double N = bu.N, H = bu.H, u8 = bu.u8, two = I.tpc == 2 ? std::sqrt(2.0) : 1.0;
    const double Dx = I.x_scale, Dw = I.w_scale, Do = output_scale();
    const double K = keyswitch_term((double)p.n_limbs(), N, I.rho);
    const double X = max_abs_input * two, B = I.b_max * two, n = (double)I.n, n2 = (double)I.n2;
    const double G = N * (0.5 + u8 * Dw * I.w_max);                 // a diagonal's slot, off its weight
    const double S = N * input_noise_bound + N * K;                 // a baby step's slot, off Dx x
    const double products = Dw * I.w_row1 * S + Dx * X * n * G + n * G * S;
    const double e0 = n2 * H + (I.n2 > 1 ? (n2 - 1) * K + H : 0.0);
    const double windows = n / (double)I.m;                         // 2^F
    const double eF = windows * e0 + (windows - 1) * (K + H);
    double pre = (products + N * eF) / (Dx * Dw) + N * H / Do;
    if (I.bias) pre += N * (0.5 + u8 * Do * B) / Do;
    const double Z = I.w_row1 * X + B;
    return pre + u8 * N * (Z + pre);
}

void ApproxPackedLinear::apply(const Ciphertext& x, Ciphertext& y, Stream* s) const {
    Impl& I = *impl_;
    const size_t T = x.batch();
    const FheParams& p = I.ctx->params();
    const size_t poly = p.n_limbs() * p.n();
    if (x.is_ntt() || x.size() != 2 || T == 0 || x.words() != T * 2 * poly || y.size() != 2 || y.batch() != I.passes * T ||
        y.words() != I.passes * T * 2 * (poly - p.n()))
        throw Exception(ErrorCode::INVALID_ARGUMENT,
                        "ApproxPackedLinear::apply: T 2-component coefficient-domain ciphertexts on data_ctx in, output_ciphertexts() * T on next_ctx out");
    I.ensure(T);   // (re)allocates only when a larger batch than ever before arrives
    I.run(x, *I.full, s);                                          // level L, scale input_scale * weight_scale
    check(dpfhe_rescale(handle_of(*I.ctx), y.data(), I.full->data(), I.passes * T * 2, s), "dpfhe_rescale");
    // + bias: output ciphertext o of every token (item o * T + t) takes bias item o
    if (I.bias) check(dpfhe_add_plain(handle_of(*I.next), y.data(), y.data(), I.bias->data(), I.passes * T, 2, I.passes, 0, s), "dpfhe_add_plain");
    y.set_ntt(false);
    // enqueue only: the scratch belongs to the layer, the caller synchronises (Context::synchronize) before reading y
}

// ---- N3: hand-over between packed layers and the transformer block's linear skeleton ------------------------------------------
class PackedSelect::Impl {
public:
    const Context* ctx = nullptr;
    HybridKeySwitcher* ks = nullptr;
    size_t offset = 0, tpc = 1;
    uint32_t shift_elt = 0, swap_elt = 0;
    std::vector<uint32_t> spread_elts;          // right rotations by period, 2 period, ... up to half a slot row
    std::unique_ptr<Plaintext> mask;            // NTT domain: 1 on slots [0, length) of row 0, 0 elsewhere
    std::unique_ptr<Ciphertext> a, b;           // scratch, T items each
    size_t tokens = 0;
    void ensure(size_t T) {
        if (T <= tokens) return;
        a.reset(new Ciphertext(*ctx, 2, T));
        b.reset(new Ciphertext(*ctx, 2, T));
        tokens = T;
    }
};

PackedSelect::PackedSelect(const Context& ctx, const BatchEncoder& enc, HybridKeySwitcher& ks, size_t offset, size_t length, size_t period, size_t tokens_per_ciphertext) : impl_(new Impl) {
    if (tokens_per_ciphertext != 1 && tokens_per_ciphertext != 2) throw Exception(ErrorCode::INVALID_ARGUMENT, "PackedSelect: one or two tokens per ciphertext");
    const FheParams& p = ctx.params();
    const size_t N = p.n(), row = N / 2, L = p.n_limbs();
    if (enc.slot_count() != N || length == 0 || period < length || (period & (period - 1)) || period > row || offset + length > row)
        throw Exception(ErrorCode::INVALID_ARGUMENT, "PackedSelect: slice of slot row 0, period a power of two in [length, N/2]");
    Impl& I = *impl_;
    I.ctx = &ctx; I.ks = &ks; I.offset = offset; I.tpc = tokens_per_ciphertext;
    if (offset) { I.shift_elt = enc.galois_element((int)offset); ks.add_galois_element(I.shift_elt); }
    for (size_t sft = period; sft < row; sft <<= 1) { I.spread_elts.push_back(enc.galois_element(-(int)sft)); ks.add_galois_element(I.spread_elts.back()); }
    I.swap_elt = (uint32_t)(2 * N - 1);
    if (I.tpc == 1) ks.add_galois_element(I.swap_elt);
    std::vector<uint32_t> slots(N, 0);
    for (size_t i = 0; i < length; ++i) { slots[i] = 1; if (I.tpc == 2) slots[row + i] = 1; }   // (two tokens: the same slice of row 1)
    I.mask.reset(new Plaintext(ctx, 1, false));
    enc.encode_device(slots.data(), 1, *I.mask, /*to_ntt=*/true);
    I.ensure(1);
    ctx.synchronize();
}
PackedSelect::~PackedSelect() = default;
size_t PackedSelect::key_switches_per_apply() const { return (impl_->offset ? 1 : 0) + impl_->spread_elts.size() + (impl_->tpc == 1 ? 1 : 0); }

void PackedSelect::apply(const Ciphertext& x, Ciphertext& y, Stream* s) const {
    Impl& I = *impl_;
    const size_t T = x.batch();
    if (x.is_ntt() || x.size() != 2 || y.size() != 2 || y.batch() != T || T == 0)
        throw Exception(ErrorCode::INVALID_ARGUMENT, "PackedSelect::apply: T 2-component coefficient-domain ciphertexts in and out");
    I.ensure(T);
    dpfhe_ctx* h = handle_of(*I.ctx);
    Ciphertext &a = *I.a, &b = *I.b;
    const Ciphertext* cur = &x;
    if (I.offset) {   // slot offset + i -> slot i
        I.ks->apply_galois_grouped(x, 0, std::vector<uint32_t>(1, I.shift_elt), T, a, 0, s);
        cur = &a;
    }
    // mask: NTT, every polynomial times the (broadcast) mask in one launch, back
    check(dpfhe_ntt_fwd_oop(h, b.data(), cur->data(), T * 2, s), "dpfhe_ntt_fwd_oop");
    check(dpfhe_multiply_plain(h, b.data(), b.data(), I.mask->data(), T * 2, s), "dpfhe_multiply_plain");
    check(dpfhe_ntt_inv(h, b.data(), T * 2, s), "dpfhe_ntt_inv");
    b.set_ntt(false);
    // spread along the row: b += rot(b, -period), then -2 period, ...; then the other row
    Ciphertext* have = &b;
    Ciphertext* tmp = &a;
    auto rotate_add = [&](uint32_t g, Ciphertext& out) {
        I.ks->apply_galois_grouped(*have, 0, std::vector<uint32_t>(1, g), T, *tmp, 0, s);
        check(dpfhe_add(h, out.data(), have->data(), tmp->data(), T * 2, s), "dpfhe_add");
        out.set_ntt(false);
    };
    if (I.tpc == 1) {
        for (uint32_t g : I.spread_elts) rotate_add(g, *have);
        rotate_add(I.swap_elt, y);
    } else {   // two tokens per ciphertext: every row keeps its own token - spread inside the rows only, the last step writes y
        const FheParams& p = I.ctx->params();
        if (I.spread_elts.empty()) {
            hip_check(hipMemcpyAsync(y.data(), have->data(), T * 2 * p.n_limbs() * p.n() * sizeof(uint64_t), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(s)), "hipMemcpyAsync");
            y.set_ntt(false);
        } else {
            for (size_t i = 0; i + 1 < I.spread_elts.size(); ++i) rotate_add(I.spread_elts[i], *have);
            rotate_add(I.spread_elts.back(), y);
        }
    }
}

class PackedTransformerBlock::Impl {
public:
    const Context* ctx = nullptr;
    HybridKeySwitcher* ks = nullptr;
    size_t d = 0, h = 0;
    std::unique_ptr<PackedLinear> qkv, proj, up, down;
    std::unique_ptr<PackedSelect> take_v;
    std::unique_ptr<Ciphertext> st[5], o, u, us, dn;   // stages + scratch, T items each
    size_t tokens = 0;
    void ensure(size_t T) {
        if (T <= tokens) return;
        for (auto& c : st) c.reset(new Ciphertext(*ctx, 2, T));
        o.reset(new Ciphertext(*ctx, 2, T)); u.reset(new Ciphertext(*ctx, 2, T)); us.reset(new Ciphertext(*ctx, 2, T)); dn.reset(new Ciphertext(*ctx, 2, T));
        tokens = T;
    }
};

PackedTransformerBlock::PackedTransformerBlock(const Context& ctx, const BatchEncoder& enc, HybridKeySwitcher& ks, const uint64_t* W_qkv, const uint64_t* W_o,
                                               const uint64_t* W_up, const uint64_t* W_down, size_t d, size_t h)
    : PackedTransformerBlock(ctx, enc, ks, W_qkv, W_o, W_up, W_down, d, h, nullptr, nullptr, nullptr, nullptr) {}

PackedTransformerBlock::PackedTransformerBlock(const Context& ctx, const BatchEncoder& enc, HybridKeySwitcher& ks, const uint64_t* W_qkv, const uint64_t* W_o,
                                               const uint64_t* W_up, const uint64_t* W_down, size_t d, size_t h, const uint64_t* b_qkv, const uint64_t* b_o,
                                               const uint64_t* b_up, const uint64_t* b_down) : impl_(new Impl) {
    if (!W_qkv || !W_o || !W_up || !W_down || d == 0 || h == 0) throw Exception(ErrorCode::INVALID_ARGUMENT, "PackedTransformerBlock: null or empty matrix");
    Impl& I = *impl_;
    I.ctx = &ctx; I.ks = &ks; I.d = d; I.h = h;
    // the biases ride on the layers: b_v reaches `a` through the PackedSelect of the v third, b_up enters W_down's input with W_up h1
    I.qkv.reset(new PackedLinear(ctx, enc, ks, W_qkv, 3 * d, d, 1, b_qkv));
    I.proj.reset(new PackedLinear(ctx, enc, ks, W_o, d, d, 1, b_o));
    I.up.reset(new PackedLinear(ctx, enc, ks, W_up, h, d, 1, b_up));
    I.down.reset(new PackedLinear(ctx, enc, ks, W_down, d, h, 1, b_down));
    const size_t row = ctx.params().n() / 2;
    // the hand-overs below rely on: one output ciphertext per layer, outputs of the wide layers at slot r of row 0 (out >= period),
    // and W_down consuming a vector that fills a whole slot row
    if (I.qkv->output_ciphertexts() != 1 || I.up->output_ciphertexts() != 1 || I.down->output_ciphertexts() != 1 || I.proj->output_ciphertexts() != 1 ||
        3 * d < I.qkv->input_period() || 3 * d > row || h < I.up->input_period() || I.down->input_period() != row || I.proj->input_period() != I.qkv->input_period())
        throw Exception(ErrorCode::INVALID_ARGUMENT, "PackedTransformerBlock: needs 3 d <= N/2, h >= the padded d and the padded h = N/2 (GPT-2 small at N = 8192: d = 768, h = 3072)");
    I.take_v.reset(new PackedSelect(ctx, enc, ks, 2 * d, d, I.proj->input_period()));
    ks.add_galois_element((uint32_t)(2 * ctx.params().n() - 1));
    I.ensure(1);
}
PackedTransformerBlock::~PackedTransformerBlock() = default;
size_t PackedTransformerBlock::hidden() const { return impl_->d; }
size_t PackedTransformerBlock::inner() const { return impl_->h; }
size_t PackedTransformerBlock::key_switches_per_token() const {
    const Impl& I = *impl_;
    return I.qkv->key_switches_per_apply() + I.take_v->key_switches_per_apply() + I.proj->key_switches_per_apply() + I.up->key_switches_per_apply() + 1 +
           I.down->key_switches_per_apply();
}
void PackedTransformerBlock::pack_input(const uint64_t* x, uint64_t* slots) const { impl_->qkv->pack_input(x, slots); }
void PackedTransformerBlock::unpack_output(const uint64_t* slots, uint64_t* y) const { impl_->down->unpack_output(slots, y); }
const Ciphertext& PackedTransformerBlock::stage(int index) const {
    if (index < 0 || index > 4 || !impl_->st[index]) throw Exception(ErrorCode::INVALID_ARGUMENT, "PackedTransformerBlock::stage: index in [0, 4]");
    return *impl_->st[index];
}

void PackedTransformerBlock::apply(const Ciphertext& x, Ciphertext& y, Stream* s) const {
    Impl& I = *impl_;
    const size_t T = x.batch();
    if (x.is_ntt() || x.size() != 2 || y.size() != 2 || y.batch() != T || T == 0)
        throw Exception(ErrorCode::INVALID_ARGUMENT, "PackedTransformerBlock::apply: T 2-component coefficient-domain ciphertexts in and out");
    I.ensure(T);
    dpfhe_ctx* h = handle_of(*I.ctx);
    const FheParams& p = I.ctx->params();
    const size_t words = T * 2 * p.n_limbs() * p.n();
    Ciphertext &qkv = *I.st[0], &a = *I.st[1], &h1 = *I.st[2], &u2 = *I.st[3], &h2 = *I.st[4];
    I.qkv->apply(x, qkv, s);                                   // q | k | v at slots 0 .. 3d-1 of row 0 (gpt_model.cpp:793)
    I.take_v->apply(qkv, a, s);                                // attention over one position: the output is v; re-packed as a layer input
    I.proj->apply(a, *I.o, s);                                 // attention-output projection
    check(dpfhe_add(h, h1.data(), x.data(), I.o->data(), T * 2, s), "dpfhe_add");   // residual
    h1.set_ntt(false);
    I.up->apply(h1, *I.u, s);                                  // FFN up (gpt_model.cpp:848): outputs at slot r of row 0
    I.ks->apply_galois_grouped(*I.u, 0, std::vector<uint32_t>(1, (uint32_t)(2 * p.n() - 1)), T, *I.us, 0, s);   // row swap
    check(dpfhe_add(h, u2.data(), I.u->data(), I.us->data(), T * 2, s), "dpfhe_add");                          // both rows: W_down's input packing
    u2.set_ntt(false);
    I.down->apply(u2, *I.dn, s);                               // FFN down
    check(dpfhe_add(h, h2.data(), h1.data(), I.dn->data(), T * 2, s), "dpfhe_add");   // residual
    h2.set_ntt(false);
    hip_check(hipMemcpyAsync(y.data(), h2.data(), words * sizeof(uint64_t), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(s)), "hipMemcpyAsync");
    y.set_ntt(false);
}

}  // namespace fhe
}  // namespace deeppowers
