// GPU test of the Stream* argument of the C++ facade (include/deeppowers/fhe.hpp): every method that promises "enqueues on `stream`" is run on ONE
// non-blocking stream S behind the gate of tests/cpp/stream_gate.hip, with the protocol of Gate::gated (tests/cpp/facade_test.h): the warm-up and the gate
// run on zero inputs (an encryption of zero in the input ciphertext buffer), the real inputs arrive and the outputs are wiped on S behind the gate, the call
// must return with the gate's event pending and within G / 4.  Here, after S has run, the result decrypts to the plaintext computation (or, for the
// word-level Evaluator methods, equals the words of the same call on the idle null stream).
// The three methods that synchronise `stream` on purpose (Evaluator::apply_galois, HybridKeySwitcher::relinearize / apply_galois) are held to their
// values, and to returning only after S has run (they waited for S).
// Built and run by tests/test_gpu_stream_contract.py (-m gpu); argv[1] = G in seconds.  Exit code 0 = all checks passed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#define FACADE_TEST_GATE
#include "dpfhe.h"
#include "facade_test.h"

using namespace deeppowers::fhe;
using namespace facade_test;

static Lcg rnd{2024};
static uint64_t small8() { return rnd.small8(); }

// everything at N = 1024 on five data limbs + a special prime (the small ring packed_rect(10) of test_fhe_api.cpp uses)
struct Rig {
    uint64_t special = 0, special_psi = 0;
    FheParams p;
    Context ctx;
    Evaluator ev;
    KeyGenerator kg;
    Encryptor enc;
    Decryptor dec;
    BatchEncoder be;
    HybridKeySwitcher hks;
    size_t n;
    Gate gate;   // the non-blocking stream S, the gate G and the tally of the gated calls
    explicit Rig(double G) : p(ring(10, 5, special, special_psi)), ctx(p, 0), ev(ctx), kg(ctx, TestSeed{81}), enc(ctx, kg.secret_key(), TestSeed{82}), dec(ctx, kg.secret_key()),
            be(ctx, T_MOD), hks(ctx, kg.secret_key(), special, special_psi, TestSeed{83}), n(p.n()), gate(G) {}
    // C ciphertexts of the given slot vectors, and C encryptions of zero
    void encrypt_slots(const std::vector<uint64_t>& slots, Ciphertext& real, Ciphertext& zero) {
        const size_t C = real.batch();
        std::vector<int64_t> cx(C * n), z(C * n, 0);
        for (size_t c = 0; c < C; ++c) be.encode(&slots[c * n], &cx[c * n]);
        enc.encrypt_exact(cx.data(), T_MOD, real);
        enc.encrypt_exact(z.data(), T_MOD, zero);
    }
    std::vector<uint64_t> decrypt_slots(const Ciphertext& ct) {
        std::vector<uint64_t> dm(ct.batch() * n), got(ct.batch() * n);
        dec.decrypt_exact(ct, T_MOD, dm.data());
        for (size_t i = 0; i < ct.batch(); ++i) be.decode(&dm[i * n], &got[i * n]);
        return got;
    }
};

// ---- PackedLinear::apply: ragged 77 x 24, folded 12 x 100, biased, one and two tokens per ciphertext, 3 ciphertexts -----------------------------------------
static void packed_linear(Rig& r) {
    const size_t n = r.n, C = 3;
    // out, in, tokens per ciphertext, bias; {1, 64}: one diagonal - no giant step, the inner sum reaches y by a hipMemcpyAsync
    const size_t shapes[][4] = {{77, 24, 1, 0}, {12, 100, 1, 0}, {77, 24, 1, 1}, {64, 64, 2, 1}, {12, 100, 2, 0}, {1, 64, 1, 0}};
    for (auto& sh : shapes) {
        const size_t out = sh[0], in = sh[1], tpc = sh[2], T = C * tpc;
        std::vector<uint64_t> W(out * in), bias(out), x(T * in), slots(C * n);
        for (auto& v : W) v = small8();
        for (auto& v : bias) v = rnd(T_MOD);
        for (auto& v : x) v = 1 + rnd(100);
        PackedLinear lin(r.ctx, r.be, r.hks, W.data(), out, in, tpc, sh[3] ? bias.data() : nullptr);
        const size_t outs = lin.output_ciphertexts();
        for (size_t c = 0; c < C; ++c) {
            if (tpc == 1) lin.pack_input(&x[c * in], &slots[c * n]);
            else lin.pack_input_rows(&x[2 * c * in], &x[(2 * c + 1) * in], &slots[c * n]);
        }
        Ciphertext cx(r.ctx, 2, C), real(r.ctx, 2, C), zero(r.ctx, 2, C), cy(r.ctx, 2, outs * C);
        r.encrypt_slots(slots, real, zero);
        char what[96];
        std::snprintf(what, sizeof what, "PackedLinear::apply %zu x %zu, %zu per ciphertext%s", out, in, tpc, sh[3] ? ", biased" : "");
        r.gate.gated(what, {late(cx, zero, real)}, {out_of(cy)}, [&](Stream* s) { lin.apply(cx, cy, s); });
        const std::vector<uint64_t> got = r.decrypt_slots(cy);
        std::vector<uint64_t> tok(outs * n), y0(out), y1(out);
        size_t bad = 0;
        for (size_t c = 0; c < C; ++c) {
            for (size_t o = 0; o < outs; ++o) std::memcpy(&tok[o * n], &got[(o * C + c) * n], n * 8);
            if (tpc == 1) lin.unpack_output(tok.data(), y0.data());
            else lin.unpack_output_rows(tok.data(), y0.data(), y1.data());
            bad += y0 != affine(W, sh[3] ? bias.data() : nullptr, out, in, &x[tpc * c * in], T_MOD);
            if (tpc == 2) bad += y1 != affine(W, sh[3] ? bias.data() : nullptr, out, in, &x[(2 * c + 1) * in], T_MOD);
        }
        if (bad) std::printf("  %s: %zu wrong tokens\n", what, bad);
        CHECK(bad == 0);
    }
}

// ---- PackedSelect::apply: a slice at a non-zero offset, one and two tokens per ciphertext ---------------------------------------------------------------
static void packed_select(Rig& r) {
    const size_t n = r.n, row = n / 2, C = 3, offset = 40, length = 20, period = 32;
    for (size_t tpc : {(size_t)1, (size_t)2}) {
        PackedSelect sel(r.ctx, r.be, r.hks, offset, length, period, tpc);
        std::vector<uint64_t> slots(C * n);
        for (auto& v : slots) v = 1 + rnd(T_MOD - 1);
        Ciphertext cx(r.ctx, 2, C), real(r.ctx, 2, C), zero(r.ctx, 2, C), cy(r.ctx, 2, C);
        r.encrypt_slots(slots, real, zero);
        r.gate.gated(tpc == 1 ? "PackedSelect::apply" : "PackedSelect::apply, two tokens per ciphertext", {late(cx, zero, real)}, {out_of(cy)}, [&](Stream* s) { sel.apply(cx, cy, s); });
        const std::vector<uint64_t> got = r.decrypt_slots(cy);
        size_t bad = 0;
        for (size_t c = 0; c < C; ++c)
            for (size_t s = 0; s < n; ++s) {
                const size_t k = (s % row) % period, src_row = tpc == 2 ? s / row : 0;
                bad += got[c * n + s] != (k < length ? slots[c * n + src_row * row + offset + k] : 0);
            }
        CHECK(bad == 0);
    }
}

// ---- PackedTransformerBlock::apply with the four biases: d = 16, h = 500 (the constructor needs the padded h to fill a slot row: 512 at N = 1024) ---------
static void block(Rig& r) {
    const size_t n = r.n, row = n / 2, d = 16, h = 500, T = 3, pd = 16;
    std::vector<uint64_t> Wqkv(3 * d * d), Wo(d * d), Wu(h * d), Wd(d * h), bqkv(3 * d), bo(d), bu(h), bd(d), x(T * d), slots(T * n);
    for (auto* v : {&Wqkv, &Wo, &Wu, &Wd})
        for (auto& e : *v) e = small8();
    for (auto& e : x) e = 1 + rnd(100);
    for (auto* v : {&bqkv, &bo, &bu, &bd})
        for (auto& e : *v) e = rnd(T_MOD);
    PackedTransformerBlock blk(r.ctx, r.be, r.hks, Wqkv.data(), Wo.data(), Wu.data(), Wd.data(), d, h, bqkv.data(), bo.data(), bu.data(), bd.data());
    for (size_t tk = 0; tk < T; ++tk) blk.pack_input(&x[tk * d], &slots[tk * n]);
    Ciphertext cx(r.ctx, 2, T), real(r.ctx, 2, T), zero(r.ctx, 2, T), cy(r.ctx, 2, T);
    r.encrypt_slots(slots, real, zero);
    r.gate.gated("PackedTransformerBlock::apply", {late(cx, zero, real)}, {out_of(cy)}, [&](Stream* s) { blk.apply(cx, cy, s); });
    const std::vector<uint64_t> got = r.decrypt_slots(cy);
    size_t bad = 0;
    for (size_t tk = 0; tk < T; ++tk) {
        const uint64_t* xt = &x[tk * d];
        const std::vector<uint64_t> qkv = affine(Wqkv, bqkv.data(), 3 * d, d, xt, T_MOD), o = affine(Wo, bo.data(), d, d, &qkv[2 * d], T_MOD);
        std::vector<uint64_t> h1(d), h2(d);
        for (size_t i = 0; i < d; ++i) h1[i] = (xt[i] + o[i]) % T_MOD;
        const std::vector<uint64_t> u = affine(Wu, bu.data(), h, d, h1.data(), T_MOD), dn = affine(Wd, bd.data(), d, h, u.data(), T_MOD);
        for (size_t i = 0; i < d; ++i) h2[i] = (h1[i] + dn[i]) % T_MOD;
        for (size_t s = 0; s < n; ++s) {
            const size_t c = (s % row) % pd;
            bad += got[tk * n + s] != (c < d ? h2[c] : 0);
        }
    }
    CHECK(bad == 0);
}

// ---- ExactMultiplier::multiply, Rerandomizer::rerandomize, Evaluator::compact, BatchEncoder::encode_device from a device pointer ----------------------
static void exact_ops(Rig& r) {
    const size_t n = r.n, B = 3;
    FheParams p2 = r.p;
    p2.moduli.resize(2); p2.psi.resize(2);
    Context ctx2(p2, 0);
    SecretKey sk2(ctx2, r.kg.secret_key().coefficients());
    Encryptor enc2(ctx2, sk2, TestSeed{91});
    Decryptor dec2(ctx2, sk2);
    BatchEncoder be2(ctx2, T_MOD);
    std::vector<uint64_t> sx(B * n), dd(B * n), got(n);
    std::vector<int64_t> cx(B * n), zeros(B * n, 0);
    for (auto& v : sx) v = 1 + rnd(T_MOD - 1);
    for (size_t i = 0; i < B; ++i) be2.encode(&sx[i * n], &cx[i * n]);
    {
        ExactMultiplier mul(r.ctx, ctx2, T_MOD);
        Ciphertext a(ctx2, 2, B), real(ctx2, 2, B), zero(ctx2, 2, B), sq(ctx2, 3, B);
        enc2.encrypt_exact(cx.data(), T_MOD, real);
        enc2.encrypt_exact(zeros.data(), T_MOD, zero);
        r.gate.gated("ExactMultiplier::multiply", {late(a, zero, real)}, {out_of(sq)}, [&](Stream* s) { mul.multiply(a, a, sq, s); });
        dec2.decrypt_exact(sq, T_MOD, dd.data());
        size_t bad = 0;
        for (size_t i = 0; i < B; ++i) {
            be2.decode(&dd[i * n], got.data());
            for (size_t k = 0; k < n; ++k) bad += got[k] != (uint64_t)((unsigned __int128)sx[i * n + k] * sx[i * n + k] % T_MOD);
        }
        CHECK(bad == 0);
    }
    std::vector<int64_t> m(B * n);
    for (auto& v : m) v = (int64_t)(1 + rnd(T_MOD - 1));
    Ciphertext ct(r.ctx, 2, B), real(r.ctx, 2, B), zero(r.ctx, 2, B);
    r.enc.encrypt_exact(m.data(), T_MOD, real);
    r.enc.encrypt_exact(zeros.data(), T_MOD, zero);
    {
        PublicKey pk(r.ctx);
        r.kg.create_public_key(pk);
        Rerandomizer rr(r.ctx, pk, TestSeed{92});
        const unsigned flood = rr.max_flood_bits(T_MOD);
        r.gate.gated("Rerandomizer::rerandomize", {late(ct, zero, real)}, {}, [&](Stream* s) { rr.rerandomize(ct, T_MOD, flood, s); });
        r.dec.decrypt_exact(ct, T_MOD, dd.data());
        size_t bad = 0;
        for (size_t i = 0; i < B * n; ++i) bad += dd[i] != (uint64_t)m[i];
        CHECK(bad == 0);
        const std::vector<uint64_t> a = words(ct), b = words(real);
        CHECK(std::memcmp(a.data(), b.data(), a.size() * 8) != 0);          // (and it did re-randomise)
    }
    {
        const auto bits = CompactCiphertext::recommended_bits(r.p.log2_n, T_MOD);
        CompactCiphertext cc(r.ctx, B, bits.first, bits.second);
        r.gate.gated("Evaluator::compact", {late(ct, zero, real)}, {Out{cc.data(), cc.bytes()}}, [&](Stream* s) { r.ev.compact(ct, cc, s); });
        r.dec.decrypt_exact(cc, T_MOD, dd.data());
        size_t bad = 0;
        for (size_t i = 0; i < B * n; ++i) bad += dd[i] != (uint64_t)m[i];
        CHECK(bad == 0);
    }
    {
        std::vector<uint32_t> slots(B * n), z(B * n, 0);
        for (auto& v : slots) v = (uint32_t)rnd(T_MOD);
        uint32_t *d_slots = nullptr, *d_real = nullptr, *d_zero = nullptr;
        HIP(hipMalloc((void**)&d_slots, slots.size() * 4)); HIP(hipMalloc((void**)&d_real, slots.size() * 4)); HIP(hipMalloc((void**)&d_zero, slots.size() * 4));
        HIP(hipMemcpy(d_real, slots.data(), slots.size() * 4, hipMemcpyHostToDevice));
        HIP(hipMemcpy(d_zero, z.data(), z.size() * 4, hipMemcpyHostToDevice));
        for (bool to_ntt : {false, true}) {
            Plaintext out(r.ctx, B), ref(r.ctx, B);
            r.gate.gated(to_ntt ? "BatchEncoder::encode_device (device pointer, transformed)" : "BatchEncoder::encode_device (device pointer)",
                  {Late{d_slots, d_zero, d_real, slots.size() * 4}}, {out_of(out)}, [&](Stream* s) { r.be.encode_device(d_slots, B, out, to_ntt, s); });
            r.be.encode_device(slots.data(), B, ref, to_ntt);                 // from the host pointer, on the null stream: staged and synchronised
            r.ctx.synchronize();
            CHECK(words(out) == words(ref) && out.is_ntt() == to_ntt);
        }
        HIP(hipFree(d_slots)); HIP(hipFree(d_real)); HIP(hipFree(d_zero));
    }
}

// ---- the word-level Evaluator methods: gated on S == the same call on the idle null stream, word for word ------------------------------------------------
static void evaluator_methods(Rig& r) {
    const size_t n = r.n, L = r.p.n_limbs(), B = 3;
    auto fill = [&](PolyBuffer& b, bool zero) {
        std::vector<uint64_t> h(b.words());
        for (size_t i = 0; i < h.size(); ++i) h[i] = zero ? 0 : rnd(r.p.moduli[(i / n) % L]);
        b.copy_from_host(h.data());
    };
    Ciphertext a(r.ctx, 2, B), b(r.ctx, 2, B), ra(r.ctx, 2, B), rb(r.ctx, 2, B), z(r.ctx, 2, B), o2(r.ctx, 2, B), ref2(r.ctx, 2, B), o3(r.ctx, 3, B), ref3(r.ctx, 3, B);
    fill(ra, false); fill(rb, false); fill(z, true);
    const std::vector<Late> ab = {late(a, z, ra), late(b, z, rb)};
    auto load_real = [&] { HIP(hipMemcpy(a.data(), ra.data(), a.words() * 8, hipMemcpyDeviceToDevice)); HIP(hipMemcpy(b.data(), rb.data(), b.words() * 8, hipMemcpyDeviceToDevice)); };
    // (name, the call writing `out`): out-of-place binary and unary methods on 2-component buffers
    struct Op { const char* name; std::function<void(PolyBuffer&, Stream*)> call; };
    const Op ops[] = {
        {"Evaluator::add", [&](PolyBuffer& o, Stream* s) { r.ev.add(a, b, o, s); }},
        {"Evaluator::sub", [&](PolyBuffer& o, Stream* s) { r.ev.sub(a, b, o, s); }},
        {"Evaluator::negate", [&](PolyBuffer& o, Stream* s) { r.ev.negate(a, o, s); }},
        {"Evaluator::dyadic_multiply", [&](PolyBuffer& o, Stream* s) { r.ev.dyadic_multiply(a, b, o, s); }},
    };
    for (auto& op : ops) {
        r.gate.gated(op.name, ab, {out_of(o2)}, [&](Stream* s) { op.call(o2, s); });
        load_real();
        op.call(ref2, nullptr);
        r.ctx.synchronize();
        CHECK(words(o2) == words(ref2));
    }
    {   // the accumulator is an input too
        Ciphertext acc(r.ctx, 2, B), racc(r.ctx, 2, B);
        fill(racc, false);
        std::vector<Late> in3 = ab;
        in3.insert(in3.begin(), late(acc, z, racc));
        r.gate.gated("Evaluator::dyadic_multiply_add", in3, {}, [&](Stream* s) { r.ev.dyadic_multiply_add(a, b, acc, s); });
        load_real();
        HIP(hipMemcpy(ref2.data(), racc.data(), ref2.words() * 8, hipMemcpyDeviceToDevice));
        r.ev.dyadic_multiply_add(a, b, ref2);
        r.ctx.synchronize();
        CHECK(words(acc) == words(ref2));
    }
    for (bool fwd : {true, false}) {   // in place; the domain flag is set before every call
        r.gate.gated(fwd ? "Evaluator::transform_to_ntt_inplace" : "Evaluator::transform_from_ntt_inplace", {late(a, z, ra)}, {},
              [&](Stream* s) { a.set_ntt(!fwd); if (fwd) r.ev.transform_to_ntt_inplace(a, s); else r.ev.transform_from_ntt_inplace(a, s); });
        HIP(hipMemcpy(ref2.data(), ra.data(), ref2.words() * 8, hipMemcpyDeviceToDevice));
        ref2.set_ntt(!fwd);
        if (fwd) r.ev.transform_to_ntt_inplace(ref2); else r.ev.transform_from_ntt_inplace(ref2);
        r.ctx.synchronize();
        CHECK(words(a) == words(ref2));
        a.set_ntt(false); ref2.set_ntt(false);
    }
    r.gate.gated("Evaluator::multiply", ab, {out_of(o3)}, [&](Stream* s) { r.ev.multiply(a, b, o3, s); });
    load_real();
    r.ev.multiply(a, b, ref3);
    r.ctx.synchronize();
    CHECK(words(o3) == words(ref3));
    {
        RelinKeys rk(r.ctx);
        r.kg.create_relin_keys(rk);
        Ciphertext in3(r.ctx, 3, B), z3(r.ctx, 3, B);
        fill(z3, true);
        r.gate.gated("Evaluator::relinearize", {late(in3, z3, ref3)}, {out_of(o2)}, [&](Stream* s) { r.ev.relinearize(in3, rk, o2, s); });
        r.ev.relinearize(ref3, rk, ref2);
        r.ctx.synchronize();
        CHECK(words(o2) == words(ref2));
    }
    {
        Context next(r.p.drop_last_limb(), 0);
        Ciphertext lo(next, 2, B), lo_ref(next, 2, B);
        r.gate.gated("Evaluator::rescale", {late(a, z, ra)}, {out_of(lo)}, [&](Stream* s) { r.ev.rescale(a, lo, s); });
        r.ev.rescale(ra, lo_ref);
        r.ctx.synchronize();
        CHECK(words(lo) == words(lo_ref));
    }
    {   // NTT-domain methods: multiply_plain, the three matrix-vector products, reduce_sum
        const size_t rows = 2, cols = 3;
        Plaintext pt(r.ctx, 1, true), W(r.ctx, rows * cols, true);
        fill(pt, false); fill(W, false);
        a.set_ntt(true); ra.set_ntt(true); o2.set_ntt(true); ref2.set_ntt(true);
        r.gate.gated("Evaluator::multiply_plain", {late(a, z, ra)}, {out_of(o2)}, [&](Stream* s) { r.ev.multiply_plain(a, pt, o2, s); });
        r.ev.multiply_plain(ra, pt, ref2);
        r.ctx.synchronize();
        CHECK(words(o2) == words(ref2));
        Ciphertext y(r.ctx, 2, rows, true), yref(r.ctx, 2, rows, true);
        r.gate.gated("Evaluator::matvec_plain", {late(a, z, ra)}, {out_of(y)}, [&](Stream* s) { r.ev.matvec_plain(W, a, y, s); });
        r.ev.matvec_plain(W, ra, yref);
        r.ctx.synchronize();
        CHECK(words(y) == words(yref));
        ScalarMatrix Ws(r.ctx, rows, cols);
        std::vector<int64_t> w(rows * cols);
        for (auto& v : w) v = (int64_t)rnd(1 << 20) - (1 << 19);
        Ws.set(w.data());
        r.gate.gated("Evaluator::matvec_scalar", {late(a, z, ra)}, {out_of(y)}, [&](Stream* s) { r.ev.matvec_scalar(Ws, a, y, s); });
        r.ev.matvec_scalar(Ws, ra, yref);
        r.ctx.synchronize();
        CHECK(words(y) == words(yref));
        Plaintext W1(r.ctx, rows, true);                                       // cols = 1, n_rhs = 3: x is [1][3]
        fill(W1, false);
        Ciphertext ym(r.ctx, 2, rows * B, true), ymref(r.ctx, 2, rows * B, true);
        r.gate.gated("Evaluator::matvec_plain_multi", {late(a, z, ra)}, {out_of(ym)}, [&](Stream* s) { r.ev.matvec_plain_multi(W1, a, ym, B, s); });
        r.ev.matvec_plain_multi(W1, ra, ymref, B);
        r.ctx.synchronize();
        CHECK(words(ym) == words(ymref));
        Ciphertext one(r.ctx, 2, 1, true), one_ref(r.ctx, 2, 1, true);
        r.gate.gated("Evaluator::reduce_sum", {late(a, z, ra)}, {out_of(one)}, [&](Stream* s) { r.ev.reduce_sum(a, one, s); });
        r.ev.reduce_sum(ra, one_ref);
        r.ctx.synchronize();
        CHECK(words(one) == words(one_ref));
        a.set_ntt(false); ra.set_ntt(false); o2.set_ntt(false); ref2.set_ntt(false);
    }
    {   // exact plaintext addition and subtraction
        ExactPlaintext pb(r.ctx, T_MOD, 1);
        std::vector<int64_t> c(n);
        for (auto& v : c) v = (int64_t)rnd(T_MOD);
        pb.set_coefficients(c.data());
        r.gate.gated("Evaluator::add_plain_exact", {late(a, z, ra)}, {out_of(o2)}, [&](Stream* s) { r.ev.add_plain_exact(a, pb, o2, s); });
        r.ev.add_plain_exact(ra, pb, ref2);
        r.ctx.synchronize();
        CHECK(words(o2) == words(ref2));
        r.gate.gated("Evaluator::sub_plain_exact", {late(a, z, ra)}, {out_of(o2)}, [&](Stream* s) { r.ev.sub_plain_exact(a, pb, o2, s); });
        r.ev.sub_plain_exact(ra, pb, ref2);
        r.ctx.synchronize();
        CHECK(words(o2) == words(ref2));
    }
}

// ---- the methods that synchronise `stream` on purpose: values, and that they waited for S ----------------------------------------------------------------
static void synchronising_methods(Rig& r) {
    const size_t n = r.n, B = 2;
    std::vector<uint64_t> slots(B * n);
    for (auto& v : slots) v = 1 + rnd(T_MOD - 1);
    Ciphertext cx(r.ctx, 2, B), real(r.ctx, 2, B), zero(r.ctx, 2, B), cy(r.ctx, 2, B);
    r.encrypt_slots(slots, real, zero);
    const uint32_t g = r.be.galois_element(1);                                  // both rows one slot to the left
    auto rotated_ok = [&](const Ciphertext& ct) {
        const std::vector<uint64_t> got = r.decrypt_slots(ct);
        const size_t row = n / 2;
        size_t bad = 0;
        for (size_t i = 0; i < B; ++i)
            for (size_t s = 0; s < n; ++s) bad += got[i * n + s] != slots[i * n + (s / row) * row + (s % row + 1) % row];
        return bad == 0;
    };
    GaloisKeys gk(r.ctx, g);
    r.kg.create_galois_keys(gk);
    r.gate.gated("Evaluator::apply_galois", {late(cx, zero, real)}, {out_of(cy)}, [&](Stream* s) { r.ev.apply_galois(cx, gk, cy, s); }, /*enqueue_only=*/false);
    CHECK(rotated_ok(cy));
    r.hks.add_galois_element(g);
    r.gate.gated("HybridKeySwitcher::apply_galois", {late(cx, zero, real)}, {out_of(cy)}, [&](Stream* s) { r.hks.apply_galois(cx, g, cy, s); }, false);
    CHECK(rotated_ok(cy));
    // the rotations that only enqueue (their first call packs and caches the keys, which synchronises: that is the warm-up)
    r.gate.gated("HybridKeySwitcher::apply_galois_many", {late(cx, zero, real)}, {out_of(cy)}, [&](Stream* s) { r.hks.apply_galois_many(cx, std::vector<uint32_t>(B, g), cy, 0, s); });
    CHECK(rotated_ok(cy));
    r.gate.gated("HybridKeySwitcher::apply_galois_grouped", {late(cx, zero, real)}, {out_of(cy)}, [&](Stream* s) { r.hks.apply_galois_grouped(cx, 0, std::vector<uint32_t>(1, g), B, cy, 0, s); });
    CHECK(rotated_ok(cy));
    r.gate.gated("HybridKeySwitcher::apply_galois_hoisted", {late(cx, zero, real)}, {out_of(cy)}, [&](Stream* s) { r.hks.apply_galois_hoisted(cx, 0, B, std::vector<uint32_t>(1, g), cy, 0, s); });
    CHECK(rotated_ok(cy));
    {   // relinearisation of a product: decrypts to the slot-wise square
        FheParams p2 = r.p;
        p2.moduli.resize(2); p2.psi.resize(2);
        Context ctx2(p2, 0);
        SecretKey sk2(ctx2, r.kg.secret_key().coefficients());
        Encryptor enc2(ctx2, sk2, TestSeed{93});
        Decryptor dec2(ctx2, sk2);
        BatchEncoder be2(ctx2, T_MOD);
        HybridKeySwitcher hks2(ctx2, sk2, r.special, r.special_psi, TestSeed{94});
        ExactMultiplier mul(r.ctx, ctx2, T_MOD);
        std::vector<int64_t> c(B * n), zeros(B * n, 0);
        for (size_t i = 0; i < B; ++i) be2.encode(&slots[i * n], &c[i * n]);
        Ciphertext a(ctx2, 2, B), z2(ctx2, 2, B), sq(ctx2, 3, B), sq0(ctx2, 3, B), in3(ctx2, 3, B), out(ctx2, 2, B);
        enc2.encrypt_exact(c.data(), T_MOD, a);
        enc2.encrypt_exact(zeros.data(), T_MOD, z2);
        mul.multiply(a, a, sq);
        mul.multiply(z2, z2, sq0);
        ctx2.synchronize();
        r.gate.gated("HybridKeySwitcher::relinearize", {late(in3, sq0, sq)}, {out_of(out)}, [&](Stream* s) { hks2.relinearize(in3, out, s); }, false);
        std::vector<uint64_t> dd(B * n), got(n);
        dec2.decrypt_exact(out, T_MOD, dd.data());
        size_t bad = 0;
        for (size_t i = 0; i < B; ++i) {
            be2.decode(&dd[i * n], got.data());
            for (size_t k = 0; k < n; ++k) bad += got[k] != (uint64_t)((unsigned __int128)slots[i * n + k] * slots[i * n + k] % T_MOD);
        }
        CHECK(bad == 0);
    }
}

// ---- a stream destroyed before its scratch arena is released: the release waits for the arena's last recorded work, never for the stream handle -------
static void destroyed_stream(Rig& r) {
    const size_t n = r.n, L = r.p.n_limbs(), terms = 2;
    Ciphertext a(r.ctx, 2, terms), b(r.ctx, 2, terms), sum(r.ctx, 3, 1), ref(r.ctx, 3, 1);
    for (Ciphertext* ct : {&a, &b}) {
        std::vector<uint64_t> h(ct->words());
        for (size_t i = 0; i < h.size(); ++i) h[i] = rnd(r.p.moduli[(i / n) % L]);
        ct->copy_from_host(h.data());
    }
    r.ctx.release_scratch(nullptr, true);
    CHECK(r.ctx.scratch_bytes() == 0);
    r.ev.multiply_sum(a, b, terms, false, ref);                           // on the null stream
    r.ctx.synchronize();
    void* s = nullptr;
    CHECK(stream_gate_stream_create(&s) == 0 && s);
    const size_t before = r.ctx.scratch_bytes();
    r.ev.multiply_sum(a, b, terms, false, sum, s);                        // composed at every ring degree: an arena for s
    CHECK(r.ctx.scratch_bytes() > before);
    HIP(hipStreamSynchronize(static_cast<hipStream_t>(s)));
    CHECK(stream_gate_stream_destroy(s) == 0);
    CHECK(dpfhe_ctx_release_scratch(static_cast<dpfhe_ctx*>(r.ctx.handle()), nullptr, DPFHE_SCRATCH_ALL) == DPFHE_SUCCESS);
    CHECK(dpfhe_ctx_scratch_bytes(static_cast<dpfhe_ctx*>(r.ctx.handle())) == 0);
    CHECK(words(sum) == words(ref));
}

int main(int argc, char** argv) {
    const double G = argc > 1 ? std::atof(argv[1]) : 0.040;
    if (!(G >= 0.010 && G <= 0.1)) { std::printf("G = %g s is outside [0.010, 0.1]\n", G); return 2; }
    try {
        Rig r(G);
        if (!r.gate.ok()) { std::printf("no non-blocking stream\n"); return 2; }
        evaluator_methods(r);
        packed_linear(r);
        packed_select(r);
        block(r);
        exact_ops(r);
        synchronising_methods(r);
        destroyed_stream(r);
        r.ctx.synchronize();
        std::printf("%d gated facade calls; G = %.1f ms; slowest t_enqueue %.3f ms (%s)\n", r.gate.gated_calls, G * 1e3, r.gate.slowest * 1e3, r.gate.slowest_what.c_str());
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    return finish("stream C++ facade OK");
}
