"""CPU: the fused multiply's lazy transforms at N = 4096 (twiddles split at bit 29, unreduced butterfly products), through tools/emulate.cpp:
the product chain against Python integers with its exact assertions armed, every entry of the lazy bound plans recomputed from the stated rule,
the emulated kernel against the oracle word for word, and the two pinned table blobs unchanged beside the new one."""
import ctypes as C
import hashlib
import json
import os
import random
import subprocess

import numpy as np
import pytest

import class_edges
from deeppowers_amd.params import FheParams
from oracle.cbind import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = C.POINTER(C.c_uint64)
I = C.POINTER(C.c_int)
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(ROOT, "tools", "libemu.so")
    src = os.path.join(ROOT, "tools", "emulate.cpp")
    deps = [src] + [os.path.join(ROOT, "deeppowers_amd", "csrc", f) for f in ("ntt_core.h", "ntt_top.h", "ntt_halves.h", "ntt_quarters.h", "modarith.h", "tables.h", "ctx_tables.h", "devtables.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src])
    lib = C.CDLL(so)
    lib.emu_overflows.restype = C.c_long
    lib.emu_fold_tw29.argtypes = [C.c_uint64] * 4
    lib.emu_fold_tw29.restype = C.c_uint64
    lib.emu_ct_mul_lazy29.argtypes = [C.c_uint64, C.c_uint64, C.c_int, U, U, U, U, U]
    lib.emu_lazy29_plan.argtypes = [C.c_int, C.c_int, C.c_int, I, I, I]
    lib.emu_lazy29_totals.argtypes = [I]
    lib.emu_lazy29_totals.restype = None
    return lib


BENCH = FheParams.n4096_l4()
EDGE = class_edges.edge_moduli("fold", 12)


def arith_primes():
    """the four bench primes and the fold primes with the largest and the smallest admissible d at N = 4096"""
    cat = class_edges.catalogue_moduli(12)
    return list(BENCH.moduli) + [cat["fold_edge"][0], cat["fold_near"][0]]


def chain29(y, w, q):
    """mul_tw29_add's chain without the addend, in Python integers: (H, L - addend, H.hi 2d)"""
    d = (1 << 60) - q
    ws = (w << 32) % q
    a, b, as_, bs = w & ((1 << 29) - 1), w >> 29, ws & ((1 << 29) - 1), ws >> 29
    assert a < 1 << 29 and as_ < 1 << 29 and b < 1 << 31 and bs < 1 << 31
    y0, y1 = y & 0xFFFFFFFF, y >> 32
    H = y0 * b + y1 * bs
    assert H <= M64
    return H, (H & 0xFFFFFFFF) * (1 << 29) + y0 * a + y1 * as_, (H >> 32) * 2 * d


@pytest.mark.parametrize("q", arith_primes(), ids=lambda q: f"d{(1 << 60) - q:#x}")
def test_mul_tw29_add_matches_python_integers_up_to_its_limit(emu, q):
    """R = addend + y w (mod q), R < 4.125 * 2^60 + y / 8 + addend, nothing asserts with the addend at exactly the largest value the chain holds, and
    the emulator's exact assertion fires one above it"""
    d = (1 << 60) - q
    rng = random.Random(q)
    ys = [0, 1, 1 << 63, M64] + [rng.getrandbits(64) for _ in range(40)]
    ws = [0, 1, q - 1] + [rng.randrange(q) for _ in range(40)]
    for y in ys:
        for w in ws:
            H, L0, F = chain29(y, w, q)
            limit = M64 - L0 - F                     # the largest addend for which L and R = L + H.hi 2d stay below 2^64
            assert limit >= (11 << 60) + (7 << 57) - (y >> 3) - 1, "any addend with addend + y / 8 < 11.875 * 2^60 must be admissible"
            for addend in (0, rng.randrange(limit + 1), limit):
                before = emu.emu_overflows()
                r = emu.emu_fold_tw29(d, y, w, addend)
                assert emu.emu_overflows() == before, (hex(y), hex(w), hex(addend))
                assert r == L0 + F + addend and r % q == (addend + y * w) % q
                assert r < (4 << 60) + (1 << 57) + (y >> 3) + 1 + addend
            if limit < M64:                          # (y w = 0 leaves the whole word to the addend: nothing above it to try)
                before = emu.emu_overflows()
                emu.emu_fold_tw29(d, y, w, limit + 1)
                assert emu.emu_overflows() > before, "one above the limit must trip the assertion"


# ---- the lazy plans, from the rule stated in ntt_core.h ---------------------------------------------------------------------------------------------
UNIT, RED, WORD = 1024, 1025, 16 * 1024
LAZY = 4 * UNIT + UNIT // 8 + 1         # 4.125 * 2^60 in q / 1024, rounded up
FWD_CAP, INV_CAP, INV_OUT = 14 * UNIT, 6 * UNIT + UNIT // 4, 3 * UNIT // 2
LB_TOP, STAGES, E = 3, 4, 16            # every phase of the (12, 4) geometry: local bits 3 .. 0


def fwd_plan(in_bound, cap):
    b, red_a, Ks, n = [in_bound] * E, {}, {}, 0
    for u in range(STAGES):
        bit = 1 << (LB_TOP - u)
        for k in range(E):
            if k & bit:
                continue
            A, P = b[k], LAZY + (b[k | bit] + 7) // 8
            K = -(-P // UNIT)
            red = P + A > WORD or A + K * UNIT > WORD
            if not red and u == STAGES - 1 and A > RED and (P + A > cap or A + K * UNIT > cap) and P + RED <= cap and RED + K * UNIT <= cap:
                red = True
            if red:
                A, n = RED, n + 1
            red_a[u, k], Ks[u, k] = red, K
            b[k], b[k | bit] = P + A, A + K * UNIT
            assert b[k] <= WORD and b[k | bit] <= WORD
    red_end = [v > cap for v in b]
    b = [RED if r else v for v, r in zip(b, red_end)]
    return red_a, Ks, red_end, b, n + sum(red_end)


def inv_plan(in_bound, cap, last):
    b, red, offs, n = [in_bound] * E, {}, {}, 0
    for u in range(STAGES):
        bit = 1 << u
        fin = last and u == STAGES - 1
        sum_cap = WORD - UNIT // 8 if fin else WORD
        for k in range(E):
            if k & bit:
                continue
            bx, by = b[k], b[k | bit]
            red[u, k] = red[u, k | bit] = False
            for _ in range(2):
                if bx + by <= sum_cap and bx + -(-by // UNIT) * UNIT <= WORD:
                    break
                if bx >= by and bx > RED:
                    red[u, k], bx = True, RED
                else:
                    red[u, k | bit], by = True, RED
                n += 1
            off = -(-by // UNIT)
            assert bx + by <= sum_cap and bx + off * UNIT <= WORD
            offs[u, k] = off
            b[k] = UNIT + ((bx + by) >> 12) + 2 if fin else bx + by
            b[k | bit] = RED if fin else LAZY + (bx + off * UNIT + 7) // 8
            n += fin
    red_end = [v > cap for v in b]
    b = [RED if r else v for v, r in zip(b, red_end)]
    return red, offs, red_end, b, n + sum(red_end)


def test_lazy_plans_follow_the_stated_rule(emu):
    """every entry of the three forward and three inverse phase plans of the N = 4096 geometry: reductions, K / offsets, bounds, and the reduction counts the
    kernel asserts at compile time (40 forward, 55 inverse per transform and thread, against 96 butterflies)"""
    tot = (C.c_int * 8)()
    emu.emu_lazy29_totals(tot)
    assert tot[5] == FWD_CAP and tot[6] == INV_CAP and tot[7] == RED
    flags, consts, tail = (C.c_int * 64)(), (C.c_int * 64)(), (C.c_int * 34)()
    in_bound, total = UNIT, 0
    for p in range(3):
        cap = WORD if p == 2 else FWD_CAP
        red_a, Ks, red_end, out, n = fwd_plan(in_bound, cap)
        assert emu.emu_lazy29_plan(0, p, in_bound, flags, consts, tail) == 0
        for (u, k), r in red_a.items():
            assert flags[u * 16 + k] == r and consts[u * 16 + k] == Ks[u, k], (p, u, k)
        assert [tail[k] for k in range(16)] == red_end and [tail[18 + k] for k in range(16)] == out
        assert tail[16] == max(out) == tot[2 + p] and tail[17] == n
        in_bound, total = max(out), total + n
    assert total == tot[0] == 40
    assert in_bound <= WORD                      # what the tensor step's a side takes: any 64-bit word
    total = 0
    for p in (2, 1, 0):
        cap = INV_OUT if p == 0 else INV_CAP
        in_bound = RED if p == 2 else INV_CAP
        red, offs, red_end, out, n = inv_plan(in_bound, cap, p == 0)
        assert emu.emu_lazy29_plan(1, p, in_bound, flags, consts, tail) == 0
        for (u, k), r in red.items():
            assert flags[u * 16 + k] == r, (p, u, k)
        for (u, k), o in offs.items():
            assert consts[u * 16 + k] == o, (p, u, k)
        assert [tail[k] for k in range(16)] == red_end and tail[16] == max(out) <= cap and tail[17] == n
        total += n
    assert total == tot[1] == 55


# ---- the emulated kernel ---------------------------------------------------------------------------------------------------------------------------
def patterns(orc, q, n, seed):
    rnd = orc.fill(4, seed).reshape(4, n)
    alt = np.where(np.arange(n) % 2 == 0, 0, q - 1).astype(np.uint64)
    return {"max": np.full((4, n), q - 1, np.uint64), "zero": np.zeros((4, n), np.uint64), "random": rnd, "alternating": np.stack([alt, alt[::-1], alt, alt[::-1]])}


LIMBS = [("bench", l, BENCH.moduli[l], BENCH.psi[l]) for l in range(BENCH.n_limbs)] + [("edge", l, EDGE.moduli[l], EDGE.psi[l]) for l in range(EDGE.n_limbs)]


@pytest.mark.parametrize("name,limb,q,psi", LIMBS, ids=[f"{n}{l}" for n, l, _, _ in LIMBS])
def test_emulated_lazy_multiply_matches_oracle_without_wraps(emu, name, limb, q, psi):
    """ct_mul_quad_kernel<FoldArith, 12, 4>'s per-thread code on the bit-29 blob, assertions armed: coefficient-domain and NTT-domain output"""
    n = 4096
    orc = Oracle(12, [q], [psi])
    before = emu.emu_overflows()
    for pat, polys in patterns(orc, q, n, 1100 + limb).items():
        a0, a1, b0, b1 = (np.ascontiguousarray(polys[i], dtype=np.uint64) for i in range(4))
        want = orc.ct_mul(np.stack([a0, a1]).reshape(1, 2, 1, n), np.stack([b0, b1]).reshape(1, 2, 1, n)).reshape(3, n)
        for out_ntt in (0, 1):
            out = np.zeros(3 * n, np.uint64)
            assert emu.emu_ct_mul_lazy29(q, psi, out_ntt, a0.ctypes.data_as(U), a1.ctypes.data_as(U), b0.ctypes.data_as(U), b1.ctypes.data_as(U), out.ctypes.data_as(U)) == 0
            ref = want if not out_ntt else np.stack([orc.ntt_fwd(np.ascontiguousarray(want[j])) for j in range(3)])
            assert np.array_equal(out.reshape(3, n), ref), (pat, out_ntt)
    assert emu.emu_overflows() == before, "a lazy word wrapped around 2^64 or a chain left its exact bounds"


# ---- the table blobs -------------------------------------------------------------------------------------------------------------------------------
with open(os.path.join(ROOT, "tests", "golden", "ctx_table_digests.json")) as _f:
    CTX_DIGESTS = json.load(_f)


def test_pinned_blobs_keep_their_digests_beside_the_lazy_blob(emu):
    """the context-wide blob and the class blob are byte for byte what tests/golden/ctx_table_digests.json pins; the lazy blob exists exactly for the
    contexts at log2 N = 12 with a fold limb, sized fwd | inv | last in 256-byte sections"""
    B = C.POINTER(C.c_ubyte)
    emu.emu_ctx_blob.argtypes = [C.c_int, C.c_int, U, U, C.c_int, B, C.c_size_t, B]
    emu.emu_ctx_blob.restype = C.c_long
    recs = list(CTX_DIGESTS) + [{"log2n": 12, "moduli": list(BENCH.moduli), "psi": list(BENCH.psi), "limb_cls": [1] * 4, "ctx_blob": None, "class_blob": None}]
    seen_lazy = 0
    for rec in recs:
        m, w = np.array(rec["moduli"], np.uint64), np.array(rec["psi"], np.uint64)
        L = len(rec["moduli"])
        cls = np.zeros(16, np.uint8)
        blob = lambda which, buf, cap: emu.emu_ctx_blob(rec["log2n"], L, m.ctypes.data_as(U), w.ctypes.data_as(U), which, buf, cap, cls.ctypes.data_as(B))
        for which, key in ((0, "ctx_blob"), (1, "class_blob")):
            if "name" not in rec:
                continue
            size = blob(which, None, 0)
            assert size == (rec[key]["bytes"] if rec[key] else 0), (rec["name"], key)
            if rec[key]:
                buf = np.zeros(size, np.uint8)
                assert blob(which, buf.ctypes.data_as(B), size) == size
                assert hashlib.sha256(buf.tobytes()).hexdigest() == rec[key]["sha256"], (rec["name"], key)
        size = blob(2, None, 0)
        fold_limb = L <= 16 and 1 in [int(v) for v in cls[:L]] or all((1 << 60) - q < 1 << 24 for q in rec["moduli"])
        up = lambda x: (x + 255) & ~255
        want = up(up(2 * up(L * 4096 * 16)) + L * 32) if rec["log2n"] == 12 and fold_limb else 0
        assert size == want, rec.get("name")
        seen_lazy += size > 0
    assert seen_lazy >= 1
    # the bench context's lazy blob: every twiddle's halves in range, and the pair reassembles to w and w 2^32 mod q
    rec = recs[-1]
    m, w = np.array(rec["moduli"], np.uint64), np.array(rec["psi"], np.uint64)
    buf = np.zeros(size, np.uint8)
    assert emu.emu_ctx_blob(12, 4, m.ctypes.data_as(U), w.ctypes.data_as(U), 2, buf.ctypes.data_as(B), size, None) == size
    words = buf.view(np.uint64)
    for l, q in enumerate(BENCH.moduli):
        tw = words[l * 4096 * 2: (l + 1) * 4096 * 2].reshape(4096, 2)
        lo, hi = tw & np.uint64(0xFFFFFFFF), tw >> np.uint64(32)
        assert int(lo.max()) < 1 << 29 and int(hi.max()) < 1 << 31
        for wv, wsv in [tuple(int(v) for v in lo[i] + (hi[i] << np.uint64(29))) for i in (0, 1, 1000, 4095)]:
            assert wv < q and wsv == (wv << 32) % q
