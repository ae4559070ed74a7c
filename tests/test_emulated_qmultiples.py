"""CPU: where the inverse butterflies of the fused multiply at N = 4096 take their multiple of q from (ntt_core.h Gs29Ride, FoldArith::mul_tw29_add_uniform),
through tools/emulate.cpp with its assertions armed: the chain that carries a multiple against Python integers, every entry of the derived table recomputed
from the stated rule, one thread's phase against a plain butterfly network, a multiple folded where the bounds have no room (it must trip the assertions),
and the emulated kernel against the oracle word for word."""
import ctypes as C
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
    lib.emu_fold_tw29_uniform.argtypes = [C.c_uint64] * 4
    lib.emu_fold_tw29_uniform.restype = C.c_uint64
    lib.emu_ct_mul_lazy29.argtypes = [C.c_uint64, C.c_uint64, C.c_int, U, U, U, U, U]
    lib.emu_lazy29_plan.argtypes = [C.c_int, C.c_int, C.c_int, I, I, I]
    lib.emu_gs29_ride.argtypes = [C.c_int, C.c_int, I]
    lib.emu_gs29_ride_shipped.argtypes = [I]
    lib.emu_gs29_phase.argtypes = [C.c_int, C.c_uint64, I, U, C.c_uint64, U]
    return lib


BENCH = FheParams.n4096_l4()
EDGE = class_edges.edge_moduli("fold", 12)
LIMBS = [("bench", l, BENCH.moduli[l], BENCH.psi[l]) for l in range(BENCH.n_limbs)] + [("edge", l, EDGE.moduli[l], EDGE.psi[l]) for l in range(EDGE.n_limbs)]
PRIMES = [q for _, _, q, _ in LIMBS]

UNIT, RED, WORD = 1024, 1025, 16 * 1024
LAZY = 4 * UNIT + UNIT // 8 + 1
INV_CAP, INV_OUT = 6 * UNIT + UNIT // 4, 3 * UNIT // 2
STAGES, E = 4, 16
PHASES = {2: (RED, INV_CAP, False), 1: (INV_CAP, INV_CAP, False), 0: (INV_CAP, INV_OUT, True)}   # phase: input bound, output cap, last (in the order they run)


def chain29(y, w, q):
    """the twiddle chain without an addend, in Python integers: (H, L, H.hi 2d)"""
    d = (1 << 60) - q
    ws = (w << 32) % q
    a, b, as_, bs = w & ((1 << 29) - 1), w >> 29, ws & ((1 << 29) - 1), ws >> 29
    y0, y1 = y & 0xFFFFFFFF, y >> 32
    H = y0 * b + y1 * bs
    assert H <= M64
    return H, (H & 0xFFFFFFFF) * (1 << 29) + y0 * a + y1 * as_, (H >> 32) * 2 * d


# ---- the chain that carries a multiple of q ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", PRIMES, ids=lambda q: f"d{(1 << 60) - q:#x}")
def test_chain_with_a_multiple_on_board_matches_python_integers_up_to_its_limit(emu, q):
    """R = y w (mod q) whatever multiple k q rides, R = the plain chain's word + k q exactly, nothing asserts up to the largest k the word holds and the
    exact assertion fires one multiple above it"""
    d = (1 << 60) - q
    rng = random.Random(q + 1)
    ys = [0, 1, 1 << 63, M64] + [rng.getrandbits(64) for _ in range(40)]
    ws = [0, 1, q - 1] + [rng.randrange(q) for _ in range(40)]
    for y in ys:
        for w in ws:
            _, L0, F = chain29(y, w, q)
            kmax = min((M64 - L0 - F) // q, 15)        # (16 q does not fit a word)
            assert kmax >= (11 * 8 + 7 - ((y >> 57) + 1)) // 8, "any multiple with k q + y / 8 < 11.875 * 2^60 must be admissible"
            for k in {0, 1, rng.randrange(kmax + 1), kmax}:
                before = emu.emu_overflows()
                r = emu.emu_fold_tw29_uniform(d, y, w, k)
                assert emu.emu_overflows() == before, (hex(y), hex(w), k)
                assert r == L0 + F + k * q and r % q == y * w % q
            if kmax < 15:
                before = emu.emu_overflows()
                emu.emu_fold_tw29_uniform(d, y, w, kmax + 1)
                assert emu.emu_overflows() > before, "one multiple above the limit must trip the assertion"


# ---- the derived table, from the rule stated in ntt_core.h ------------------------------------------------------------------------------------------
def shipped_plan(emu, phase):
    in_bound, cap, last = PHASES[phase]
    flags, consts, tail = (C.c_int * 64)(), (C.c_int * 64)(), (C.c_int * 34)()
    assert emu.emu_lazy29_plan(1, phase, in_bound, flags, consts, tail) == 0
    red = [[bool(flags[u * 16 + k]) for k in range(E)] for u in range(STAGES)]
    off = [[consts[u * 16 + k] for k in range(E)] for u in range(STAGES)]
    return red, off, [bool(tail[k]) for k in range(E)]


def ride_fits(red, off, red_end, ride, in_bound, cap, last):
    """the phase walked with the true bounds under the plan's own reductions and offsets: every subtrahend <= off q, every sum inside its cap, every
    difference and product inside a word, every unreduced output inside the hand-over cap, every multiple consumed by the butterfly it was meant for"""
    b, on = [in_bound] * E, [False] * E
    for u in range(STAGES):
        bit = 1 << u
        fin = last and u == STAGES - 1
        sum_cap = WORD - UNIT // 8 if fin else WORD
        for k in range(E):
            if k & bit:
                continue
            kk = k | bit
            bx, by = b[k], b[kk]
            if on[kk] or (on[k] and red[u][k]):
                return False
            bx = RED if red[u][k] else bx
            by = RED if red[u][kk] else by
            offq = off[u][k] * UNIT
            dl = bx if on[k] else bx + offq
            if by > offq or bx + by > sum_cap or dl > WORD:
                return False
            rides = ride[u][kk]
            if rides and (fin or u + 1 >= STAGES or kk & (bit << 1)):
                return False
            b[k] = UNIT + ((bx + by) >> 12) + 2 if fin else bx + by
            b[kk] = RED if fin else LAZY + (dl + 7) // 8 + (off[u + 1][kk] * UNIT if rides else 0)
            if b[kk] > WORD:
                return False
            on[k], on[kk] = False, rides
    return not any(on) and all(red_end[k] or b[k] <= cap for k in range(E))


def derive_ride(red, off, red_end, in_bound, cap, last):
    ride = [[False] * E for _ in range(STAGES)]
    for u in range(STAGES - 1):
        for kk in range(E):
            if not kk & (1 << u) or kk & (2 << u):
                continue
            ride[u][kk] = True
            if not ride_fits(red, off, red_end, ride, in_bound, cap, last):
                ride[u][kk] = False
    return ride


def test_derived_table_follows_the_stated_rule(emu):
    """every entry of the three phases' tables, as the emulator derives them and as the shipped body compiles them in; the plans themselves pass the walk
    with nothing on board; 3 of the first phase's 12 candidates ride and none of the other phases' (their products are at 5.78 q)"""
    flags, shipped = (C.c_int * 64)(), (C.c_int * 192)()
    total = emu.emu_gs29_ride_shipped(shipped)
    counts = {}
    for phase, (in_bound, cap, last) in PHASES.items():
        red, off, red_end = shipped_plan(emu, phase)
        assert ride_fits(red, off, red_end, [[False] * E for _ in range(STAGES)], in_bound, cap, last)
        want = derive_ride(red, off, red_end, in_bound, cap, last)
        n = emu.emu_gs29_ride(phase, in_bound, flags)
        for u in range(STAGES):
            for k in range(E):
                assert bool(flags[u * 16 + k]) == want[u][k] == bool(shipped[phase * 64 + u * 16 + k]), (phase, u, k)
        counts[phase] = n
        assert n == sum(map(sum, want))
    assert counts == {2: 3, 1: 0, 0: 0} and total == 3


# ---- one thread's phase -------------------------------------------------------------------------------------------------------------------------------
def run_phase(emu, phase, q, ride, w, w_last, x):
    ws = (C.c_uint64 * 32)(*w)
    xs = (C.c_uint64 * 16)(*x)
    fl = None if ride is None else (C.c_int * 64)(*[int(ride[u][k]) for u in range(STAGES) for k in range(E)])
    before = emu.emu_overflows()
    assert emu.emu_gs29_phase(phase, q, fl, ws, w_last, xs) == 0
    return list(xs), emu.emu_overflows() - before


@pytest.mark.parametrize("q", PRIMES[:2] + PRIMES[-2:], ids=lambda q: f"d{(1 << 60) - q:#x}")
def test_first_inverse_phase_with_multiples_on_board_is_a_butterfly_network(emu, q):
    """the phase whose table has entries, on words at the top of its input bound and random ones: residues equal x' = a + b, y' = (a - b) w stage by stage"""
    d = (1 << 60) - q
    rng = random.Random(q + 2)
    top = (1 << 60) + 16 * d - 1
    for x in ([top] * 16, [0] * 16, [top if k & 1 else 0 for k in range(16)], [0 if k & 1 else top for k in range(16)], [rng.randrange(top + 1) for _ in range(16)]):
        w = [rng.randrange(q) for _ in range(32)]
        got, trips = run_phase(emu, 2, q, None, w, 1, x)
        assert trips == 0
        ref = [v % q for v in x]
        for u in range(STAGES):
            for k in range(E):
                if k & (1 << u):
                    continue
                a, b = ref[k], ref[k | 1 << u]
                ref[k], ref[k | 1 << u] = (a + b) % q, (a - b) * w[u * 8 + (k >> (u + 1))] % q
        assert [v % q for v in got] == ref


def test_a_multiple_folded_where_the_bounds_have_no_room_trips_the_assertions(emu):
    """Second inverse phase: its inputs are below 6.25 q, a first-stage product reaches 4.125 * 2^60 + 13.25 q / 8 = 5.78 q, and the next butterfly of two such
    products has offset 6: 5.78 + 5.78 + 6 passes 16 q, so the rule leaves the entry clear.  Forced on, with inputs and twiddles that drive both products
    towards their bound, the sum wraps and the armed emulator says so; the shipped table takes the same words without a word."""
    q = BENCH.moduli[0]
    in_bound, cap, last = PHASES[1]
    red, off, red_end = shipped_plan(emu, 1)
    assert off[0][0] == 7 and off[1][1] == 6 and not red[1][1] and not red[1][3]
    forced = [[False] * E for _ in range(STAGES)]
    forced[0][1] = True
    assert not ride_fits(red, off, red_end, forced, in_bound, cap, last)
    # the difference of the stage-0 butterflies (0, 1) and (2, 3): y = a - b + 7 q, as large as the input bound allows, low word all ones
    a = q * 6400 // 1024 - 1
    y = ((a + 7 * q) >> 32 << 32) - 1
    b = a + 7 * q - y
    assert 0 <= b < a
    rng = random.Random(29)
    best = max((rng.randrange(q) for _ in range(4000)), key=lambda w: sum(chain29(y, w, q)[1:]))
    r = sum(chain29(y, best, q)[1:])
    assert r + 6 * q <= M64 < 2 * r + 6 * q, "each product fits a word with the multiple on board, their sum does not"
    x = [a, b, a, b] + [0] * 12
    w = [best] * 8 + [1] * 24
    _, trips = run_phase(emu, 1, q, forced, w, 1, x)
    assert trips > 0
    _, trips = run_phase(emu, 1, q, None, w, 1, x)
    assert trips == 0


# ---- the emulated kernel ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,limb,q,psi", LIMBS, ids=[f"{n}{l}" for n, l, _, _ in LIMBS])
def test_emulated_multiply_with_the_new_butterflies_matches_oracle_without_wraps(emu, name, limb, q, psi):
    """ct_mul_quad_kernel<FoldArith, 12, 4>'s per-thread code, assertions armed, on all-(q - 1), all-zero and random inputs"""
    n = 4096
    orc = Oracle(12, [q], [psi])
    before = emu.emu_overflows()
    for pat, polys in {"max": np.full((4, n), q - 1, np.uint64), "zero": np.zeros((4, n), np.uint64), "random": orc.fill(4, 4100 + limb).reshape(4, n)}.items():
        a0, a1, b0, b1 = (np.ascontiguousarray(polys[i], dtype=np.uint64) for i in range(4))
        want = orc.ct_mul(np.stack([a0, a1]).reshape(1, 2, 1, n), np.stack([b0, b1]).reshape(1, 2, 1, n)).reshape(3, n)
        out = np.zeros(3 * n, np.uint64)
        assert emu.emu_ct_mul_lazy29(q, psi, 0, a0.ctypes.data_as(U), a1.ctypes.data_as(U), b0.ctypes.data_as(U), b1.ctypes.data_as(U), out.ctypes.data_as(U)) == 0
        assert np.array_equal(out.reshape(3, n), want), pat
    assert emu.emu_overflows() == before, "a lazy word wrapped around 2^64 or a chain left its exact bounds"
