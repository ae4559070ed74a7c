"""CPU: every place on the hot path where a Galois element g selects a permutation, along the ELEMENT - the whole group at the small rings, the 2-adic
edges (tests/galois_elements.py edge_elements) at the large ones - against definitions in Python integers:

  the oracles themselves          Oracle.apply_galois and the Python restatement the fused-pass tests use (rotate_add_ref.automorphism) against sigma;
  workmap.h galois_inverse        g g^-1 = 1 mod 2N for every odd g at every ring degree (the launchers of every coefficient-domain rotation);
  dpfhe_rotate_add_pass_host      the host twin's own inverse and gather (csrc/rotate_add.h), on products with a known quotient;
  ntt_core.h galois_src_pos       against src_pos (the position path at N = 256 / 512, both hoisted key-switch kernels);
  workmap.h QpMap::pair_map       test_work_maps_cpu.py test_qp_pair_map's assertions (the two baby-step kernels);
  ntt_core.h gather_plan          the kernels' own plan, staged loads, LDS rows and reads on in[i] = i (tools/emulate.cpp emu_gather_map): one-piece with
                                  h = (g - 1) / 2, and through galois_sub_block at N = 32768 / 65536 - the source position, the staged range inside the
                                  polynomial, the wave's lanes agreeing on their region.

The coefficient-domain gathers of kernels_rotate.h (galois_kernel, galois_multi_kernel, rotate_add_pass_kernel) have no CPU twin of their index code: they
are held along the same elements on the GPU (tests/test_gpu_galois_elements.py), and what they compute from g on the host - galois_inverse - here.

Two planted defects show that the checks bite where the element list the suite had before ((3, 5, 2N - 1, 3^7), rings up to N = 8192) does not."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import galois_elements as ge
import rotate_add_ref
from deeppowers_amd.params import ntt_primes
from oracle.cbind import Oracle
from test_emulated_kernels import emu  # noqa: F401  (the module fixture that builds tools/libemu.so)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64 = C.POINTER(C.c_int64)
LOG_N2 = 12          # the sub-transforms of a split transform: N2 = 4096 (devtables.h kSplitLog2N2)


@pytest.fixture(scope="module")
def wm(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu") / "libemu_workmap.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "emulate_workmap.cpp")])
    lib = C.CDLL(so)
    for name, res, args in (
        ("wm_qp_segments", C.c_uint, [C.c_int, C.c_uint]),
        ("wm_qp_pair_map", None, [C.c_int, C.c_uint, C.c_uint, C.c_uint, I64]),
        ("wm_galois_src_pos", C.c_int, [C.c_int, C.c_uint, I64]),
        ("wm_galois_inverse", C.c_uint, [C.c_uint, C.c_uint]),
        ("wm_galois_inverse_all", None, [C.c_uint, I64]),
    ):
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    return lib


@pytest.fixture(scope="module")
def gather(emu):
    """tools/libemu.so (built by test_emulated_kernels' fixture) with the gather exports declared"""
    lib = emu
    lib.emu_gather_map.argtypes = [C.c_int, C.c_uint, I64]
    lib.emu_gather_map.restype = C.c_int
    lib.emu_gather_map_split.argtypes = [C.c_int, C.c_uint, I64, I64]
    lib.emu_gather_map_split.restype = C.c_int
    return lib


def _p(a):
    return a.ctypes.data_as(I64)


# ---- the element sets and the definitions ----------------------------------------------------------------------------------------------------------------
def test_element_sets():
    for ln, count in ge.EDGE_COUNTS.items():
        elts = ge.edge_elements(ln)
        assert len(elts) == count == len(set(elts)) and all(g & 1 and 0 < g < (2 << ln) for g in elts)
    assert len(ge.edge_elements(12)) <= 64 < len(ge.edge_elements(13))           # from N = 8192 more than one 64-element launch group
    for ln in range(8, 17):
        n, elts = 1 << ln, ge.edge_elements(ln)
        assert ge.all_elements(ln) == [g for g in range(2 * n) if g & 1]
        assert {pow(3, 1 << k, 2 * n) for k in range(ln - 1)} <= set(elts)        # the slot-sum ladders' steps ...
        assert all(pow(3, 1 << k, 2 << ln) % (1 << (k + 3)) == 1 + (1 << (k + 2)) for k in range(1, ln - 1))   # ... are 1 + 2^(k+2) mod 2^(k+3) from k = 1
        for j in range(3, ln + 1):                                                # both signs at every power of two
            assert any(g % (1 << j) == 1 and g != 1 for g in elts) and any(g % (1 << j) == (1 << j) - 1 for g in elts)
        assert sum(g % 8 in (5, 7) for g in elts) >= ln                          # the negative half -3^k (powers of 3 are 1 or 3 mod 8): the row swaps


def test_vector_forms_are_the_definitions():
    """galois_elements.src_pos_table / sigma_words, which the large rings are compared with, are src_pos / sigma at every element of N = 256"""
    q = 65537
    a = np.array([0, q - 1, 1] + [(7 * i * i + 3) % q for i in range(253)], np.uint64)
    for g in ge.all_elements(8):
        assert ge.src_pos_table(g, 8).tolist() == [ge.src_pos(g, p, 8) for p in range(256)]
        assert ge.sigma_words(a, g, q).tolist() == ge.sigma(a.tolist(), g, q)


# ---- the oracles first -------------------------------------------------------------------------------------------------------------------------------------
def _oracle_inputs(orc, seed):
    """[3][L][N]: random words with 0 and q - 1 planted (the sign of zero), all q - 1, and all 0 but one word"""
    x = orc.fill(3, seed)
    qcol = np.array(orc.moduli, np.uint64)[:, None]
    x[0, :, 0::7] = 0
    x[0, :, 3::11] = np.broadcast_to(qcol - np.uint64(1), x[0].shape)[:, 3::11]
    x[1] = qcol - np.uint64(1)
    x[2] = 0
    x[2, :, 1] = 1
    return x


@pytest.mark.parametrize("ln", [8, 12, 16])
def test_oracle_automorphism_is_sigma(ln):
    """One fold prime (2^60 - d) and one prime below 2^47, both limbs of one context; every element at N = 256, edge_elements at N = 4096 and 65536.
    At every element and on both limbs: sigma in Python integers, coefficient by coefficient, equals Oracle.apply_galois and rotate_add_ref.automorphism on the
    striped item (at N = 65536 about ten seconds of Python loops).  The other two items are held to sigma_words, which the same comparisons tie to sigma."""
    f, s = ntt_primes(ln, 1), ntt_primes(ln, 1, 47)
    assert f.moduli[0] > (1 << 59) and s.moduli[0] < (1 << 47)
    orc = Oracle(ln, f.moduli + s.moduli, f.psi + s.psi)
    x = _oracle_inputs(orc, 1200 + ln)
    assert (x == 0).any() and (x[0] == np.array(orc.moduli, np.uint64)[:, None] - np.uint64(1)).any()
    elts = ge.all_elements(ln) if ln == 8 else ge.edge_elements(ln)
    for g in elts:
        got = orc.apply_galois(x, g)
        for l, q in enumerate(orc.moduli):
            for item in range(3):
                assert np.array_equal(got[item, l], ge.sigma_words(x[item, l], g, q)), (g, q, item)
            want = ge.sigma(x[0, l].tolist(), g, q)
            assert got[0, l].tolist() == want, (g, q)
            assert rotate_add_ref.automorphism(x[0, l], g, q).tolist() == want, (g, q)


# ---- galois_inverse ------------------------------------------------------------------------------------------------------------------------------------------
def newton_inverse(g, two_n, steps=5):
    """workmap.h galois_inverse restated in Python on 32-bit words, with the number of Newton steps a parameter"""
    inv = 1
    for _ in range(steps):
        inv = (inv * (2 - g * inv)) & 0xFFFFFFFF
    return inv & (two_n - 1)


def inverse_failures(inverse_of, ln, elts):
    """the check: g inv = 1 mod 2N and inv < 2N -> the elements that miss it"""
    two_n = 2 << ln
    return [g for g in elts if not (0 <= inverse_of(g) < two_n and (g * inverse_of(g)) % two_n == 1)]


@pytest.mark.parametrize("ln", range(8, 17))
def test_galois_inverse_at_every_element(wm, ln):
    two_n = 2 << ln
    inv = np.full(two_n // 2, -1, np.int64)
    wm.wm_galois_inverse_all(two_n, _p(inv))
    g = np.arange(1, two_n, 2, dtype=np.int64)
    assert ((inv >= 0) & (inv < two_n)).all() and ((g * inv) % two_n == 1).all()
    for e in ge.edge_elements(ln):                                               # ... and one by one, in Python integers, with the entry the launchers call
        i = wm.wm_galois_inverse(e, two_n)
        assert i == inv[e >> 1] == pow(e, -1, two_n) == newton_inverse(e, two_n)
    assert inverse_failures(lambda e: int(inv[e >> 1]), ln, ge.edge_elements(ln)) == []


def old_elements(ln):
    """what test_work_maps_cpu.py ran before the element sets, at rings up to N = 8192"""
    return (3, 5, (2 << ln) - 1, pow(3, 7, 2 << ln))


def test_planted_defect_four_newton_steps():
    """PLANTED: galois_inverse with four Newton steps instead of five - 16 correct bits, not 32: right mod 2^16 (every ring up to N = 32768), wrong mod 2^17.
    The inverse check rejects it at N = 65536 - on the whole group and on edge_elements alone - and the old list at its old rings accepts it."""
    def four(ln):
        return lambda g: newton_inverse(g, 2 << ln, steps=4)
    assert inverse_failures(four(16), 16, ge.all_elements(16))
    caught = inverse_failures(four(16), 16, ge.edge_elements(16))
    assert caught and (1 << 17) - 1 in caught                                    # (-1 is its own inverse; four steps from 1 give 2^16 - 1)
    for ln in range(8, 14):
        assert inverse_failures(four(ln), ln, old_elements(ln)) == []
    for ln in range(8, 16):                                                      # nor would ANY element below N = 65536 have shown it
        assert inverse_failures(four(ln), ln, ge.all_elements(ln)) == []
    assert inverse_failures(lambda g: newton_inverse(g, 1 << 17), 16, ge.all_elements(16)) == []   # the restatement itself, with five


# ---- dpfhe_rotate_add_pass_host: galois_inverse and a gather of its own on the host (csrc/rotate_add.h) ------------------------------------------------------
@pytest.mark.parametrize("ln", [8, 13, 14, 16])
def test_rotate_add_pass_host_along_the_elements(ln):
    """out.c0 = round(work.c0 / P) + c0 + sigma_g(c0), out.c1 = round(work.c1 / P) + c1, with work = R P for a known small R per coefficient (the division
    itself is held at its edges by tests/test_rotate_add_cpu.py): every element at N = 256, edge_elements at N = 8192, 16384 and 65536; c0 carries 0 and
    q - 1 words"""
    p = ntt_primes(ln, 3)
    n, Ld, P = p.n, 2, p.moduli[-1]
    rng = np.random.default_rng(2100 + ln)
    R = rng.integers(0, 1 << 20, size=(1, 2, 1, n)).astype(np.uint64)
    qd = np.array(p.moduli[:Ld], np.uint64)[None, None, :, None]
    work = np.zeros((1, 2, Ld + 1, n), np.uint64)
    for l, q in enumerate(p.moduli[:Ld]):
        work[0, :, l] = ((R[0, :, 0].astype(object) * P) % q).astype(np.uint64)  # (R P mod P = 0 on the special limb)
    in2 = rng.integers(0, 1 << 59, size=(1, 2, Ld, n)).astype(np.uint64) % qd
    in2[0, 0, :, 0::7] = 0
    in2[0, 0, :, 3::11] = np.broadcast_to(qd[0, 0] - np.uint64(1), (Ld, n))[:, 3::11]
    base = (R % qd + in2) % qd
    bad = []
    for g in ge.all_elements(ln) if ln == 8 else ge.edge_elements(ln):
        want = base.copy()
        for l, q in enumerate(p.moduli[:Ld]):
            want[0, 0, l] = (want[0, 0, l] + ge.sigma_words(in2[0, 0, l], g, q)) % np.uint64(q)
        if not np.array_equal(rotate_add_ref.pass_twin(p, work, in2, g), want):
            bad.append(g)
    assert bad == []
    g = (2 << ln) - 3                                                            # ... and once against the Python-integer pass itself
    if ln == 8:
        assert np.array_equal(rotate_add_ref.pass_twin(p, work, in2, g), rotate_add_ref.pass_reference(p.moduli, work, in2, g))


# ---- galois_src_pos ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ln", range(8, 17))
def test_galois_src_pos_along_the_elements(wm, ln):
    """every element at N = 256 and 1024, edge_elements at every other ring degree the export instantiates (up to N = 65536, where g e reaches 2^34)"""
    n = 1 << ln
    out = np.zeros(n, np.int64)
    for g in ge.all_elements(ln) if ln in (8, 10) else ge.edge_elements(ln):
        assert wm.wm_galois_src_pos(ln, g, _p(out)) == 0
        assert np.array_equal(out, ge.src_pos_table(g, ln)), g
        if ln == 8 or g in (3, 2 * n - 1):
            assert out.tolist() == [ge.src_pos(g, p, ln) for p in range(n)], g
    assert wm.wm_galois_src_pos(17, 3, _p(out)) == -1


# ---- QpMap::pair_map -----------------------------------------------------------------------------------------------------------------------------------------
def _check_pair_map(wm, ln, pairs, g, rev1, nseg):
    """test_work_maps_cpu.py test_qp_pair_map's assertions for one element, on whole segments at a time"""
    n, half, seg = 1 << ln, 1 << (ln - 1), 256 * pairs
    sp = ge.src_pos_table(g, ln)
    written = []
    rows = np.zeros((seg, 4), np.int64)
    for sseg in range(nseg):
        wm.wm_qp_pair_map(ln, pairs, g, sseg, _p(rows))
        out, src, swap, ok = rows.T
        assert np.array_equal(ok, (out < half).astype(np.int64)), (g, sseg)
        live = ok != 0
        out, src, swap = out[live], src[live], swap[live]
        written.append(out)
        assert (src // seg == sseg).all() if nseg > 1 else (src < half).all(), (g, sseg)
        cf = (g * (2 * rev1[out] + 1)) % (2 * n)
        assert np.array_equal(swap, (cf >= n).astype(np.int64)), (g, sseg)
        s0, s1 = sp[2 * out], sp[2 * out + 1]
        assert np.array_equal(s0, 2 * src + swap) and np.array_equal(s1, 2 * src + 1 - swap), (g, sseg)
        assert len(set((out // seg).tolist())) == 1, (g, sseg)                  # one output segment per source segment
    assert np.array_equal(np.sort(np.concatenate(written)), np.arange(half)), g


@pytest.mark.parametrize("ln,pairs", [(8, 1), (8, 2), (10, 1), (10, 2), (13, 1), (13, 2), (14, 1), (14, 2)])
def test_qp_pair_map_along_the_elements(wm, ln, pairs):
    """every element at N = 256 and 1024, edge_elements at N = 8192 and 16384"""
    nseg = wm.wm_qp_segments(ln, pairs)
    assert nseg == max(1, (1 << (ln - 1)) // (256 * pairs))
    rev1 = ge.brv_table(ln - 1)
    for g in ge.all_elements(ln) if ln <= 10 else ge.edge_elements(ln):
        _check_pair_map(wm, ln, pairs, g, rev1, nseg)


# ---- gather_plan, as the kernels use it ----------------------------------------------------------------------------------------------------------------------
def gather_failures(gather_of, ln, elts):
    """the check: the source position every output position reads is src_pos -> the elements that miss it"""
    return [g for g in elts if not np.array_equal(gather_of(g), ge.src_pos_table(g, ln))]


def kernel_gather(gather, ln):
    def run(g):
        out = np.full(1 << ln, -1, np.int64)
        rc = gather.emu_gather_map(ln, g, _p(out))
        return out if rc == 0 else np.full(1 << ln, rc, np.int64)
    return run


@pytest.mark.parametrize("ln", [10, 11, 12, 13, 14])
def test_one_piece_gather_along_the_elements(gather, ln):
    """ntt_inv_galois_kernel's gather with h = (g - 1) / 2: every element at N = 1024, edge_elements at N = 2048 ... 16384.  A staged range outside the
    polynomial or a wave whose lanes disagree on their region comes back as -7 in every position."""
    elts = ge.all_elements(ln) if ln == 10 else ge.edge_elements(ln)
    assert gather_failures(kernel_gather(gather, ln), ln, elts) == []
    if ln == 10:                                                                 # the definition itself, position by position
        for g in (3, 9, 2047):
            assert kernel_gather(gather, ln)(g).tolist() == [ge.src_pos(g, p, ln) for p in range(1 << ln)]
    assert gather.emu_gather_map(9, 3, _p(np.zeros(512, np.int64))) == -1


@pytest.mark.parametrize("ln", [15, 16])
def test_split_gather_along_the_elements(gather, ln):
    """ntt_inv_galois_sub_kernel's gather through galois_sub_block: block * 4096 + index is src_pos of b * 4096 + k, and every sub-block is its own source
    exactly when g = 1 mod 2 N1 - the elements at which an in-place call would not need its staging"""
    n, n1 = 1 << ln, 1 << (ln - LOG_N2)
    out, blocks = np.zeros(n, np.int64), np.zeros(n1, np.int64)
    own = []
    for g in ge.edge_elements(ln):
        assert gather.emu_gather_map_split(ln, g, _p(out), _p(blocks)) == 0, g
        assert np.array_equal(out, ge.src_pos_table(g, ln)), g
        assert np.array_equal(out >> LOG_N2, np.repeat(blocks, 1 << LOG_N2)), g
        assert sorted(blocks.tolist()) == list(range(n1)), g
        stays = blocks.tolist() == list(range(n1))
        assert stays == (g % (2 * n1) == 1), g
        own.append(stays)
    assert sum(own) > 2 and not all(own)                                         # both directions are met on the set (2^j + 1 and t - 2^j + 1 from 2^j = 2 N1 up)
    assert out.tolist()[:4096:97] == [ge.src_pos(ge.edge_elements(ln)[-1], p, ln) for p in range(0, 4096, 97)]


def shortcut_gather(ln, shortcut=True):
    """PLANTED (the gather check's defect): the one-piece gather restated in Python - r' = (g r + h) mod N on bit-reversed positions, the wave's region from its
    first word - with a shortcut: a wave whose source region is its OWN region (shift 0) is taken for a wave that needs no gather and reads its words in
    place.  That is right only for g = 1.  A ring of W = N / 1024 waves keeps every wave in its own region exactly when g = 1 mod 2 W (8 at N = 4096, 32 at
    N = 16384) - and such a g still permutes the words inside the region.
    shortcut=False: the same restatement without the defect, which the test holds to the kernels' own gather at the rings where the defect is asserted."""
    n, wave = 1 << ln, 64 * 16
    rev = ge.brv_table(ln)

    def run(g):
        sp = rev[(g * rev + ((g - 1) >> 1)) & (n - 1)]
        for w in range(n // wave if shortcut else 0):
            if sp[w * wave] // wave == w:
                sp[w * wave:(w + 1) * wave] = np.arange(w * wave, (w + 1) * wave)
        return sp
    return run


def test_planted_defect_own_region_shortcut(gather):
    """the gather check rejects shortcut_gather on edge_elements at N = 4096, 8192 and 16384 - at exactly the elements that are 1 mod 2 W, the slot-sum
    ladders' 3^(2^k) from 2^(k+2) = 2 W among them; the old list - 3, 5, 2N - 1 and 3^7 are 3, 5, 7 and 3 mod 8 - accepts it at all three.  (With one wave,
    N = 1024, or two, where 5 is 1 mod 4, any list rejects it.)"""
    for ln in (12, 13, 14):
        two_w = 2 << (ln - 10)
        caught = gather_failures(shortcut_gather(ln), ln, ge.edge_elements(ln))
        assert caught == [g for g in ge.edge_elements(ln) if g % two_w == 1 and g != 1]
        assert pow(3, 1 << (ln - 10), 2 << ln) in caught and pow(3, 1 << (ln - 2), 2 << ln) in caught and (1 << ln) + 1 in caught
        assert gather_failures(shortcut_gather(ln), ln, old_elements(ln)) == []
        # the restatement is the kernels' gather: without the shortcut at every element of the set, with it at every element but the ones caught
        kernel = kernel_gather(gather, ln)
        for g in ge.edge_elements(ln):
            assert np.array_equal(shortcut_gather(ln, shortcut=False)(g), kernel(g)), (ln, g)
            assert np.array_equal(shortcut_gather(ln)(g), kernel(g)) == (g not in caught), (ln, g)
    assert gather_failures(shortcut_gather(10), 10, old_elements(10)) and gather_failures(shortcut_gather(11), 11, old_elements(11)) == [5]
