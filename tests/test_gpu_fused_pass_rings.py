"""-m gpu: the four fused last passes of the approximate family along the ring ladder (include/dpfhe.h dpfhe_rotate_add_hybrid, dpfhe_relinearize_rescale_hybrid,
dpfhe_lincomb_rescale, dpfhe_relinearize_lincomb_rescale_hybrid; rotate_add_pass_kernel in csrc/kernels_rotate.h, relin_rescale_kernel, lincomb_rescale_kernel and
relin_lincomb_rescale_kernel in csrc/kernels_keyswitch.h).

Each entry's own module holds it to the oracle at the rings its feature picked (N = 256, 1024, 4096, the all-fold contexts above N = 8192).  Here the RING is the
variable and the workload stays small: N = 512 and 2048 (one and four full chunks), N = 8192 - the largest fused ring, and the only one where a workgroup of
rotate_add_pass_kernel walks TWO chunks (workmap.h RotateAddMap: 8 slices of 16 chunks) -, generic primes at N = 16384 (ShoupArith behind the composed key
products; the un-staged gather of rotate_add_pass_kernel<ShoupArith, false>), N = 32768 and N = 65536 (the split transforms) on fold and on generic primes, and
class_edges' "mixed" context at N = 4096 and 8192: eight limbs of 60 / 47 / 59 / 17 (16 at N = 4096) / 51 / 50 / 60 / 48 bits, one of every class, Ld = 7, a 48-bit special prime
under 60-bit data limbs, the key products from one launch per class.

Every output word is compared (np.array_equal: no sampling, no tolerance) with
  * test_gpu_rotate_add.reference: the oracle's automorphism, hybrid key switch and modular add, step by step;
  * the oracle's hybrid key switch followed by its rescale, or by the Python-integer sum and rescale of tests/relin_lincomb_ref.py;
  * the Python-integer linear combination and rescale of tests/fused_rescale_ref.py.
The device calls, rigs, shapes' helpers and arena cases are the ones of tests/test_gpu_rotate_add.py, test_gpu_fused_rescale.py, test_gpu_relin_lincomb.py and
test_gpu_footprint.py.

dpfhe_rotate_add_hybrid sends its Galois elements 64 items at a time inside the step loop, and its key products run the grouped layout with key_group = batch:
test_rotate_add_batch_thresholds crosses the launch group at 65 items (two steps: the second group lands in d_acc and then in d_out2; one step: d_acc is NULL)
and puts batch * Ld on 6, 8 and 9 polynomials, around one round of 8 of the XCD deal.

What each group is the first in the suite to run (read from cabi_rotate.hip, cabi_keyswitch.hip, cabi.h with_ctx_arith and workmap.h):
  N = 8192, any context     rotate_add_pass_kernel<., true> with per = 2: the second trip of the slice loop - FoldArith on fold_ld2 / fold_ld4, ShoupArith on the
                            other three; relin_rescale_kernel, lincomb_rescale_kernel and relin_lincomb_rescale_kernel word for word at 16 chunks
  shoup at N = 16384        rotate_add_pass_kernel<ShoupArith, false> (the gather from global memory on generic arithmetic); relin_rescale_kernel<ShoupArith> and
                            relin_lincomb_rescale_kernel<ShoupArith> behind key_products_composed
  N = 32768, 65536          the three rescaling passes behind the composed products on the split transforms (rotate-and-add had N = 32768 on fold primes only);
                            N = 65536 for all four, the widest ntt_grid_fits case; ShoupArith on both rings
  mixed at N = 4096, 8192   the four passes fed by relin_launch's for_each_class (five launches) at Ld = 7, their ShoupArith instantiations on limbs of every width
  N = 512, 2048             relin geometries 9 and 11 in front of the passes
  lincomb at N >= 2048      lincomb_rescale_kernel against a reference on the device beyond two chunks
  65 items                  the second for_slices group of dpfhe_rotate_add_hybrid (first = 64: dst + first * ct_words in d_acc and in d_out2, cur + first * ct_words
                            in d_in2 and in d_acc), RelinMap's grouped layout with key_group = 65, and key_group = 2, 3, 4 on 6, 9 and 8 polynomials"""
import functools
import itertools

import numpy as np
import pytest

import class_edges
import fused_rescale_ref as fr
import relin_lincomb_ref as rl
import rotate_add_ref as ra
import test_gpu_footprint as fp
import test_gpu_fused_rescale as fu
import test_gpu_relin_lincomb as trl
import test_gpu_rotate_add as tra
from deeppowers_amd.evaluator import to_host
from deeppowers_amd.params import FheParams, min_primitive_2n_root, ntt_primes

pytestmark = pytest.mark.gpu

# (context, log2 N).  fold_ldK: ntt_primes(log2 N, K + 1), all fold (the pinned primes are 1 mod 16384 and stop at N = 8192); every other name is a class_edges kind
LADDER = ([(name, ln) for ln in (9, 11) for name in ("fold_ld2", "shoup")]
          + [(name, 13) for name in ("fold_ld2", "fold_ld4", "shoup", "f64_under_fold", "mixed")]
          + [("mixed", 12), ("shoup", 14)]
          + [(name, ln) for ln in (15, 16) for name in ("fold_ld2", "shoup")])
# dpfhe_lincomb_rescale: fold and generic primes at every ring from 12 to 16 as well.  At N = 65536 on TWO limbs (fold_ld1, shoup2) instead of three and four: with
# K = 16 the Python-integer reference alone took 0.5 s on the ladder's contexts there, more than twice the slowest case of the three modules this one draws on
LINCOMB = LADDER[:-2] + [("fold_ld2", 12), ("shoup", 12), ("fold_ld2", 14), ("fold_ld1", 16), ("shoup2", 16)]


def generic_primes(log2n, limbs=4):
    """class_edges.edge_moduli("shoup", log2n) - the two widest generic primes, the first above 2^59, the first above 2^50 - or its first `limbs` limbs, from the
    catalogue's PRIMES alone: edge_moduli finds a root for every prime of the catalogue, N multiplications each, before it picks four
    (tests/test_fused_pass_rings_cpu.py holds the two equal)"""
    cat = class_edges.catalogue_moduli(log2n)
    qs = (cat["shoup60"][:2] + cat["shoup_above_59"][:1] + cat["shoup_above_50"][:1])[:limbs]
    return FheParams(log2n, qs, tuple(min_primitive_2n_root(1 << log2n, q) for q in qs))


@functools.lru_cache(maxsize=None)
def params(name, log2n):
    if name.startswith("fold_ld"):
        return ntt_primes(log2n, int(name[7:]) + 1)
    if name.startswith("pinned_ld"):
        return fr.pinned(log2n, int(name[9:]) + 1)
    if name in ("shoup", "shoup2") and log2n >= 15:
        return generic_primes(log2n, 2 if name == "shoup2" else 4)
    return class_edges.edge_moduli(name, log2n)


def by_shape(ctxs, shapes, at_13):
    """(context, log2 N, shape) for every shape, one case each; `at_13` only at N = 8192"""
    return [(name, ln, s) for name, ln in ctxs for s in shapes + ((at_13,) if ln == 13 else ())]


def shape_ids(cases):
    return [f"{name}_n{1 << ln}_{a}x{b}" for name, ln, (a, b) in cases]


@pytest.fixture
def rig():
    made = []

    def make(name, log2n):
        r = fp.ParamsRig(name, params(name, log2n))
        assert r.ctx.uses_fold == name.startswith(("fold_ld", "pinned_ld"))
        made.append(r)
        return r
    yield make
    for r in made:
        r.close()


# ---- dpfhe_rotate_add_hybrid ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,log2n", LADDER, ids=fp.ids(LADDER))
def test_rotate_add_equals_the_oracle(rig, name, log2n):
    r = rig(name, log2n)
    Ld, data = r.L - 1, fp.data_oracle(r)
    for steps, batch in tra.COMPOSED_SHAPES + (((3, 3),) if log2n == 13 else ()):
        elts = tra.ladder_elements(r.n, steps)
        keys = r.words(r.orc, (steps, Ld, 2), 41 + steps)
        ct = r.words(data, (batch, 2), 50 + batch)
        got, want = tra.device(r, ct, elts, keys), tra.reference(r, ct, elts, keys)
        assert got.shape == want.shape == (batch, 2, Ld, r.n)
        assert np.array_equal(got, want), (name, log2n, steps, batch, np.argwhere(got != want)[:4])


def plant_from(p, ct, g, plan, start):
    """every (direct word, gathered word, sign of the gather) over {0, 1, q - 1} once more in item 0's c0, on every data limb, at coefficients k >= start whose
    own word and whose gather source rotate_add_ref.pass_inputs' plan has left free.  -> the coefficients, in the order planted"""
    n, Ld = p.n, p.n_limbs - 1
    fixed = set()
    for k, *_ in plan:
        fixed |= {k, ra.gather_source(k, g, n)[0]}
    ks = []
    for negated in (False, True):
        for d, s in itertools.product(ra.WORDS, repeat=2):
            for k in range(start, n):
                src, neg = ra.gather_source(k, g, n)
                if neg != negated or src == k or k in fixed or src in fixed:
                    continue
                fixed |= {k, src}
                for l, q in enumerate(p.moduli[:Ld]):
                    ct[0, 0, l, k], ct[0, 0, l, src] = ra.word(d, q), ra.word(s, q)
                ks.append(k)
                break
    return ks


@pytest.mark.parametrize("name", ("fold_ld4", "mixed"))
def test_transparent_input_sums_land_on_the_edges_in_both_chunks_of_a_slice(rig, name):
    """test_gpu_rotate_add.test_transparent_input_sums_land_on_the_edges' construction at N = 8192 (c1 = 0: the output is (c0 + sigma_g(c0), 0)), where slice 0 of
    a polynomial is chunks 0 and 1.  pass_inputs plants from coefficient 0 upward - chunk 0 -, plant_from plants the same pairs again from 512 on - chunk 1, the
    second trip of the slice loop: both sets of sums are 0, 1, 2, q - 1 and q - 2 on every limb, the 17-bit one of the mixed context included"""
    r = rig(name, 13)
    Ld, g = r.L - 1, 3
    _, ct, plan = ra.pass_inputs(r.p, 2, 19, g)
    first = [k for k, *_ in plan]
    second = plant_from(r.p, ct, g, plan, 512)
    assert r.n // 512 == 16 and len(second) == 18 and max(first) < 512 <= min(second) and max(second) < 1024
    ct[:, 1] = 0
    keys = r.words(r.orc, (1, Ld, 2), 23)
    want = tra.reference(r, ct, [g], keys)
    assert not want[:, 1].any()
    for ks in (first, second):
        for l, q in enumerate(r.p.moduli[:Ld]):
            sums = {int(want[0, 0, l, k]) for k in ks}
            assert sums == {0, 1, 2, q - 1, q - 2}, (l, sorted(sums))
    got = tra.device(r, ct, [g], keys)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


def step_elements(n, steps):
    return tra.ladder_elements(n, steps) if steps in (1, 3) else [ra.elements(n)[0], ra.elements(n)[3]]


# (context, log2 N, steps, items, items x Ld)
THRESHOLDS = [("fold_ld2", 8, 2, 65, 130), ("fold_ld2", 8, 1, 65, 130), ("fold_ld2", 8, 1, 4, 8), ("fold_ld3", 8, 1, 2, 6), ("fold_ld3", 8, 1, 3, 9)]


@pytest.mark.parametrize("name,log2n,steps,batch,polys", THRESHOLDS, ids=[f"{n}_n{1 << ln}_{s}x{b}" for n, ln, s, b, _ in THRESHOLDS])
def test_rotate_add_batch_thresholds(rig, name, log2n, steps, batch, polys):
    """every item of every case against the oracle: the smallest ring keeps 65 items cheap"""
    r = rig(name, log2n)
    Ld, data = r.L - 1, fp.data_oracle(r)
    assert batch * Ld == polys
    elts = step_elements(r.n, steps)
    keys = r.words(r.orc, (steps, Ld, 2), 141 + steps)
    ct = r.words(data, (batch, 2), 150 + batch)
    got, want = tra.device(r, ct, elts, keys), tra.reference(r, ct, elts, keys)
    assert got.shape == want.shape == (batch, 2, Ld, r.n)
    assert np.array_equal(got, want), (steps, batch, sorted({int(i) for i in np.argwhere(got != want)[:, 0]}))


def test_rotate_add_second_launch_group_at_n8192(rig):
    """65 items x 2 steps on the two-chunk slices: both sides of the launch group and its last item against the oracle, word for word"""
    r = rig("fold_ld2", 13)
    Ld, data, steps, batch = r.L - 1, fp.data_oracle(r), 2, 65
    elts = step_elements(r.n, steps)
    keys = r.words(r.orc, (steps, Ld, 2), 143)
    ct = r.words(data, (batch, 2), 215)
    got = tra.device(r, ct, elts, keys)
    assert got.shape == ct.shape
    for item in sorted({0, 63, 64, batch - 1}):
        want = tra.reference(r, ct[item:item + 1], elts, keys)
        assert np.array_equal(got[item:item + 1], want), (item, np.argwhere(got[item:item + 1] != want)[:4])


# ---- the three rescaling passes --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,log2n", LADDER, ids=fp.ids(LADDER))
def test_relinearize_rescale_hybrid_equals_the_oracle(rig, name, log2n):
    r = rig(name, log2n)
    Ld, data = r.L - 1, fp.data_oracle(r)
    key = r.words(r.orc, (Ld, 2), 41)
    for batch in ((1,) if log2n >= 15 else (1, 3)):
        ct3 = r.words(data, (batch, 3), 50 + batch)
        got, want = fu.device(r, ct3, key), fu.reference(r, ct3, key)
        assert got.shape == want.shape == (batch, 2, Ld - 1, r.n)
        assert np.array_equal(got, want), (name, log2n, batch, np.argwhere(got != want)[:4])


LINCOMB_CASES = by_shape(LINCOMB, ((1, 1), (16, 1)), (3, 3))                  # (K, items)
RELIN_LINCOMB_CASES = by_shape(LADDER, ((0, 1), (5, 1)), (1, 3))


@pytest.mark.parametrize("name,log2n,shape", LINCOMB_CASES, ids=shape_ids(LINCOMB_CASES))
def test_lincomb_rescale_equals_the_integers(rig, name, log2n, shape):
    import torch
    r = rig(name, log2n)
    K, batch = shape
    x, w = fr.lincomb_inputs(r.p, K, batch, 100 * K + log2n)
    got = r.ev.lincomb_rescale(r.dev(x), r.dev(w))
    torch.cuda.synchronize()
    got, want = to_host(got), fr.lincomb_rescale_reference(r.p.moduli, x, w)
    assert got.shape == want.shape == (batch, 2, r.L - 1, r.n)
    assert np.array_equal(got, want), (name, log2n, K, batch, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("name,log2n,shape", RELIN_LINCOMB_CASES, ids=shape_ids(RELIN_LINCOMB_CASES))
def test_relinearize_lincomb_rescale_equals_the_oracle_and_the_integers(rig, name, log2n, shape):
    r = rig(name, log2n)
    Ld, data = r.L - 1, fp.data_oracle(r)
    K, batch = shape
    key = r.words(r.orc, (Ld, 2), 41)
    ct3 = r.words(data, (batch, 3), 50 + batch)
    terms, w = rl.terms_and_weights(r.p, K, batch, 60 + K)
    assert [z.shape[2] for z in terms] == rl.term_limbs(K, Ld)
    assert K < 2 or (terms[1].shape[2] == Ld + 2 and (terms[1][:, :, Ld:] == rl.NOT_A_RESIDUE).all())     # terms at mixed heights, the unread limbs no residues
    got, want = trl.device(r, ct3, key, terms, w), trl.reference(r, ct3, key, terms, w)
    assert got.shape == want.shape == (batch, 2, Ld - 1, r.n)
    assert np.array_equal(got, want), (name, log2n, K, batch, np.argwhere(got != want)[:4])


# ---- footprints at N = 8192 ------------------------------------------------------------------------------------------------------------------------------------
FOOTPRINT = {"rotate_add": lambda r: tra.arena_cases(r, tra.ALL_SHAPES), "fused_rescale": fu.arena_cases, "relin_lincomb": trl.arena_cases}


@pytest.mark.parametrize("entry", list(FOOTPRINT))
def test_footprint_at_n8192(rig, entry):
    """the arena cases of the three modules on the pinned primes at Ld = 4: a two-chunk slice that wrote past its polynomial lands in a guard band or in a
    neighbour's words"""
    assert fp.Case.gate is None
    FOOTPRINT[entry](rig("pinned_ld4", 13))
