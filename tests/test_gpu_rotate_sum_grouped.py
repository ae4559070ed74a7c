"""-m gpu: hoisted slot sums on grouped-digit keys (include/dpfhe.h dpfhe_rotate_sum_hoisted_grouped; csrc/kernels_rotate_sum.h), word for word against Python
integers (tests/rotate_sum_grouped_ref.py) on the mixed-class contexts of tests/test_gpu_switch_key_grouped.py and on all-fold contexts of pinned 2^60 - d primes
(the Dot30 lane; ascending, so P >= D_max), and against the device's automorphism + dpfhe_switch_key_grouped + dpfhe_add at one rotation.  N = 256 at every
coefficient, larger rings at that file's sample().  arena_cases() also runs behind the stream gate (tests/test_gpu_stream_contract_rotate_sum_grouped.py)."""
import os
import subprocess

import numpy as np
import pytest

import cpp_build
import remainder_edges as re_
import rotate_sum_grouped_ref as ref
import switch_key_grouped_ref as ks_ref
import test_gpu_footprint as fp
import test_gpu_switch_key_grouped as skg
from class_edges import edge_chain, worst_case
from deeppowers_amd.evaluator import Ciphertext, Context, Evaluator, to_device, to_host
from deeppowers_amd.params import FheParams, ntt_primes
from oracle.cbind import Oracle

pytestmark = pytest.mark.gpu

LA = [(4, 2), (5, 2), (3, 3), (4, 1), (6, 4)]        # even groups; a short last group; one group (J = 1 on the special limbs); alpha = 1; a short group at alpha = 4
RT = [(1, 1), (7, 5), (3, 3), (64, 2)]               # (n_rot, n_items): one of each; a tile + a remainder tile, > 8 terms; a tile of 3 live rows; the cap
# every (Ld, alpha) with two shapes, every shape on both kinds of context; then several segments on both kinds, and the composed transforms
CASES = ([(kind, 8, LA[i], RT[(i + j) % 4]) for i in range(4) for j, kind in enumerate(("mixed", "fold"))] + [("mixed", 8, LA[4], RT[1]), ("fold", 8, LA[4], RT[3])]
         + [("fold", 13, (4, 2), (3, 2)), ("mixed", 13, (5, 2), (2, 1)), ("fold", 14, (4, 2), (2, 1))])
FOOTPRINT = [("mixed", 8, (5, 2)), ("fold", 14, (4, 2))]


class Rig:
    """the extended context of one (kind, log2 N, Ld, alpha), warmed up, its data context and the oracles of both"""

    def __init__(self, kind, log2n, Ld, alpha):
        self.p = skg.params(log2n, Ld, alpha) if kind == "mixed" else edge_chain("fold", log2n, Ld + alpha)
        self.kind, self.Ld, self.alpha, self.L, self.n, self.beta = f"{kind}_{Ld}+{alpha}", Ld, alpha, Ld + alpha, 1 << log2n, -(-Ld // alpha)
        self.orc, self.data = Oracle.from_params(self.p), Oracle(log2n, self.p.moduli[:Ld], self.p.psi[:Ld])
        self.ctx = Context(self.p, 0)
        self.ev, self.dctx = Evaluator(self.ctx), Context(FheParams(log2n, tuple(self.p.moduli[:Ld]), tuple(self.p.psi[:Ld])), 0)
        assert (set(self.ctx.limb_classes) == {"fold"}) == (kind == "fold")
        assert self.ctx._lib.dpfhe_rotate_sum_hoisted_grouped(self.ctx.handle, None, None, 0, alpha, None, None, 1, None, None, None, None) == 0      # the warm-up

    def dev(self, a):
        return to_device(np.ascontiguousarray(a), self.ctx.device)

    def inputs(self, R, T, seed):
        """(R elements, their keys [R][beta][2][L][N], T items with worst-case stripes)"""
        n = self.n
        e = [3, pow(3, -1, 2 * n), 5, n + 1, 2 * n - 1, 2 * n - 3, pow(3, 77, 2 * n), 1, pow(3, n // 4, 2 * n)] + [pow(5, i, 2 * n) for i in range(2, R)]
        cts = worst_case(self.data.fill(T * 2, seed).reshape(T, 2, self.Ld, n), np.array(self.data.moduli, np.uint64)[:, None], n)
        return e[:R], self.orc.fill(R * self.beta * 2, seed + 1).reshape(R, self.beta, 2, self.L, n), cts

    def run(self, cts, elts, keys):
        return to_host(self.ev.rotate_sum_hoisted_grouped(Ciphertext(self.dev(cts)), elts, self.dev(keys), self.alpha).data)

    def check(self, got, cts, elts, keys):
        for t, ct in enumerate(cts):
            want = ref.divide_and_add(ref.sum_qp(self.orc, self.data, ct, elts, keys, self.Ld, self.alpha), ct, self.p.moduli, self.Ld, skg.sample(self.n))
            for (comp, k), words in want.items():
                assert [int(w) for w in got[t, comp, :, k]] == words, (self.kind, self.n, t, comp, k)


@pytest.fixture(scope="module")
def rigs():
    made = {}
    yield lambda *key: made.get(key) or made.setdefault(key, Rig(key[0], key[1], *key[2]))
    for r in made.values():
        r.ctx.close()
        r.dctx.close()


@pytest.mark.parametrize("kind,log2n,la,rt", CASES, ids=[f"{k}_n{1 << ln}_{la[0]}+{la[1]}_r{rt[0]}x{rt[1]}" for k, ln, la, rt in CASES])
def test_words_equal_python_integers(rigs, kind, log2n, la, rt):
    r = rigs(kind, log2n, la)
    elts, keys, cts = r.inputs(*rt, 920 + log2n)
    got = r.run(cts, elts, keys)
    r.check(got, cts, elts, keys)
    if rt[0] == 1:      # on the device: the automorphism, dpfhe_switch_key_grouped with 2 components, dpfhe_add of the input - the whole buffer
        dev = Evaluator(r.dctx)
        switched = r.ev.switch_key_grouped(Ciphertext(dev.apply_galois_words(r.dev(cts), elts[0])), r.dev(keys[0]), r.alpha).data
        assert np.array_equal(got, to_host(dev.add_words(switched, r.dev(cts))))


def test_adversarial_keys_fill_the_lazy_sums(rigs):
    """fold, N = 8192, nine rotations of one item: rotation g's key is perm_g of a key under which every product with the item's transformed group digits is
    q - 1, so every product the Dot30 columns take lazily is the largest canonical word (tests/test_gpu_rotate_sum.py's case, on group digits)"""
    r = rigs("fold", 13, (4, 2))
    (elts, _, cts), orc = r.inputs(9, 1, 930), r.orc
    x, rnd = orc.ntt_fwd(ks_ref.lift(cts[0, 1], r.p.moduli, r.Ld, r.alpha), threads=0), orc.fill(r.beta, 931)
    key, zero = re_.key_for_targets(orc, x, re_.constant(orc, (r.beta, 2), lambda q: q - 1), np.stack([rnd, rnd], axis=1))
    assert int(zero.sum()) < 4
    keys = np.stack([orc.ntt_fwd(orc.apply_galois(orc.ntt_inv(key, threads=0), g), threads=0) for g in elts])
    r.check(r.run(cts, elts, keys), cts, elts, keys)


def arena_cases(r, shapes=((3, 1), (5, 5))):
    """every buffer carved out of one arena at 16-byte alignment between guard bands, scratch at exactly the header's sizes; the expected words are the
    device's own from plain buffers (held to Python integers above)"""
    lib, h, L, n, Ld, G = r.ctx._lib, r.ctx.handle, r.L, r.n, r.Ld, r.beta
    for R, T in shapes:
        elts, keys, cts = r.inputs(R, T, 940)
        c = fp.Case(r)
        c.inp("in2", cts, 2 * Ld * n)
        c.inp("keys", keys, G * 2 * L * n)
        for name, item in (("in_ntt", 2 * Ld * n), ("digits", G * L * n), ("sum_qp", 2 * L * n)):
            c.scratch(name, T * item, item)
        c.out("out2", T * 2 * Ld * n, 2 * Ld * n, r.run(cts, elts, keys))
        c.run(f"dpfhe_rotate_sum_hoisted_grouped {Ld}+{r.alpha}, {R} rotations x{T}", lambda at: lib.dpfhe_rotate_sum_hoisted_grouped(
            h, at("out2"), at("in2"), T, r.alpha, fp.u32(elts), at("keys"), R, at("in_ntt"), at("digits"), at("sum_qp"), at.stream))


def test_footprint(rigs):
    for shape in FOOTPRINT:
        arena_cases(rigs(*shape))


def test_device_entry_rejects_bad_arguments(rigs):
    import torch
    r = rigs("mixed", 8, (5, 2))
    lib, L, Ld, n, G = r.ctx._lib, r.L, r.Ld, r.n, r.beta
    fill = lambda *s: torch.full(s, 7, dtype=torch.int64, device=r.ctx.device)
    t = {"out": fill(1, 2, Ld, n), "in": fill(1, 2, Ld, n), "keys": fill(65, G, 2, L, n), "in_ntt": fill(1, 2, Ld, n), "digits": fill(1, G, L, n), "sum_qp": fill(1, 2, L, n)}
    a = dict({k: v.data_ptr() for k, v in t.items()}, elts=fp.u32([3] * 65), n_rot=2, alpha=r.alpha, items=1, h=r.ctx.handle)

    def call(**kw):
        b = dict(a, **kw)
        return lib.dpfhe_rotate_sum_hoisted_grouped(b["h"], b["out"], b["in"], b["items"], b["alpha"], b["elts"], b["keys"], b["n_rot"], b["in_ntt"], b["digits"], b["sum_qp"], None)
    table = [dict(alpha=0), dict(alpha=11), dict(alpha=L), dict(n_rot=0), dict(n_rot=65), dict(elts=fp.u32([3, 4])), dict(elts=fp.u32([2 * n + 1, 3])), dict(items=1 << 40),
             dict(out=a["in"]), dict(sum_qp=a["digits"]), dict(in_ntt=a["in"]), dict(digits=a["keys"])] + [{k: a[k] + 8} for k in t] + [{k: None} for k in t]
    assert [call(**kw) for kw in table] == [2000] * len(table)
    narrow = Context(FheParams(8, tuple(reversed(r.p.moduli[Ld - 1:Ld + 1])), tuple(reversed(r.p.psi[Ld - 1:Ld + 1]))), 0)      # P below the one data prime
    wide = Context(ntt_primes(8, 21), 0)                                                            # more limbs than a BaseExtArgs has destinations
    assert call(h=narrow.handle, alpha=1) == 2002 and call(h=wide.handle, items=0) == 2000 and call(items=0) == 0
    narrow.close(), wide.close()
    torch.cuda.synchronize()
    assert bool((t["out"] == 7).all())                                              # every refusal left the output untouched
    assert call(**{"in": a["keys"]}) == 0                                           # the input and the keys are only read: they may overlap
    torch.cuda.synchronize()


def test_cpp_slot_sum_grouped_facade():
    """tests/cpp/slot_sum_grouped/test_slot_sum_grouped_api.cpp, once: SlotSum over a GroupedKeySwitcher at N = 4096 within the header's error_bound"""
    os.makedirs(os.path.join(cpp_build.BIN_DIR, "slot_sum_grouped"), exist_ok=True)
    out = subprocess.run([cpp_build.build_program("slot_sum_grouped/test_slot_sum_grouped_api")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("slot sum grouped C++ facade OK"), out.stdout[-4000:] + out.stderr[-2000:]
