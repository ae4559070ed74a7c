"""-m gpu: hybrid key switching with grouped digits and several special primes (include/dpfhe.h dpfhe_switch_key_grouped; csrc/keyswitch_grouped.h, workmap.h
GroupedKsMap), word for word against Python integers (tests/switch_key_grouped_ref.py) and against the six-entry composition the header names, on the same device.
One mixed-class context per shape: data limbs of 17 to 51 bits of the narrow classes under special primes of 59 and 60 bits, so the generic arithmetic of the two
new kernels meets narrow primes and P >= D_max holds at every alpha.  Above N = 256 the Python reference is compared at the first and last 64 coefficients and a
stride of 211; the composition is compared everywhere.  arena_cases() is what tests/test_gpu_stream_contract_switch_key_grouped.py runs behind the stream gate;
the decryption semantics are held through the C++ facade's own keys (tests/test_gpu_switch_key_grouped_facade.py)."""
import numpy as np
import pytest

import switch_key_grouped_ref as ref
import test_gpu_footprint as fp
from class_edges import catalogue, worst_case
from deeppowers_amd.evaluator import Ciphertext, Context, Evaluator, to_device, to_host
from deeppowers_amd.params import FheParams, ntt_primes
from oracle.cbind import Oracle

pytestmark = pytest.mark.gpu

SHAPES = [(4, 2), (5, 2), (5, 3), (3, 3), (4, 1), (6, 4)]       # even groups; a short last group of 1 and of 2; one group only; alpha = 1; a short group at alpha = 4
DATA = ["f64_edge", "fscaled_edge_50", "shoup_above_50", "smallest", "f64_wide_low", "f64_wide_edge", "fscaled_edge_49", "fscaled_edge_48"]
SPECIAL = ["fold_edge", "shoup60", "fscaled_edge_59", "shoup_above_59"]


def params(log2n, Ld, alpha):
    cat = catalogue(log2n)
    take = lambda names, count: [cat[name][i] for i in range(2) for name in names if name in cat and len(cat[name]) > i][:count]   # (a band may hold no prime at this N)
    ps = take(DATA, Ld) + take(SPECIAL, alpha)
    assert len(ps) == Ld + alpha and len({q for q, _ in ps}) == len(ps)
    return FheParams(log2n, tuple(q for q, _ in ps), tuple(w for _, w in ps))


class Grouped:
    """the extended context of one (log2 N, Ld, alpha), its data context, three items of three components, a uniform key, and the reference's key products"""

    def __init__(self, log2n, Ld, alpha, items=3):
        self.p, self.Ld, self.alpha, self.kind = params(log2n, Ld, alpha), Ld, alpha, f"grouped_{Ld}+{alpha}"
        self.L, self.n, self.groups = Ld + alpha, 1 << log2n, len(ref.groups(Ld, alpha))
        self.orc = Oracle.from_params(self.p)
        self.data = Oracle(log2n, self.p.moduli[:Ld], self.p.psi[:Ld])
        self.ctx = Context(self.p, 0)
        self.ev = Evaluator(self.ctx)
        self.dctx = Context(FheParams(log2n, tuple(self.p.moduli[:Ld]), tuple(self.p.psi[:Ld])), 0)
        assert len(set(self.ctx.limb_classes)) > 1
        self.ct = worst_case(self.data.fill(items * 3, 910 + log2n).reshape(items, 3, Ld, self.n), np.array(self.data.moduli, np.uint64)[:, None], self.n)
        self.key = self.orc.fill(self.groups * 2, 911).reshape(self.groups, 2, self.L, self.n)
        self._work = {}

    def dev(self, a):
        return to_device(np.ascontiguousarray(a), self.ctx.device)

    def work(self, t):
        """INTT(sum_d NTT(digit_d of item t's component 2) (.) key_d), by the reference"""
        if t not in self._work:
            self._work[t] = ref.key_products(self.orc, ref.lift(self.ct[t, 2], self.p.moduli, self.Ld, self.alpha), self.key)
        return self._work[t]

    def close(self):
        self.ctx.close()
        self.dctx.close()


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(log2n, Ld, alpha):
        if (log2n, Ld, alpha) not in made:
            made[log2n, Ld, alpha] = Grouped(log2n, Ld, alpha)
        return made[log2n, Ld, alpha]
    yield get
    for c in made.values():
        c.close()


def sample(n):
    return list(range(n)) if n <= 256 else sorted(set(range(64)) | set(range(n - 64, n)) | set(range(0, n, 211)))


def run(c, ct, key):
    return to_host(c.ev.switch_key_grouped(Ciphertext(c.dev(ct)), c.dev(key), c.alpha).data)


def check_reference(c, got, ct, work_of, at):
    for t in range(ct.shape[0]):
        for (comp, k), words in ref.divide_and_add(work_of(t), ct[t], c.p.moduli, c.Ld, at).items():
            assert [int(w) for w in got[t, comp, :, k]] == words, (c.kind, c.n, t, comp, k)


def composition(c, ct, key):
    """dpfhe_base_extend per group -> dpfhe_ntt_fwd -> dpfhe_dyadic_mul / _mul_add -> dpfhe_ntt_inv -> dpfhe_scale_round -> dpfhe_add"""
    import torch
    ev, batch, comps = c.ev, ct.shape[0], ct.shape[1]
    sw, dkey = c.dev(ct[:, -1]), c.dev(key)
    lifted = torch.stack([ev.base_extend(sw[:, g.start:g.stop].contiguous(), g.start, 0, c.L) for g in ref.groups(c.Ld, c.alpha)], dim=1).contiguous()
    x = ev.ntt_forward(lifted)
    acc = torch.empty((batch, 2, c.L, c.n), dtype=torch.int64, device=c.ctx.device)
    for comp in range(2):
        a = None
        for d in range(c.groups):
            xd, kd = x[:, d].contiguous(), dkey[d, comp].expand(batch, c.L, c.n).contiguous()
            a = ev.dyadic_mul(xd, kd) if a is None else ev.dyadic_mul_add_(a, xd, kd)
        acc[:, comp] = a
    r = ev.scale_round(ev.ntt_inverse(acc), c.Ld, c.alpha, 0, c.Ld, 1)
    addend = np.zeros((batch, 2, c.Ld, c.n), np.uint64)
    addend[:, :comps - 1] = ct[:, :comps - 1]
    return to_host(Evaluator(c.dctx).add_words(r, c.dev(addend)))


@pytest.mark.parametrize("batch", (1, 3))
@pytest.mark.parametrize("comps", (2, 3))
@pytest.mark.parametrize("Ld,alpha", SHAPES, ids=[f"{a}+{b}" for a, b in SHAPES])
@pytest.mark.parametrize("log2n", (8, 13, 14))
def test_words_equal_python_integers_and_the_composition(cases, log2n, Ld, alpha, comps, batch):
    c = cases(log2n, Ld, alpha)
    ct = np.ascontiguousarray(c.ct[:batch] if comps == 3 else c.ct[:batch][:, [0, 2]])      # component 2 is the switched one either way
    got = run(c, ct, c.key)
    check_reference(c, got, ct, c.work, sample(c.n))
    want = composition(c, ct, c.key)
    assert np.array_equal(got, want), (np.argwhere(got != want)[:4])


def test_planted_edges(cases):
    """item 0: every group's centred digit is D / 2, -(D / 2), -(D / 2) + 1, 0, 1 and -1 at coefficients 0 .. 5; item 1: c = 1 and a key whose group 0 is the
    transform of chosen integers X = m P + r over Q P (the other groups are zero), so the sum the division sees has r in {0, 1, P / 2, P / 2 + 1, P - 1}"""
    c = cases(8, 5, 2)
    q, P, n = c.p.moduli, ref.product(c.p.moduli[c.Ld:]), c.n
    ct = np.array(c.ct[:2])
    for g in ref.groups(c.Ld, c.alpha):
        D = ref.product(q[i] for i in g)
        for k, v in enumerate((D // 2, -(D // 2), -(D // 2) + 1, 0, 1, -1)):
            for i in g:
                ct[0, 2, i, k] = v % q[i]
    planted = ref.digits(ct[0, 2], q, c.Ld, c.alpha)
    assert all(xd[:6] == [D // 2, -(D // 2), -(D // 2) + 1, 0, 1, -1] for xd, D in zip(planted, (ref.product(q[i] for i in g) for g in ref.groups(c.Ld, c.alpha))))
    got = run(c, ct[:1], c.key)
    work0 = ref.key_products(c.orc, ref.lift(ct[0, 2], q, c.Ld, c.alpha), c.key)
    check_reference(c, got, ct[:1], lambda t: work0, list(range(n)))

    rng = np.random.default_rng(77)
    edges = (0, 1, P // 2, P // 2 + 1, P - 1)
    Q = ref.product(q[:c.Ld])
    X = [[int(rng.integers(0, 1 << 62)) % Q * P + edges[(k + comp) % 5] for k in range(n)] for comp in range(2)]
    key = np.zeros_like(c.key)
    key[0] = c.orc.ntt_fwd(np.array([[[x % int(m) for x in X[comp]] for m in q] for comp in range(2)], np.uint64))
    ct[1, 2] = 0
    ct[1, 2, :, 0] = 1
    work1 = ref.key_products(c.orc, ref.lift(ct[1, 2], q, c.Ld, c.alpha), key)
    assert ref.crt(list(work1[0]), q)[:5] == [x % (Q * P) for x in X[0][:5]]        # the sum is the chosen one
    got = run(c, ct[1:2], key)
    check_reference(c, got, ct[1:2], lambda t: work1, list(range(n)))


def arena_cases(c, items=2):
    """every buffer carved out of one arena at 16-byte alignment between guard bands, scratch at exactly the header's sizes; the expected words in Python integers"""
    lib, h, L, Ld, n, G = c.ctx._lib, c.ctx.handle, c.L, c.Ld, c.n, c.groups
    for comps in (2, 3):
        ct = np.ascontiguousarray(c.ct[:items] if comps == 3 else c.ct[:items][:, [0, 2]])
        want = np.zeros((items, 2, Ld, n), np.uint64)
        for t in range(items):
            for (comp, k), words in ref.divide_and_add(c.work(t), ct[t], c.p.moduli, Ld, list(range(n))).items():
                want[t, comp, :, k] = words
        case = fp.Case(c)
        case.inp("in", ct, comps * Ld * n)
        case.inp("key", c.key, 2 * L * n)
        case.scratch("digits", items * G * L * n, G * L * n)
        case.scratch("work", items * 2 * L * n, 2 * L * n)
        case.out("out2", items * 2 * Ld * n, 2 * Ld * n, want)
        case.run(f"dpfhe_switch_key_grouped {Ld}+{c.alpha}, {comps} components x{items}",
                 lambda at: lib.dpfhe_switch_key_grouped(h, at("out2"), at("in"), comps, c.alpha, at("key"), at("digits"), at("work"), items, at.stream))


FOOTPRINT = [(8, 5, 2), (14, 4, 2)]


def test_device_entry_rejects_bad_arguments(cases):
    import torch
    c = cases(8, 5, 2)
    lib, h, L, Ld, n, G = c.ctx._lib, c.ctx.handle, c.L, c.Ld, c.n, c.groups
    fill = lambda *s: torch.full(s, 7, dtype=torch.int64, device=c.ctx.device)
    t = {"out": fill(1, 2, Ld, n), "in": fill(1, 3, Ld, n), "key": fill(G, 2, L, n), "digits": fill(1, G, L, n), "work": fill(1, 2, L, n)}
    a = dict({k: v.data_ptr() for k, v in t.items()}, comps=3, alpha=c.alpha, batch=1)

    def call(handle=h, **kw):
        b = dict(a, **kw)
        return lib.dpfhe_switch_key_grouped(handle, b["out"], b["in"], b["comps"], b["alpha"], b["key"], b["digits"], b["work"], b["batch"], None)
    table = [dict(alpha=0), dict(alpha=11), dict(alpha=L), dict(comps=1), dict(comps=4), dict(batch=1 << 40),
             dict(out=a["in"]), dict(work=a["digits"]), dict(digits=a["key"]), dict(out=a["work"])]
    table += [{name: a[name] + 8} for name in t] + [{name: None} for name in t]
    for kw in table:
        assert call(**kw) == 2000, kw
    narrow = Context(FheParams(8, tuple(reversed(c.p.moduli[Ld - 1:Ld + 1])), tuple(reversed(c.p.psi[Ld - 1:Ld + 1]))), 0)      # P below the one data prime
    code = lib.dpfhe_switch_key_grouped(narrow.handle, a["out"], a["in"], 3, 1, a["key"], a["digits"], a["work"], 1, None)
    narrow.close()
    wide = ntt_primes(8, 21)                                                                     # more limbs than a BaseExtArgs has destinations
    wide = Context(wide, 0)
    assert lib.dpfhe_switch_key_grouped(wide.handle, a["out"], a["in"], 3, 2, a["key"], a["digits"], a["work"], 0, None) == 2000
    wide.close()
    torch.cuda.synchronize()
    assert code == 2002 and call(batch=0) == 0 and bool((t["out"] == 7).all())      # every refusal left the output untouched
