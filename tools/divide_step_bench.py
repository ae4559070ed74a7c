"""Same-process A/B timing of a Goldschmidt division step against its composition on the older entries (tool; MEASUREMENTS.md "Division steps"):
  (a) dpfhe_ct_mul_complement (coefficient domain in and out)
          against  dpfhe_negate on the denominators + dpfhe_add_plain of the constant + the factor copied out per item (two broadcasting device copies) +
          dpfhe_ct_mul over all G (T + 1) pairs - the same words, asserted;
  (b) dpfhe_ct_mul_complement + dpfhe_relinearize_rescale_hybrid over all products (HybridKeySwitcher::multiply_complement_rescale_range)
          against  that composition + dpfhe_relinearize_rescale_hybrid - the same words, asserted
  at N = 32768 and N = 16384 on 7 data limbs + P, G = 8 groups of T = 8 numerators, with the self product.
After a warm-up the two forms alternate, ROUNDS rounds of REPS back-to-back calls each between two events; per form the median round, the fastest and the
slowest are printed (the spread of the baseline is the noise a difference has to exceed).  Counts: the entry runs 2 (T + 1) forward and 3 (T + 1) inverse
transforms per group and limb, the composition 4 (T + 1) and 3 (T + 1): 5/7 of the transforms.
The `trace15` mode runs part (a) of the larger shape alone, for a kernel trace.
usage: python tools/divide_step_bench.py [rounds = 7] [reps = 10] [all | quick | trace15]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deeppowers_amd import _cabi  # noqa: E402
from deeppowers_amd.evaluator import Context  # noqa: E402
from deeppowers_amd.params import FheParams, ntt_primes  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
MODE = sys.argv[3] if len(sys.argv) > 3 else "all"


def words(gen, moduli, lead, n, dev):
    q = torch.tensor(moduli, dtype=torch.int64, device=dev).view(-1, 1)
    return torch.randint(0, 2 ** 62, tuple(lead) + (len(moduli), n), generator=gen, dtype=torch.int64, device=dev) % q


def alternate(forms):
    """forms: name -> callable enqueueing one call.  -> name -> sorted milliseconds per call, one per round"""
    for f in forms.values():
        f()
        f()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(ROUNDS):
        for name, f in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                f()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / REPS)
    return {name: sorted(v) for name, v in ms.items()}


def report(row, ms, base, new):
    for name, v in ms.items():
        row[name + "_ms"] = {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}
    b, f = ms[base], ms[new]
    row[f"{new}_over_{base}"] = round(f[len(f) // 2] / b[len(b) // 2], 4)
    row[f"{base}_spread"] = round((b[-1] - b[0]) / b[len(b) // 2], 4)
    print(json.dumps(row), flush=True)


def shape(ext_params, groups, terms, parts="ab"):
    """ext_params: the extended context (Ld data limbs + P)"""
    lib = _cabi.load()
    ext = Context(ext_params, 0)
    data_params = ext_params.drop_last_limb()
    data = Context(data_params, 0)
    dev, L, Ld, n = ext.device, ext_params.n_limbs, ext_params.n_limbs - 1, ext_params.n
    G, T = groups, terms
    items = G * T + G
    g = torch.Generator(device=dev).manual_seed(17)
    a = words(g, data_params.moduli, (G, T, 2), n, dev)
    b = words(g, data_params.moduli, (G, 2), n, dev)
    key = words(g, ext_params.moduli, (Ld, 2), n, dev)
    kappa_int = (1 << 61) - 12345
    kappa = torch.tensor([kappa_int % q for q in data_params.moduli], dtype=torch.int64, device=dev)
    constant = torch.zeros((1, Ld, n), dtype=torch.int64, device=dev)        # kappa X^0, coefficient domain
    constant[0, :, 0] = kappa
    z = lambda *s: torch.empty(s, dtype=torch.int64, device=dev)
    out_new, out_old = z(items, 3, Ld, n), z(items, 3, Ld, n)
    factor, lhs, rhs = z(G, 2, Ld, n), z(items, 2, Ld, n), z(items, 2, Ld, n)
    p = lambda t: t.data_ptr()
    base = {"log2_n": ext_params.log2_n, "data_limbs": Ld, "terms": T, "groups": G, "with_self": True, "rounds": ROUNDS, "reps": REPS}
    # the composition's left operands do not change between calls: the numerators group-major, then the denominators (laid out once, not timed)
    lhs[:G * T].copy_(a.view(G * T, 2, Ld, n))
    lhs[G * T:].copy_(b)
    rhs_num, rhs_self, factor_bc = rhs[:G * T].view(G, T, 2, Ld, n), rhs[G * T:], factor.view(G, 1, 2, Ld, n).expand(G, T, 2, Ld, n)

    def complement():
        _cabi.check(lib.dpfhe_ct_mul_complement(data.handle, p(out_new), p(a), p(b), p(kappa), G, T, 1, 0, None), "dpfhe_ct_mul_complement")

    def composition():
        _cabi.check(lib.dpfhe_negate(data.handle, p(factor), p(b), G * 2, None), "dpfhe_negate")      # (counts RNS polynomials: 2 per ciphertext)
        _cabi.check(lib.dpfhe_add_plain(data.handle, p(factor), p(factor), p(constant), G, 2, 1, 0, None), "dpfhe_add_plain")
        rhs_num.copy_(factor_bc)                                              # the factor copied out per item, in the fewest launches there are: one
        rhs_self.copy_(factor)                                                # broadcasting copy for the G T numerators, one for the G self products
        _cabi.check(lib.dpfhe_ct_mul(data.handle, p(out_old), p(lhs), p(rhs), items, 0, None), "dpfhe_ct_mul")

    if "a" in parts:
        ms = alternate({"composition": composition, "complement": complement})
        same = bool(torch.equal(out_new, out_old))
        rows_new, rows_old = 2 * T + 2 + 3 * (T + 1), 7 * (T + 1)             # include/dpfhe.h: rows of N words per group and limb of the tensor pass
        report(dict(base, part="a", entry="dpfhe_ct_mul_complement", same_words=same,
                    forward_transforms_per_group_and_limb={"complement": 2 * (T + 1), "composition": 4 * (T + 1)},
                    tensor_pass_algorithmic_bytes={"complement": G * Ld * rows_new * n * 8, "composition": G * Ld * rows_old * n * 8}), ms, "composition", "complement")
        assert same, "dpfhe_ct_mul_complement and the composition gave different words"

    if "b" in parts:
        work = z(items, 2, L, n)
        step_new, step_old = z(items, 2, Ld - 1, n), z(items, 2, Ld - 1, n)

        def complement_step():
            complement()
            _cabi.check(lib.dpfhe_relinearize_rescale_hybrid(ext.handle, p(step_new), p(out_new), p(key), p(work), items, None), "dpfhe_relinearize_rescale_hybrid")

        def composition_step():
            composition()
            _cabi.check(lib.dpfhe_relinearize_rescale_hybrid(ext.handle, p(step_old), p(out_old), p(key), p(work), items, None), "dpfhe_relinearize_rescale_hybrid")
        ms = alternate({"composition_step": composition_step, "complement_step": complement_step})
        same = bool(torch.equal(step_new, step_old))
        report(dict(base, part="b", entry="multiply_complement_rescale_range", same_words=same, key_switches=items), ms, "composition_step", "complement_step")
        assert same, "the step and the composition gave different words"
    torch.cuda.empty_cache()
    for c in (data, ext):
        c.close()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if MODE == "quick":
        shape(ntt_primes(12, 4), 2, 3)
    elif MODE == "trace15":
        shape(FheParams.n32768(8), 8, 8, parts="a")
    else:
        for params in (FheParams.n32768(8), ntt_primes(14, 8)):
            shape(params, 8, 8)
