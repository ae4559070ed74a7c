"""Same-process A/B timing of the sum of ciphertext products against what it replaces (tool; MEASUREMENTS.md "Sums of products"):
  (a) dpfhe_ct_mul_sum (coefficient domain in and out)
          against  dpfhe_ct_mul(DPFHE_OUT_NTT) over all pairs + dpfhe_reduce_sum per group + dpfhe_ntt_inv - the same words;
  (b) dpfhe_ct_mul_sum + dpfhe_relinearize_rescale_hybrid over the groups (HybridKeySwitcher::multiply_sum_rescale_range)
          against  `terms` separate product steps - dpfhe_ct_mul + dpfhe_relinearize_rescale_hybrid over all pairs in one batch - plus their additions
          (dpfhe_reduce_sum per group on the next level).  The words differ in the roundings (one against `terms`): times only.
  at N = 8192 / Ld = 5 and N = 32768 / Ld = 7, terms in {4, 8, 64}, groups in {1, 8}.
After a warm-up of every shape the two forms alternate, ROUNDS rounds of REPS back-to-back calls each between two events; per form the median round, the
fastest and the slowest are printed (the spread of the baseline is the noise a difference has to exceed), and (a) asserts that both forms gave the same words.
The `trace13` / `trace15` modes run one shape (terms 8, groups 8) for a kernel trace.
usage: python tools/product_sum_bench.py [rounds = 7] [reps = 10] [all | quick | trace13 | trace15]"""
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


def shape(ext_params, groups, terms):
    """ext_params: the extended context (Ld data limbs + P)"""
    lib = _cabi.load()
    ext = Context(ext_params, 0)
    data_params = ext_params.drop_last_limb()
    data = Context(data_params, 0)
    nxt = Context(data_params.drop_last_limb(), 0)
    dev, L, Ld, n = ext.device, ext_params.n_limbs, ext_params.n_limbs - 1, ext_params.n
    G, K = groups, terms
    g = torch.Generator(device=dev).manual_seed(13)
    a = words(g, data_params.moduli, (G, K, 2), n, dev)
    b = words(g, data_params.moduli, (G, K, 2), n, dev)
    key = words(g, ext_params.moduli, (Ld, 2), n, dev)
    z = lambda *s: torch.empty(s, dtype=torch.int64, device=dev)
    sum_new, sum_old, prods = z(G, 3, Ld, n), z(G, 3, Ld, n), z(G, K, 3, Ld, n)
    p = lambda t: t.data_ptr()
    base = {"log2_n": ext_params.log2_n, "data_limbs": Ld, "terms": K, "groups": G, "rounds": ROUNDS, "reps": REPS}

    # ---- (a) the tensor products summed: one entry against three
    def mul_sum():
        _cabi.check(lib.dpfhe_ct_mul_sum(data.handle, p(sum_new), p(a), p(b), G, K, G, 0, None), "dpfhe_ct_mul_sum")

    def three_calls():
        _cabi.check(lib.dpfhe_ct_mul(data.handle, p(prods), p(a), p(b), G * K, _cabi.OUT_NTT, None), "dpfhe_ct_mul")
        for i in range(G):
            _cabi.check(lib.dpfhe_reduce_sum(data.handle, p(sum_old[i]), p(prods[i]), K, 3, None), "dpfhe_reduce_sum")
        _cabi.check(lib.dpfhe_ntt_inv(data.handle, p(sum_old), G * 3, None), "dpfhe_ntt_inv")
    ms = alternate({"three_calls": three_calls, "mul_sum": mul_sum})
    same = bool(torch.equal(sum_new, sum_old))
    rows_new, rows_old = 4 * K + 3, 10 * K + 3                                 # include/dpfhe.h: rows of N words per group and limb of the tensor pass
    report(dict(base, part="a", entry="dpfhe_ct_mul_sum", same_words=same,
                tensor_pass_algorithmic_bytes={"mul_sum": G * Ld * rows_new * n * 8, "three_calls": G * Ld * rows_old * n * 8}), ms, "three_calls", "mul_sum")
    assert same, "dpfhe_ct_mul_sum and the three-call composition gave different words"

    # ---- (b) the whole step: one key switch and one rounding per group against one per pair
    work = z(G * K, 2, L, n)
    prod_c = z(G * K, 3, Ld, n)
    each = z(G, K, 2, Ld - 1, n)
    out_old, out_new = z(G, 2, Ld - 1, n), z(G, 2, Ld - 1, n)

    def sum_step():
        _cabi.check(lib.dpfhe_ct_mul_sum(data.handle, p(sum_new), p(a), p(b), G, K, G, 0, None), "dpfhe_ct_mul_sum")
        _cabi.check(lib.dpfhe_relinearize_rescale_hybrid(ext.handle, p(out_new), p(sum_new), p(key), p(work), G, None), "dpfhe_relinearize_rescale_hybrid")

    def separate_steps():
        _cabi.check(lib.dpfhe_ct_mul(data.handle, p(prod_c), p(a), p(b), G * K, 0, None), "dpfhe_ct_mul")
        _cabi.check(lib.dpfhe_relinearize_rescale_hybrid(ext.handle, p(each), p(prod_c), p(key), p(work), G * K, None), "dpfhe_relinearize_rescale_hybrid")
        for i in range(G):
            _cabi.check(lib.dpfhe_reduce_sum(nxt.handle, p(out_old[i]), p(each[i]), K, 2, None), "dpfhe_reduce_sum")
    ms = alternate({"separate_steps": separate_steps, "sum_step": sum_step})
    report(dict(base, part="b", entry="multiply_sum_rescale_range", key_switches={"sum_step": G, "separate_steps": G * K}), ms, "separate_steps", "sum_step")
    del a, b, key, sum_new, sum_old, prods, work, prod_c, each, out_old, out_new
    torch.cuda.empty_cache()
    for c in (nxt, data, ext):
        c.close()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if MODE == "quick":
        shape(ntt_primes(12, 4), 2, 5)
    elif MODE == "trace13":
        shape(FheParams.n8192_l6(), 8, 8)
    elif MODE == "trace15":
        shape(FheParams.n32768(8), 8, 8)
    else:
        for params in (FheParams.n8192_l6(), FheParams.n32768(8)):
            for K in (4, 8, 64):
                for G in (1, 8):
                    shape(params, G, K)
