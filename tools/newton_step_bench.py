"""Same-process A/B timing of the fused Newton-step entry against the three entries it replaces (tool; MEASUREMENTS.md "Newton step"):
  dpfhe_relinearize_lincomb_rescale_hybrid, K = 1, the term one limb above the level
      against  dpfhe_relinearize_hybrid (t into the first term slot) + a strided level-drop copy of the term + dpfhe_lincomb_rescale over [t, term]
  at 8 and 64 items, N = 8192 / Ld = 5 and N = 32768 / Ld = 7.
After a warm-up of every shape the two forms alternate, ROUNDS rounds of REPS back-to-back calls each between two events; per form the median round, the
fastest and the slowest are printed (the spread of the composed form is the noise a difference has to exceed), with a check that both forms gave the same
words and the algorithmic bytes of the last pass in both forms (include/dpfhe.h derives them).  The key products, which both forms run unchanged, dominate the
entry: the last pass alone is read off a kernel trace of the `trace13` / `trace15` modes (relin_lincomb_rescale_kernel against rescale_kernel + the copy +
lincomb_rescale_kernel).
usage: python tools/newton_step_bench.py [rounds = 7] [reps = 10] [all | quick | trace13 | trace15]"""
import ctypes as C
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


def step(ext_params, batch):
    """ext_params: the extended context (Ld data limbs + P).  The term has Ld + 1 limbs: it lives one level up, as y_n does in a Newton step"""
    lib = _cabi.load()
    ext = Context(ext_params, 0)
    data = Context(ext_params.drop_last_limb(), 0)
    dev, L, Ld, n = ext.device, ext_params.n_limbs, ext_params.n_limbs - 1, ext_params.n
    g = torch.Generator(device=dev).manual_seed(11)
    in3 = words(g, ext_params.moduli[:Ld], (batch, 3), n, dev)
    key = words(g, ext_params.moduli, (Ld, 2), n, dev)
    tall = list(ext_params.moduli[:Ld]) + [ext_params.moduli[0]]              # (the limb past Ld is never read by the fused form, and cut by the copy)
    term = words(g, tall, (batch, 2), n, dev)
    q = torch.tensor(ext_params.moduli[:Ld], dtype=torch.int64, device=dev)
    w = torch.randint(0, 2 ** 62, (3, Ld), generator=g, dtype=torch.int64, device=dev) % q
    work = torch.empty((batch, 2, L, n), dtype=torch.int64, device=dev)
    x = torch.empty((2, batch, 2, Ld, n), dtype=torch.int64, device=dev)      # [t, term] term-major, what dpfhe_lincomb_rescale reads
    out_c = torch.empty((batch, 2, Ld - 1, n), dtype=torch.int64, device=dev)
    out_f = torch.empty_like(out_c)
    ptrs, limbs = (C.c_void_p * 1)(term.data_ptr()), (C.c_uint32 * 1)(Ld + 1)

    def composed():
        _cabi.check(lib.dpfhe_relinearize_hybrid(ext.handle, x[0].data_ptr(), in3.data_ptr(), key.data_ptr(), work.data_ptr(), batch, None), "dpfhe_relinearize_hybrid")
        x[1].copy_(term[:, :, :Ld])                                           # the level drop: the first Ld limbs of every polynomial
        _cabi.check(lib.dpfhe_lincomb_rescale(data.handle, out_c.data_ptr(), x.data_ptr(), w.data_ptr(), 2, batch, None), "dpfhe_lincomb_rescale")

    def fused():
        _cabi.check(lib.dpfhe_relinearize_lincomb_rescale_hybrid(ext.handle, out_f.data_ptr(), in3.data_ptr(), key.data_ptr(), work.data_ptr(), ptrs, limbs, 1,
                                                                 w.data_ptr(), batch, None), "dpfhe_relinearize_lincomb_rescale_hybrid")
    ms = alternate({"composed": composed, "fused": fused})
    K = Kc = 1
    rows_fused = 2 * (L + (K + 2) * Ld - 1)                                   # include/dpfhe.h: rows of N words per item
    rows_composed = rows_fused + 4 * (1 + Kc) * Ld
    row = {"entry": "dpfhe_relinearize_lincomb_rescale_hybrid", "log2_n": ext_params.log2_n, "data_limbs": Ld, "terms": K, "batch": batch, "rounds": ROUNDS, "reps": REPS,
           "same_words": bool(torch.equal(out_c, out_f)), "pass_algorithmic_bytes": {"fused": batch * rows_fused * n * 8, "composed": batch * rows_composed * n * 8}}
    for name, v in ms.items():
        row[name + "_ms"] = {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}
    comp, fu = ms["composed"], ms["fused"]
    row["fused_over_composed"] = round(fu[len(fu) // 2] / comp[len(comp) // 2], 4)
    row["composed_spread"] = round((comp[-1] - comp[0]) / comp[len(comp) // 2], 4)
    print(json.dumps(row), flush=True)
    del in3, key, term, work, x, out_c, out_f
    ext.close()
    data.close()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if MODE == "quick":
        step(ntt_primes(12, 4), 4)
    elif MODE == "trace13":
        step(FheParams.n8192_l6(), 64)
    elif MODE == "trace15":
        step(FheParams.n32768(8), 64)
    else:
        for batch in (8, 64):
            step(FheParams.n8192_l6(), batch)
            step(FheParams.n32768(8), batch)
