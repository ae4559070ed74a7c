"""Same-process A/B timing of the fused rescales against the entries they replace (tool; MEASUREMENTS.md "Fused rescales"):
  dpfhe_relinearize_rescale_hybrid            against  dpfhe_relinearize_hybrid + dpfhe_rescale      (N = 8192, Ld = 5, batch 64; N = 32768, Ld = 6, batch 8)
  dpfhe_lincomb_rescale (K = 4, 15; T = 8)    against  one K-column dpfhe_matvec_scalar per token + dpfhe_rescale
After a warm-up of every shape the two forms alternate, ROUNDS rounds of REPS back-to-back calls each between two events; per form the median round, the
fastest and the slowest are printed (the spread of the composed form is the noise a difference has to exceed), with a check that both forms gave the same
words, the algorithmic bytes of each new pass, and dpfhe_copy's rate on a buffer of the same size in the same run.
usage: python tools/fused_rescale_bench.py [rounds = 7] [reps = 10] [quick | relin13 | relin15]
       (quick: one small shape of each kind, a rehearsal; relin13 / relin15: that relinearisation shape alone, for a kernel trace of its last pass)"""
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


def report(what, shape, ms, same, pass_bytes, copy_ms, copy_bytes):
    row = {"entry": what, **shape, "rounds": ROUNDS, "reps": REPS, "same_words": bool(same), "pass_algorithmic_bytes": pass_bytes,
           "copy_gb_per_s": round(copy_bytes / copy_ms[len(copy_ms) // 2] / 1e6, 1)}
    for name, v in ms.items():
        row[name + "_ms"] = {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}
    comp, fused = ms["composed"], ms["fused"]
    row["fused_over_composed"] = round(fused[len(fused) // 2] / comp[len(comp) // 2], 4)
    row["composed_spread"] = round((comp[-1] - comp[0]) / comp[len(comp) // 2], 4)
    print(json.dumps(row), flush=True)


def copy_rate(lib, ctx, n_words):
    src = torch.zeros(n_words, dtype=torch.int64, device=ctx.device)
    dst = torch.empty_like(src)
    return alternate({"copy": lambda: _cabi.check(lib.dpfhe_copy(ctx.handle, dst.data_ptr(), src.data_ptr(), n_words, None), "dpfhe_copy")})["copy"]


def relin(ext_params, batch):
    lib = _cabi.load()
    ext = Context(ext_params, 0)
    data = Context(ext_params.drop_last_limb(), 0)
    dev, L, Ld, n = ext.device, ext_params.n_limbs, ext_params.n_limbs - 1, ext_params.n
    g = torch.Generator(device=dev).manual_seed(7)
    in3 = words(g, ext_params.moduli[:Ld], (batch, 3), n, dev)
    key = words(g, ext_params.moduli, (Ld, 2), n, dev)
    work = torch.empty((batch, 2, L, n), dtype=torch.int64, device=dev)
    mid = torch.empty((batch, 2, Ld, n), dtype=torch.int64, device=dev)
    out_c = torch.empty((batch, 2, Ld - 1, n), dtype=torch.int64, device=dev)
    out_f = torch.empty_like(out_c)

    def composed():
        _cabi.check(lib.dpfhe_relinearize_hybrid(ext.handle, mid.data_ptr(), in3.data_ptr(), key.data_ptr(), work.data_ptr(), batch, None), "dpfhe_relinearize_hybrid")
        _cabi.check(lib.dpfhe_rescale(data.handle, out_c.data_ptr(), mid.data_ptr(), batch * 2, None), "dpfhe_rescale")

    def fused():
        _cabi.check(lib.dpfhe_relinearize_rescale_hybrid(ext.handle, out_f.data_ptr(), in3.data_ptr(), key.data_ptr(), work.data_ptr(), batch, None),
                    "dpfhe_relinearize_rescale_hybrid")
    ms = alternate({"composed": composed, "fused": fused})
    pass_bytes = batch * 2 * n * (L + Ld + Ld - 1) * 8          # the Q P sums on all L limbs and (c0, c1) on Ld, read once; Ld - 1 limbs written
    report("dpfhe_relinearize_rescale_hybrid", {"log2_n": ext_params.log2_n, "data_limbs": Ld, "batch": batch}, ms, torch.equal(out_c, out_f), pass_bytes,
           copy_rate(lib, ext, pass_bytes // 16), pass_bytes)
    del in3, key, work, mid, out_c, out_f
    ext.close()
    data.close()


def lincomb(params, K, T):
    lib = _cabi.load()
    ctx = Context(params, 0)
    dev, L, n = ctx.device, params.n_limbs, params.n
    g = torch.Generator(device=dev).manual_seed(9)
    x = words(g, params.moduli, (K, T, 2), n, dev)                      # term-major, the fused entry's layout
    x_tok = x.permute(1, 0, 2, 3, 4).contiguous()                       # token-major: the K columns of one dpfhe_matvec_scalar per token
    q = torch.tensor(params.moduli, dtype=torch.int64, device=dev)
    w = torch.randint(0, 2 ** 62, (K + 1, L), generator=g, dtype=torch.int64, device=dev) % q
    w[K] = 0                                                            # (the composed form has no constant)
    w_cols = w[:K].contiguous().view(1, K, L)
    full = torch.empty((T, 2, L, n), dtype=torch.int64, device=dev)
    out_c = torch.empty((T, 2, L - 1, n), dtype=torch.int64, device=dev)
    out_f = torch.empty_like(out_c)

    def composed():
        for t in range(T):
            _cabi.check(lib.dpfhe_matvec_scalar(ctx.handle, full[t].data_ptr(), w_cols.data_ptr(), x_tok[t].data_ptr(), 1, K, None), "dpfhe_matvec_scalar")
        _cabi.check(lib.dpfhe_rescale(ctx.handle, out_c.data_ptr(), full.data_ptr(), T * 2, None), "dpfhe_rescale")

    def fused():
        _cabi.check(lib.dpfhe_lincomb_rescale(ctx.handle, out_f.data_ptr(), x.data_ptr(), w.data_ptr(), K, T, None), "dpfhe_lincomb_rescale")
    ms = alternate({"composed": composed, "fused": fused})
    pass_bytes = T * 2 * n * (K * L + L - 1) * 8                        # every term read once on every limb, L - 1 limbs written
    report("dpfhe_lincomb_rescale", {"log2_n": params.log2_n, "limbs": L, "terms": K, "tokens": T}, ms, torch.equal(out_c, out_f), pass_bytes,
           copy_rate(lib, ctx, pass_bytes // 16), pass_bytes)
    ctx.close()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if MODE == "quick":
        relin(ntt_primes(12, 4), 4)
        lincomb(ntt_primes(12, 3), 4, 2)
    elif MODE == "relin13":
        relin(FheParams.n8192_l6(), 64)
    elif MODE == "relin15":
        relin(FheParams.n32768(7), 8)
    else:
        relin(FheParams.n8192_l6(), 64)
        relin(FheParams.n32768(7), 8)
        for K in (4, 15):
            lincomb(FheParams.n32768(4), K, 8)                          # the sum level of a polynomial at the FFN example's ring: 4 limbs -> 3
            lincomb(FheParams.n8192(4), K, 8)
