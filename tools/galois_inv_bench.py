"""dpfhe_ntt_inv_galois against dpfhe_ntt_inv on the same buffer (HIP events): at N = 32768, where the Galois inverse is the split form (sub-transforms that gather
from another sub-block + the column stages; in place through the scratch arena), beside the same pair at N = 16384 (one kernel each), in one run.
1536 residue polynomials (64 elements x 8 RNS polynomials x 3 fold limbs), g = 3; median of 5 alternated regions of `reps` calls each.
usage: python tools/galois_inv_bench.py [reps=20]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deeppowers_amd.evaluator import Context, Evaluator  # noqa: E402
from deeppowers_amd.params import ntt_primes  # noqa: E402


def region(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / reps


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    k, per = 64, 8
    ratios = {}
    for ln in (14, 15):
        p = ntt_primes(ln, 3)
        ctx = Context(p, 0)
        assert ctx.uses_fold
        ev = Evaluator(ctx)
        L, n = p.n_limbs, p.n
        q = torch.tensor(p.moduli, dtype=torch.int64, device=ctx.device).view(1, 1, L, 1)
        x = torch.randint(0, 2**62, (k, per, L, n), dtype=torch.int64, device=ctx.device) % q
        y = torch.empty_like(x)
        elts = [3] * k
        forms = {"ntt_inv in place": lambda: ev.ntt_inverse_(x), "ntt_inv_galois in place": lambda: ev.ntt_inverse_galois(x, elts, out=x),
                 "ntt_inv_galois out of place": lambda: ev.ntt_inverse_galois(x, elts, out=y)}
        for fn in forms.values():
            fn(); fn()
        torch.cuda.synchronize()
        ts = {name: [] for name in forms}
        for _ in range(5):
            for name, fn in forms.items():
                ts[name].append(region(fn, reps))
        med = {name: sorted(v)[2] for name, v in ts.items()}
        words = k * per * L * n
        for name in forms:
            # one kernel (N <= 16384): a read and a write of every word; split (above): the sub-transforms and the column stages read and write them once each
            passes = 2 if ln <= 14 else 4
            print(f"N = {n}: {name:28s} median {med[name]:8.1f} us  (regions {' '.join(f'{t:.1f}' for t in ts[name])})  {passes * words * 8 / med[name] / 1e6:5.2f} TB/s at {passes} N words per polynomial")
        ratios[ln] = (med["ntt_inv_galois in place"] / med["ntt_inv in place"], med["ntt_inv_galois out of place"] / med["ntt_inv in place"])
        print(f"N = {n}: ntt_inv_galois / ntt_inv = {ratios[ln][0]:.3f} in place, {ratios[ln][1]:.3f} out of place; scratch held {ctx.scratch_bytes >> 20} MiB")
        ctx.close()
    lim = [r * 1.10 for r in ratios[14]]
    print(f"N = 32768 against the N = 16384 ratio + 10 %: in place {ratios[15][0]:.3f} (limit {lim[0]:.3f}), out of place {ratios[15][1]:.3f} (limit {lim[1]:.3f})")


if __name__ == "__main__":
    main()
