"""Same-process A/B timing of the rotate-and-add ladder (tool, not on the product path; MEASUREMENTS.md "Slot sums"): the 10-step ladder of a sum over
blocks of 1024 slots, 8 tokens,
  fused     one dpfhe_rotate_add_hybrid
  composed  per step dpfhe_rotate_hybrid_grouped (one element, the 8 tokens in its group) + dpfhe_add - the entries a caller had before
at N = 8192, Ld = 4 + P and at N = 32768, Ld = 7 + P.  Both routes are warmed up and give the same words (asserted before anything is timed); then they
alternate, WINDOWS windows each, a window being enough back-to-back ladders between two device events to last at least WINDOW_SECONDS.  Per route the median
window, the fastest and the slowest, in milliseconds per ladder; the ratio of the medians; the spread of the composed route is the noise a difference has to
exceed.  One JSON line per shape.
usage: python tools/slot_sum_bench.py [windows = 20] [window_seconds = 0.5] [quick]      (quick: N = 4096, Ld = 2, a rehearsal)"""
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deeppowers_amd import _cabi  # noqa: E402
from deeppowers_amd.evaluator import Context  # noqa: E402
from deeppowers_amd.params import FheParams, ntt_primes  # noqa: E402

WINDOWS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
WINDOW_SECONDS = float(sys.argv[2]) if len(sys.argv) > 2 else 0.5
QUICK = len(sys.argv) > 3 and sys.argv[3] == "quick"
STEPS, TOKENS = 10, 8


def words(gen, moduli, lead, n, dev):
    q = torch.tensor(moduli, dtype=torch.int64, device=dev).view(-1, 1)
    return torch.randint(0, 2 ** 62, tuple(lead) + (len(moduli), n), generator=gen, dtype=torch.int64, device=dev) % q


def timed(f, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def ladder(ext_params):
    lib = _cabi.load()
    ext = Context(ext_params, 0)
    data = Context(ext_params.drop_last_limb(), 0)
    dev, L, Ld, n, T = ext.device, ext_params.n_limbs, ext_params.n_limbs - 1, ext_params.n, TOKENS
    g = torch.Generator(device=dev).manual_seed(11)
    x = words(g, ext_params.moduli[:Ld], (T, 2), n, dev)
    keys = words(g, ext_params.moduli, (STEPS, Ld, 2), n, dev)
    elts = [pow(3, 1 << e, 2 * n) for e in range(STEPS)]
    c_elts = (C.c_uint32 * STEPS)(*elts)
    one = [(C.c_uint32 * 1)(e) for e in elts]
    new = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)
    work, acc, out_f = new(T, 2, L, n), new(T, 2, Ld, n), new(T, 2, Ld, n)
    rot, rotated, ping, out_c = new(T, 2, Ld, n), new(T, 2, Ld, n), new(T, 2, Ld, n), new(T, 2, Ld, n)

    def fused():
        _cabi.check(lib.dpfhe_rotate_add_hybrid(ext.handle, out_f.data_ptr(), x.data_ptr(), c_elts, keys.data_ptr(), work.data_ptr(), acc.data_ptr(), STEPS, T, None),
                    "dpfhe_rotate_add_hybrid")

    def composed():
        cur = x
        for e in range(STEPS):
            dst = ping if (STEPS - 1 - e) & 1 else out_c
            _cabi.check(lib.dpfhe_rotate_hybrid_grouped(ext.handle, rot.data_ptr(), cur.data_ptr(), one[e], 1, T, keys[e].data_ptr(), work.data_ptr(), rotated.data_ptr(),
                                                        None), "dpfhe_rotate_hybrid_grouped")
            _cabi.check(lib.dpfhe_add(data.handle, dst.data_ptr(), cur.data_ptr(), rot.data_ptr(), T * 2, None), "dpfhe_add")
            cur = dst
    routes = {"composed": composed, "fused": fused}
    for f in routes.values():
        f()
        f()
    torch.cuda.synchronize()
    assert torch.equal(out_f, out_c), "the two routes differ"
    reps = {name: max(1, int(WINDOW_SECONDS * 1e3 / timed(f, 3)) + 1) for name, f in routes.items()}
    ms = {name: [] for name in routes}
    for _ in range(WINDOWS):
        for name, f in routes.items():
            ms[name].append(timed(f, reps[name]))
    row = {"entry": "dpfhe_rotate_add_hybrid", "log2_n": ext_params.log2_n, "data_limbs": Ld, "tokens": T, "steps": STEPS, "windows": WINDOWS,
           "window_seconds": WINDOW_SECONDS, "same_words": True}
    for name, v in ms.items():
        v.sort()
        row[name + "_ms"] = {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4), "ladders_per_window": reps[name]}
    comp, fus = ms["composed"], ms["fused"]
    row["fused_over_composed"] = round(fus[len(fus) // 2] / comp[len(comp) // 2], 4)
    row["composed_spread"] = round((comp[-1] - comp[0]) / comp[len(comp) // 2], 4)
    row["fused_spread"] = round((fus[-1] - fus[0]) / fus[len(fus) // 2], 4)
    print(json.dumps(row), flush=True)
    ext.close()
    data.close()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if QUICK:
        ladder(ntt_primes(12, 3))
    else:
        ladder(FheParams.n8192(5))
        ladder(FheParams.n32768(8))
