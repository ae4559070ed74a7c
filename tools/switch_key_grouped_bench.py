"""Same-process timing of a relinearisation on Ld = 12 data limbs (tool, not on the product path; MEASUREMENTS.md "Key switching with grouped digits"):
  hybrid        dpfhe_relinearize_hybrid: one special prime, 12 digits (context Ld + 1)
  grouped_a     dpfhe_switch_key_grouped at alpha = 2, 3, 4 (contexts Ld + alpha, in_components = 3)
  composed_4    the six-entry composition the header names, at alpha = 4: dpfhe_base_extend per group, dpfhe_ntt_fwd, dpfhe_dyadic_mul / _mul_add,
                dpfhe_ntt_inv, dpfhe_scale_round, dpfhe_add (the key pre-expanded over the items outside the timing: the dyadic entries take equal shapes)
at N = 8192 and N = 32768, 8 and 64 items.  Random canonical words and keys: a timing, the words are held to Python integers by the tests.  Every route is
warmed up; then they alternate, WINDOWS windows each, a window being enough back-to-back calls between two device events to last at least WINDOW_SECONDS.
Per route the median window, the fastest and the slowest, in milliseconds per call, and its ratio to `hybrid`.  One JSON line per shape, also appended to
profiles/r26_switch_key_grouped.txt.
`trace`: instead, 10 calls of the new entry at alpha = 4 and of the hybrid entry per shape and nothing else - the run to put under a kernel trace for the share of
time per stage; `trace LOG2N ITEMS` runs that one shape.
usage: python tools/switch_key_grouped_bench.py [windows = 10] [window_seconds = 0.5] [quick | trace [log2n items]]      (quick: N = 4096, Ld = 4, a rehearsal)"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deeppowers_amd import _cabi  # noqa: E402
from deeppowers_amd.evaluator import Context  # noqa: E402
from deeppowers_amd.params import FheParams, ntt_primes  # noqa: E402

WINDOWS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
WINDOW_SECONDS = float(sys.argv[2]) if len(sys.argv) > 2 else 0.5
MODE = sys.argv[3] if len(sys.argv) > 3 else ""
OUT = os.path.join(ROOT, "profiles", "r26_switch_key_grouped.txt")


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


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def chain(log2n, Ld, alpha):
    """Ld + alpha primes, ascending: the data limbs are the same at every alpha, the special ones the largest (P >= every D_d)"""
    p = ntt_primes(log2n, Ld + 4)
    pairs = sorted(zip(p.moduli, p.psi))
    pairs = pairs[:Ld] + pairs[len(pairs) - alpha:]
    return FheParams(log2n, tuple(q for q, _ in pairs), tuple(w for _, w in pairs))


def shape(log2n, Ld, T):
    lib = _cabi.load()
    n = 1 << log2n
    ctxs = {a: Context(chain(log2n, Ld, a), 0) for a in (1, 2, 3, 4)}
    data = Context(FheParams(log2n, ctxs[1].params.moduli[:Ld], ctxs[1].params.psi[:Ld]), 0)
    dev = data.device
    g = torch.Generator(device=dev).manual_seed(26)
    new = lambda *s: torch.empty(s, dtype=torch.int64, device=dev)
    x = words(g, data.params.moduli, (T, 3), n, dev)
    out = new(T, 2, Ld, n)
    routes = {}

    key1, work1 = words(g, ctxs[1].params.moduli, (Ld, 2), n, dev), new(T, 2, Ld + 1, n)
    routes["hybrid"] = lambda: _cabi.check(lib.dpfhe_relinearize_hybrid(ctxs[1].handle, out.data_ptr(), x.data_ptr(), key1.data_ptr(), work1.data_ptr(), T, None),
                                           "dpfhe_relinearize_hybrid")

    def grouped(a):
        c, L, G = ctxs[a], Ld + a, -(-Ld // a)
        key, digits, work = words(g, c.params.moduli, (G, 2), n, dev), new(T, G, L, n), new(T, 2, L, n)
        return lambda: _cabi.check(lib.dpfhe_switch_key_grouped(c.handle, out.data_ptr(), x.data_ptr(), 3, a, key.data_ptr(), digits.data_ptr(), work.data_ptr(), T, None),
                                   "dpfhe_switch_key_grouped")

    def composed(a):
        c, L, G, h = ctxs[a], Ld + a, -(-Ld // a), ctxs[a].handle
        key = words(g, c.params.moduli, (G, 2), n, dev)
        keyx = key[:, :, None].expand(G, 2, T, L, n).contiguous()
        lifted, acc, r, addend = new(G, T, L, n), new(2, T, L, n), new(2, T, Ld, n), x[:, :2].transpose(0, 1).contiguous()
        ck = _cabi.check

        def run():
            for d in range(G):
                s0, ns = d * a, min(a, Ld - d * a)
                ck(lib.dpfhe_base_extend(h, lifted[d].data_ptr(), L, x[0, 2, s0].data_ptr(), 3 * Ld, s0, ns, 0, L, T, None), "dpfhe_base_extend")
            ck(lib.dpfhe_ntt_fwd(h, lifted.data_ptr(), G * T, None), "dpfhe_ntt_fwd")      # (counts are RNS polynomials of L limbs)
            for comp in range(2):
                for d in range(G):
                    fn = lib.dpfhe_dyadic_mul if d == 0 else lib.dpfhe_dyadic_mul_add
                    ck(fn(h, acc[comp].data_ptr(), lifted[d].data_ptr(), keyx[d, comp].data_ptr(), T, None), "dpfhe_dyadic_mul")
            ck(lib.dpfhe_ntt_inv(h, acc.data_ptr(), 2 * T, None), "dpfhe_ntt_inv")
            ck(lib.dpfhe_scale_round(h, r.data_ptr(), Ld, acc.data_ptr(), Ld, a, 0, Ld, 1, 2 * T, None), "dpfhe_scale_round")
            ck(lib.dpfhe_add(data.handle, r.data_ptr(), r.data_ptr(), addend.data_ptr(), 2 * T, None), "dpfhe_add")
        return run

    if MODE == "trace":
        f = grouped(4)
        for _ in range(10):
            f()
            routes["hybrid"]()
        torch.cuda.synchronize()
        emit({"mode": "trace", "log2_n": log2n, "data_limbs": Ld, "items": T, "alpha": 4, "calls": 10})
    else:
        for a in (2, 3, 4):
            routes[f"grouped_{a}"] = grouped(a)
        routes["composed_4"] = composed(4)
        for f in routes.values():
            f()
            f()
        torch.cuda.synchronize()
        reps = {name: max(1, int(WINDOW_SECONDS * 1e3 / timed(f, 3)) + 1) for name, f in routes.items()}
        ms = {name: [] for name in routes}
        for _ in range(WINDOWS):
            for name, f in routes.items():
                ms[name].append(timed(f, reps[name]))
        row = {"log2_n": log2n, "data_limbs": Ld, "items": T, "windows": WINDOWS, "window_seconds": WINDOW_SECONDS}
        for name, v in ms.items():
            v.sort()
            row[name + "_ms"] = {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4), "calls_per_window": reps[name]}
        for name in routes:
            if name != "hybrid":
                row[name + "_over_hybrid"] = round(row[name + "_ms"]["median"] / row["hybrid_ms"]["median"], 4)
        emit(row)
    for c in list(ctxs.values()) + [data]:
        c.close()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    if MODE == "quick":
        shape(12, 4, 5)
    elif MODE == "trace" and len(sys.argv) > 5:
        shape(int(sys.argv[4]), 12, int(sys.argv[5]))
    else:
        for log2n in (13, 15):
            for T in (8, 64):
                shape(log2n, 12, T)
