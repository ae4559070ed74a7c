"""Same-process timing of a hoisted slot-sum stage on Ld = 12 data limbs (tool, not on the product path; MEASUREMENTS.md "Hoisted slot sums on grouped digits"):
  hoisted       dpfhe_rotate_sum_hoisted: one special prime, 12 digits (context Ld + 1) - the yardstick
  grouped_a     dpfhe_rotate_sum_hoisted_grouped at alpha = 1, 3, 4 (contexts Ld + alpha; 12, 4, 3 digit groups)
at N = 8192 and N = 32768, R = 1 and 7 rotations, 8 and 36 items; the same data limbs and the same items on every route (the pinned N = 32768 chain is too short
for alpha > 2: the primes are ntt_primes', ascending, the special ones the largest, as in tools/switch_key_grouped_bench.py).  Random canonical words and keys: a
timing, the words are held to Python integers by the tests.  Every route is warmed up (the grouped ones by their n_items == 0 call as well); then they alternate,
WINDOWS windows each, a window being enough back-to-back calls between two device events to last at least WINDOW_SECONDS.  Per route the median window, the
fastest and the slowest, in milliseconds per call, and its ratio to `hoisted`.  One JSON line per cell, also appended to profiles/r27_rotate_sum_grouped.txt.
`trace`: instead, TRACE_CALLS calls of every route per cell, route after route, and one JSON line per cell naming that order - the run to put under a kernel
trace.  `report KERNEL_TRACE.csv`: reads that trace (columns Kernel_Name, Start_Timestamp, End_Timestamp), takes the sum kernels' dispatches in start order, TRACE_CALLS
per route in the order `trace` ran them, and appends the median sum-kernel time per route and its ratio to `hoisted` (no device needed).
usage: python tools/rotate_sum_grouped_bench.py [windows = 10] [window_seconds = 0.3] [quick | trace | report CSV]      (quick: N = 4096, Ld = 4, a rehearsal)"""
import csv
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOWS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
WINDOW_SECONDS = float(sys.argv[2]) if len(sys.argv) > 2 else 0.3
MODE = sys.argv[3] if len(sys.argv) > 3 else ""
OUT = os.path.join(ROOT, "profiles", "r27_rotate_sum_grouped.txt")
ALPHAS, TRACE_CALLS = (1, 3, 4), 5
ROUTES = ["hoisted"] + [f"grouped_{a}" for a in ALPHAS]
CELLS = [(12, 4, R, T) for R in (1, 3) for T in (5,)] if MODE == "quick" else [(ln, 12, R, T) for ln in (13, 15) for R in (1, 7) for T in (8, 36)]


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def report(path):
    """the sum kernels of a `trace` run, in start order: per cell and route TRACE_CALLS dispatches"""
    rows = [r for r in csv.DictReader(open(path)) if "hoisted_qp_sum" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == len(CELLS) * len(ROUTES) * TRACE_CALLS, (len(rows), "sum-kernel dispatches; expected", len(CELLS) * len(ROUTES) * TRACE_CALLS)
    it = iter(rows)
    for log2n, Ld, R, T in CELLS:
        row = {"mode": "sum kernel alone (kernel trace)", "log2_n": log2n, "data_limbs": Ld, "rotations": R, "items": T, "calls": TRACE_CALLS}
        for name in ROUTES:
            took = [next(it) for _ in range(TRACE_CALLS)]
            assert all(("grouped" in r["Kernel_Name"]) == (name != "hoisted") for r in took), name
            us = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in took)
            row[name + "_kernel_us"] = {"median": round(us[len(us) // 2], 1), "min": round(us[0], 1), "max": round(us[-1], 1)}
        for name in ROUTES[1:]:
            row[name + "_over_hoisted"] = round(row[name + "_kernel_us"]["median"] / row["hoisted_kernel_us"]["median"], 4)
        emit(row)


def cell(log2n, Ld, R, T):
    import torch
    from deeppowers_amd import _cabi
    from deeppowers_amd.evaluator import Context
    from deeppowers_amd.params import FheParams, ntt_primes
    lib, n = _cabi.load(), 1 << log2n

    def chain(alpha):
        """Ld + alpha primes, ascending: the data limbs are the same at every alpha, the special ones the largest (P >= every D_d)"""
        p = ntt_primes(log2n, Ld + 4)
        pairs = sorted(zip(p.moduli, p.psi))
        pairs = pairs[:Ld] + pairs[len(pairs) - alpha:]
        return FheParams(log2n, tuple(q for q, _ in pairs), tuple(w for _, w in pairs))

    ctxs = {a: Context(chain(a), 0) for a in sorted(set(ALPHAS) | {1})}
    dev = ctxs[1].device
    g = torch.Generator(device=dev).manual_seed(27)
    new = lambda *s: torch.empty(s, dtype=torch.int64, device=dev)

    def words(moduli, lead):
        q = torch.tensor(moduli, dtype=torch.int64, device=dev).view(-1, 1)
        return torch.randint(0, 2 ** 62, tuple(lead) + (len(moduli), n), generator=g, dtype=torch.int64, device=dev) % q

    x, out, in_ntt = words(ctxs[1].params.moduli[:Ld], (T, 2)), new(T, 2, Ld, n), new(T, 2, Ld, n)
    elts = (C.c_uint32 * R)(*[pow(3, 1 + 2 * i, 2 * n) for i in range(R)])
    routes = {}

    key1, digits1, sum1 = words(ctxs[1].params.moduli, (R, Ld, 2)), new(T, Ld, Ld + 1, n), new(T, 2, Ld + 1, n)
    routes["hoisted"] = lambda: _cabi.check(lib.dpfhe_rotate_sum_hoisted(ctxs[1].handle, out.data_ptr(), x.data_ptr(), T, elts, key1.data_ptr(), R, in_ntt.data_ptr(),
                                                                         digits1.data_ptr(), sum1.data_ptr(), None), "dpfhe_rotate_sum_hoisted")

    def grouped(a):
        c, L, G = ctxs[a], Ld + a, -(-Ld // a)
        key, digits, sums = words(c.params.moduli, (R, G, 2)), new(T, G, L, n), new(T, 2, L, n)
        _cabi.check(lib.dpfhe_rotate_sum_hoisted_grouped(c.handle, None, None, 0, a, None, None, 1, None, None, None, None), "warm-up")
        return lambda: _cabi.check(lib.dpfhe_rotate_sum_hoisted_grouped(c.handle, out.data_ptr(), x.data_ptr(), T, a, elts, key.data_ptr(), R, in_ntt.data_ptr(),
                                                                        digits.data_ptr(), sums.data_ptr(), None), "dpfhe_rotate_sum_hoisted_grouped")
    for a in ALPHAS:
        routes[f"grouped_{a}"] = grouped(a)
    assert list(routes) == ROUTES

    def timed(f, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    row = {"log2_n": log2n, "data_limbs": Ld, "rotations": R, "items": T}
    if MODE == "trace":
        for f in routes.values():      # route after route: the first calls of each are its warm-up, the median of TRACE_CALLS passes them by
            for _ in range(TRACE_CALLS):
                f()
            torch.cuda.synchronize()
        emit(dict(row, mode="trace", order=ROUTES, calls=TRACE_CALLS))
    else:
        for f in routes.values():
            f()
            f()
        torch.cuda.synchronize()
        reps = {name: max(1, int(WINDOW_SECONDS * 1e3 / timed(f, 3)) + 1) for name, f in routes.items()}
        ms = {name: [] for name in routes}
        for _ in range(WINDOWS):
            for name, f in routes.items():
                ms[name].append(timed(f, reps[name]))
        row.update(windows=WINDOWS, window_seconds=WINDOW_SECONDS)
        for name, v in ms.items():
            v.sort()
            row[name + "_ms"] = {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4), "calls_per_window": reps[name]}
        for name in ROUTES[1:]:
            row[name + "_over_hoisted"] = round(row[name + "_ms"]["median"] / row["hoisted_ms"]["median"], 4)
        emit(row)
    for c in ctxs.values():
        c.close()


if __name__ == "__main__":
    if MODE == "report":
        report(sys.argv[4])
    else:
        import torch
        assert torch.cuda.is_available(), "a measurement needs the GPU"
        for shape in CELLS:
            cell(*shape)
